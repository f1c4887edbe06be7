"""The motion descriptors of flows on the device (dfx_flow_hist_device, denseflow_amd/csrc/flow_hist_kernels.hip) against their
NumPy reference (tests/flow_hist_ref.py): the integer sums exactly, the float values bit for bit.  Sizes are the smallest at
which the kernel can go wrong — one pixel, a row shorter than a lane's four pixels, one cell, ragged cells, the sizes around the
256-pixel workgroup and the 32 rows a workgroup walks with W not a multiple of 4, a third workgroup column — at every cell
size, in both access widths: a 16-byte-aligned layout and one a single element off (single-element loads).  The padding of the
flows is NaN and that of the masks 0xFF, so a read of it would show in a sum; the guard bands and the gaps around both outputs
must stay as they were."""
import numpy as np
import pytest

from tests import flow_hist_ref as R
from tests.devmem import DevBuf
from tests.fb_check_ref import smooth_flow
from tests.flow_colour_ref import plant_specials

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (3, 2), (4, 4), (5, 7), (255, 31), (256, 32), (257, 33), (260, 65), (520, 36)]
MEMS = ["vector", "scalar"]
GUARD = 64  # elements in front of and behind every output buffer
OUT_FILL = np.array([0x7FC12345], np.uint32).view(F32)[0]  # a NaN with a payload: recognised by its bits
SUMS_FILL = np.int64(-0x0101010101010102)
OUTS = {"both": (True, True), "sums": (True, False), "out": (False, True)}
# (kinds, bins, norm, still_thr, outputs): all seven kinds, bins 2 / 8 / 9 / 16, all four norms, every choice of outputs
COMBOS = [(7, 8, "none", 0.4, "both"), (1, 2, "l1", -1.0, "out"), (2, 9, "l2", 0.4, "sums"), (3, 16, "l1_sqrt", 0.4, "both"),
          (4, 8, "l2", 0.4, "out"), (5, 9, "l1", 2.0, "both"), (6, 2, "l1_sqrt", 0.4, "both"), (7, 16, "l2", 1.0, "both")]

_case_cache = {}


def _case(w, h, n, cell):
    """Flows and masks of one (size, n, cell), computed once and never changed: smooth fields, the special values planted in
    the last flow; a mask over about a fifth of the pixels that also leaves cell (0, 0) of flow 0 empty."""
    key = (w, h, n, cell)
    if key not in _case_cache:
        rng = np.random.default_rng(1000 * w + 10 * h + n)
        flows = smooth_flow(rng, n, h, w, 6.0)
        plant_specials(flows[-1])
        mask = (rng.random((n, h, w)) < 0.2).astype(np.uint8) * rng.integers(1, 256, (n, h, w)).astype(np.uint8)
        mask[0, :cell, :cell] = 255
        for a in (flows, mask):
            a.setflags(write=False)
        _case_cache[key] = (flows, mask)
    return _case_cache[key]


def _up4(v):
    return (v + 3) // 4 * 4


def _flow_geom(mem, w, h):
    """(lead floats, row pitch, plane stride, flow stride) as tests/test_flow_colour_gpu.py lays flows out."""
    p3, p4 = w + 3, _up4(w) + 4
    return {"scalar": (1, p3, h * p3 + 5, 2 * (h * p3 + 5) + 7),  # a base one float in, odd pitches: single elements
            "vector": (0, p4, h * p4 + 8, 2 * (h * p4 + 8) + 12)}[mem]  # everything a multiple of 4 floats


def _mask_geom(mem, w, h):
    """(lead bytes, pitch, stride)."""
    if mem == "scalar":
        pitch = (w + 2) | 1
        return 1, pitch, h * pitch + 3
    pitch = _up4(w) + 4
    return 0, pitch, h * pitch + 4


def _pack_flows(flows, geom):
    lead, pitch, plane, stride = geom
    n, _, h, w = flows.shape
    buf = np.full(lead + n * stride + 4, np.nan, F32)  # NaN padding: a read of it would show
    for i in range(n):
        for p in range(2):
            o = lead + i * stride + p * plane
            buf[o:o + h * pitch].reshape(h, pitch)[:, :w] = flows[i, p]
    return buf


def _pack_mask(mask, geom):
    lead, pitch, stride = geom
    n, h, w = mask.shape
    buf = np.full(lead + n * stride + 4, 0xFF, np.uint8)  # 0xFF padding: masked if read
    for i in range(n):
        o = lead + i * stride
        buf[o:o + h * pitch].reshape(h, pitch)[:, :w] = mask[i]
    return buf


def _out_geom(mem, n, D, CH, CW):
    """(lead, slot, col, row, flow strides in floats, extent): "vector": (n, D, CH, CW) with padded rows and planes; "scalar":
    (n, CH, CW, D) with padded cells, one float in."""
    if mem == "vector":
        col, row = 1, CW + 3
        slot = CH * row + 5
        flow = D * slot + 7
        return 0, slot, col, row, flow, n * flow
    slot, col = 1, D + 2
    row = CW * col + 3
    flow = CH * row + 1
    return 1, slot, col, row, flow, 1 + n * flow


class _Resident:
    """The inputs of a case on the device in one memory layout, uploaded once."""

    def __init__(self, eng, mem, flows, mask):
        self.eng, self.mem = eng, mem
        self.n, _, self.h, self.w = flows.shape
        self.fgeom, self.mgeom = _flow_geom(mem, self.w, self.h), _mask_geom(mem, self.w, self.h)
        self.d_flow = DevBuf(eng, init=_pack_flows(flows, self.fgeom))
        self.d_mask = DevBuf(eng, init=_pack_mask(mask, self.mgeom))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.d_flow.close()
        self.d_mask.close()

    def run(self, kinds, cell, bins, thr, norm, masked, outs="both"):
        """(values (n, D, CH, CW) or None, sums (n, CH, CW, D) or None); checks the guard bands and the gaps."""
        eng, n, w, h = self.eng, self.n, self.w, self.h
        CH, CW, D = -(-h // cell), -(-w // cell), R.slots(kinds, bins)
        want_sums, want_out = OUTS[outs]
        lead, s_slot, s_col, s_row, s_flow, extent = _out_geom(self.mem, n, D, CH, CW)
        sums_stride = CH * CW * D + (3 if self.mem == "scalar" else 0)
        out_host = np.full(2 * GUARD + extent, OUT_FILL, F32)
        sums_host = np.full(2 * GUARD + n * sums_stride, SUMS_FILL, np.int64)
        fl, rp, ps, fs = self.fgeom
        ml, mp, ms = self.mgeom
        with DevBuf(eng, init=out_host) as d_out, DevBuf(eng, init=sums_host) as d_sums:
            eng.flow_hist_device(self.d_flow.ptr(4 * fl), rp, ps, fs, n, kinds, cell, bins, thr, R.NORMS[norm],
                                 d_sums.ptr(8 * GUARD) if want_sums else None, sums_stride,
                                 d_out.ptr(4 * (GUARD + lead)) if want_out else None, s_slot, s_col, s_row, s_flow,
                                 self.d_mask.ptr(ml) if masked else None, mp, ms)
            out_buf, sums_buf = d_out.get(F32), d_sums.get(np.int64)
        fill_bits = np.array([OUT_FILL], F32).view(np.uint32)[0]
        vals = sums = None
        if want_out:
            idx = (GUARD + lead + np.arange(n)[:, None, None, None] * s_flow + np.arange(D)[None, :, None, None] * s_slot +
                   np.arange(CH)[None, None, :, None] * s_row + np.arange(CW)[None, None, None, :] * s_col)
            vals = out_buf[idx]
            rest = np.ones(out_buf.shape, bool)
            rest[idx.reshape(-1)] = False
            assert np.all(out_buf.view(np.uint32)[rest] == fill_bits), "a float outside d_out's elements was written"
        else:
            assert np.all(out_buf.view(np.uint32) == fill_bits), "d_out was written without being asked for"
        if want_sums:
            body = sums_buf[GUARD:GUARD + n * sums_stride].reshape(n, sums_stride)
            sums = body[:, :CH * CW * D].reshape(n, CH, CW, D).copy()
            assert np.all(body[:, CH * CW * D:] == SUMS_FILL) and np.all(sums_buf[:GUARD] == SUMS_FILL) and \
                np.all(sums_buf[GUARD + n * sums_stride:] == SUMS_FILL), "a word outside d_sums' elements was written"
        else:
            assert np.all(sums_buf == SUMS_FILL), "d_sums was written without being asked for"
        return vals, sums


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def _check(dev, flows, mask, kinds, cell, bins, thr, norm, masked, outs, ref=None, tag=""):
    vals_ref, sums_ref = ref or R.flow_hist(flows, kinds, cell, bins, thr, norm, mask if masked else None)
    vals, sums = dev.run(kinds, cell, bins, thr, norm, masked, outs)
    what = (tag, dev.mem, kinds, cell, bins, thr, norm, masked, outs)
    if sums is not None:
        bad = sums != sums_ref
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], sums[bad][:4], sums_ref[bad][:4])
    if vals is not None:
        bad = vals.view(np.uint32) != vals_ref.view(np.uint32)
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4], vals[bad][:4], vals_ref[bad][:4])
    return vals_ref, sums_ref


@pytest.mark.parametrize("cell", R.CELLS)
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_equals_the_reference_in_every_layout(dfx, w, h, cell):
    n = 3
    flows, mask = _case(w, h, n, cell)
    refs = {}
    with dfx.FlowEngine(w, h, "farn") as eng:
        for mem in MEMS:
            with _Resident(eng, mem, flows, mask) as dev:
                for masked in (False, True):
                    for kinds, bins, norm, thr, outs in COMBOS:
                        key = (masked, kinds, bins, norm, thr)
                        refs[key] = _check(dev, flows, mask, kinds, cell, bins, thr, norm, masked, outs, refs.get(key))
    sums = refs[(True, 7, 8, "none", 0.4)][1]
    assert not sums[0, 0, 0].any()  # the mask leaves that cell empty
    print(f"{w}x{h} cell {cell}: {sums.shape[1]} x {sums.shape[2]} cells, largest sum {sums.max()}")


def _special_flows(w, h):
    """0: the seam (u = -1, v = +0 / -0 alternating by rows); 1: subnormal flows; 2: random bit patterns; 3: the special
    values of the colour row, 1e9 among them, on a small smooth flow; 4: normal random vectors (the float64 normalisation
    meets sums without structure)."""
    rng = np.random.default_rng(99)
    fl = np.zeros((5, 2, h, w), F32)
    fl[0, 0] = -1.0
    fl[0, 1, 1::2] = -0.0
    tiny = np.nextafter(F32(0), F32(1))
    fl[1] = (rng.integers(-200, 200, (2, h, w)) * tiny).astype(F32)
    fl[2] = rng.integers(0, 1 << 32, (2, h, w), dtype=np.uint64).astype(np.uint32).view(F32)
    fl[3] = smooth_flow(rng, 1, h, w, 0.5)[0]
    plant_specials(fl[3])
    fl[4] = (rng.standard_normal((2, h, w)) * 5).astype(F32)
    return fl


@pytest.mark.parametrize("mem", MEMS)
def test_the_seam_subnormals_specials_and_random_bit_patterns(dfx, mem):
    w, h = 97, 61
    fl = _special_flows(w, h)
    rng = np.random.default_rng(3)
    mask = (rng.random((fl.shape[0], h, w)) < 0.1).astype(np.uint8)
    from tests.flow_colour_ref import known
    assert 0.2 < known(fl[2:3]).mean() < 0.9  # the random patterns are of both kinds
    with dfx.FlowEngine(w, h, "farn") as eng, _Resident(eng, mem, fl, mask) as dev:
        for cell, bins, norm, thr in ((4, 8, "l2", 0.4), (32, 9, "l1_sqrt", 0.0), (8, 16, "l1", -1.0), (16, 2, "none", 1e9)):
            for masked in (False, True):
                vals, sums = _check(dev, fl, mask, 7, cell, bins, thr, norm, masked, "both")
                assert np.isfinite(vals).all()
                if not masked and thr < 0:
                    hof = sums[0, ..., :bins]
                    assert hof[..., bins // 2].sum() == hof.sum() > 0  # both sides of the seam in one bin
                    assert not sums[1].any()  # subnormal vectors weigh nothing


@pytest.mark.parametrize("mem", MEMS)
def test_one_direction_and_alternating_directions(dfx, mem):
    """Every pixel of a cell into one slot — the worst case of the on-chip adds — and the four axis directions alternating
    pixel by pixel, where no two neighbours of a lane's quad share a slot."""
    w, h, n = 260, 65, 2
    fl = np.zeros((n, 2, h, w), F32)
    fl[0, 0], fl[0, 1] = 3.0, 0.0
    y, x = np.mgrid[:h, :w]
    d = (x + y) % 4
    fl[1, 0] = np.choose(d, [2.0, 0.0, -2.0, 0.0])
    fl[1, 1] = np.choose(d, [0.0, 2.0, 0.0, -2.0])
    mask = np.zeros((n, h, w), np.uint8)
    with dfx.FlowEngine(w, h, "farn") as eng, _Resident(eng, mem, fl, mask) as dev:
        for cell in R.CELLS:
            vals, sums = _check(dev, fl, mask, 7, cell, 8, 0.4, "l1", False, "both")
            full = sums[0, :h // cell, :w // cell]
            assert np.all(full[..., 0] == 3 * 256 * cell * cell) and not full[..., 1:].any()
            alt = sums[1, :h // cell, :w // cell, :8]
            assert np.all(alt[..., 0::2] == 2 * 256 * cell * cell // 4) and not alt[..., 1::2].any()
            assert sums[1, ..., 9:].any()


def _stats_bytes(eng):
    return bytes(eng.stats())


def test_every_refusal_returns_its_status_writes_nothing_and_leaves_the_handle_usable(dfx):
    w, h, n, cell, bins = 65, 17, 3, 8, 8
    flows, mask = _case(w, h, n, cell)
    CH, CW, D = 3, 9, 25
    vals_ref, sums_ref = R.flow_hist(flows, 7, cell, bins, 0.4, "l2", mask)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        with DevBuf(eng, init=flows) as d_f, DevBuf(eng, init=mask) as d_m, \
                DevBuf(eng, init=np.full(n * D * CH * CW, OUT_FILL, F32)) as d_out, \
                DevBuf(eng, init=np.full(n * CH * CW * D + 1, SUMS_FILL, np.int64)) as d_sums:
            good = dict(f=d_f.ptr(), rp=w, ps=h * w, fs=2 * h * w, n=n, kinds=7, cell=cell, bins=bins, thr=0.4, norm=3,
                        sums=d_sums.ptr(), ss=CH * CW * D, out=d_out.ptr(), o=(CH * CW, 1, CW, D * CH * CW), mask=d_m.ptr(),
                        mp=w, ms=h * w)

            def call(**kw):
                a = dict(good, **kw)
                eng.flow_hist_device(a["f"], a["rp"], a["ps"], a["fs"], a["n"], a["kinds"], a["cell"], a["bins"], a["thr"],
                                     a["norm"], a["sums"], a["ss"], a["out"], *a["o"], a["mask"], a["mp"], a["ms"])

            def untouched():
                return np.all(d_out.get(F32).view(np.uint32) == np.array([OUT_FILL], F32).view(np.uint32)[0]) and \
                    np.all(d_sums.get(np.int64) == SUMS_FILL)

            bytes_before, stats_before = eng.device_bytes(), _stats_bytes(eng)
            refused = [dict(f=None), dict(sums=None, out=None), dict(n=-1), dict(kinds=0), dict(kinds=8), dict(kinds=-1),
                       dict(bins=1), dict(bins=17), dict(bins=0), dict(cell=0), dict(cell=2), dict(cell=12), dict(cell=64),
                       dict(cell=-8), dict(norm=-1), dict(norm=4), dict(thr=float("nan")), dict(thr=float("inf")),
                       dict(thr=float("-inf")), dict(rp=w - 1), dict(ps=h * w - 1), dict(fs=2 * h * w - 1), dict(mp=w - 1),
                       dict(ms=h * w - 1), dict(sums=d_sums.ptr(4)), dict(sums=d_sums.ptr(1), out=None),
                       dict(ss=CH * CW * D - 1), dict(kinds=1, ss=CH * CW * 9 - 1), dict(cell=4, ss=5 * 17 * D - 1)]
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    call(**kw)
                assert e.value.status == 1, kw
            assert untouched(), "a refused call wrote"
            call(n=0)  # DFX_OK, launches nothing
            call(n=0, f=None, sums=None, out=None, kinds=99, cell=5, bins=0, norm=9, thr=float("nan"))
            assert untouched(), "n = 0 wrote"
            call()
            assert _same_bits(d_out.get(F32).reshape(n, D, CH, CW), vals_ref), "the handle is not usable after the refusals"
            assert np.array_equal(d_sums.get(np.int64)[:-1].reshape(n, CH, CW, D), sums_ref)
            assert d_sums.get(np.int64)[-1] == SUMS_FILL
            call(thr=-1.0), call(thr=-3e38), call(sums=None), call(out=None, o=(0, 0, 0, 0)), call(mask=None, mp=0, ms=0)
            call(kinds=1, ss=CH * CW * 9), call(sums=d_sums.ptr(8))  # accepted
            assert eng.device_bytes() == bytes_before and _stats_bytes(eng) == stats_before
    with dfx.FlowEngine(w, h, "frames") as eng:
        with DevBuf(eng, init=flows) as d_f, DevBuf(eng, 4 * n * D * CH * CW) as d_out:
            with pytest.raises(dfx.DfxError) as e:
                eng.flow_hist_device(d_f.ptr(), w, h * w, 2 * h * w, n, 7, cell, bins, 0.4, 0, None, 0, d_out.ptr(), CH * CW, 1,
                                     CW, D * CH * CW)
            assert e.value.status == 4


@pytest.mark.parametrize("algo", ["tvl1", "brox"])
def test_numpy_wrapper_on_every_flow_handle(dfx, algo):
    w, h, n = 65, 17, 3
    flows, mask = _case(w, h, n, 8)
    with dfx.FlowEngine(w, h, algo) as eng:
        got = eng.flow_hist(flows)
        want, _ = R.flow_hist(flows)
        assert got.shape == (n, 25, 3, 9) and got.dtype == F32 and _same_bits(got, want)
        assert len(dfx.flow_hist_slots()) == 25
        got, sums = eng.flow_hist(flows, ("hof", "mbhy"), 4, 9, 1.5, "l1_sqrt", mask, want_sums=True)
        want, want_sums = R.flow_hist(flows, ("hof", "mbhy"), 4, 9, 1.5, "l1_sqrt", mask)
        assert got.shape == (n, 19, 5, 17) and _same_bits(got, want)
        assert sums.dtype == np.int64 and np.array_equal(sums, want_sums)
        assert _same_bits(eng.flow_hist(flows, "mbhx", 32, 2, norm="l2"), R.flow_hist(flows, "mbhx", 32, 2, norm="l2")[0])
        assert eng.flow_hist(flows[:0], "hof", 16).shape == (0, 9, 2, 5)


def test_the_tensor_wrapper_reads_and_writes_a_strided_slice_where_it_lies(dfx):
    import torch

    w, h, n, cell, bins = 65, 17, 3, 8, 8
    flows, mask = _case(w, h, n, cell)
    CH, CW, D = 3, 9, 25
    dev = torch.device("cuda:0")
    big = torch.full((n + 1, 2, h + 3, w + 5), float("nan"), device=dev)
    view = big[1:, :, 1:h + 1, 2:w + 2]
    view.copy_(torch.from_numpy(flows.copy()))
    bigmask = torch.full((n, h + 2, w + 7), 255, dtype=torch.uint8, device=dev)
    mview = bigmask[:, 1:h + 1, 3:w + 3]
    mview.copy_(torch.from_numpy(mask.copy()))
    with dfx.FlowEngine(w, h, "farn") as eng:
        for layout, norm in (("chw", "l2"), ("hwc", "l1")):
            want, want_sums = R.flow_hist(flows, 7, cell, bins, 0.4, norm, mask)
            got, sums = eng.flow_hist_tensor(view, cell=cell, bins=bins, norm=norm, mask=mview, want_sums=True, layout=layout)
            assert got.dtype == torch.float32 and got.is_contiguous()
            assert tuple(got.shape) == ((n, D, CH, CW) if layout == "chw" else (n, CH, CW, D))
            host = got.cpu().numpy()
            assert _same_bits(host if layout == "chw" else host.transpose(0, 3, 1, 2), want), layout
            assert sums.dtype == torch.int64 and np.array_equal(sums.cpu().numpy(), want_sums)
            # out=: a slice of a larger tensor, the rest of which stays as it was
            shape = (n + 1, D + 2, CH + 1, CW + 3) if layout == "chw" else (n + 1, CH + 1, CW + 3, D + 2)
            canvas = torch.full(shape, -7.5, device=dev)
            out = canvas[1:, 1:D + 1, :CH, 2:CW + 2] if layout == "chw" else canvas[1:, :CH, 2:CW + 2, 1:D + 1]
            res = eng.flow_hist_tensor(view, cell=cell, bins=bins, norm=norm, mask=mview, layout=layout, out=out)
            assert res is out
            host = canvas.cpu().numpy()
            window = host[1:, 1:D + 1, :CH, 2:CW + 2] if layout == "chw" else host[1:, :CH, 2:CW + 2, 1:D + 1]
            assert _same_bits(window if layout == "chw" else window.transpose(0, 3, 1, 2), want), layout
            window[...] = -7.5
            assert np.all(host == -7.5)
        assert eng.flow_hist_tensor(view[:0], "hof", 16).shape == (0, 9, 2, 5)
        assert eng.flow_hist_tensor(view[:0], "hof", 16, layout="hwc").shape == (0, 2, 5, 9)
