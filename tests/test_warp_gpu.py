"""The backward warp on the device (dfx_warp_device, denseflow_amd/csrc/warp_kernels.hip) against its NumPy reference
(tests/warp_ref.py): float outputs as bit patterns, u8 images, valid masks and statistics with np.array_equal.  Sizes are the
smallest at which the kernel can go wrong — one pixel, a row shorter than a lane's four pixels, odd widths with a ragged tail
over several row groups, and 261 x 5 for a second 256-pixel workgroup column; 97 x 61 and 130 x 97 are taller than the 32 rows
a workgroup of the statistics form walks and no multiple of them — in every layout that selects another access width: dense,
every base and pitch odd (single elements), everything 16-byte aligned (the wide accesses), and two mixtures of the two so
that no buffer's width depends on another's."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import warp_ref as R
from tests.devmem import DevBuf

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(1, 1), (3, 2), (65, 17), (97, 61), (130, 97), (261, 5)]
FULL = [(65, 17), (261, 5)]   # the full cross of every axis; the reduced set elsewhere
GUARD = 64                    # elements in front of and behind every output buffer
FILL = 0xA5                   # every byte of an output buffer before a call
STATS_FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
KINDS = ("gray", "bgr", "planar")  # (channels, layout): (1, -), (3, DFX_SRC_INTERLEAVED), (3, DFX_SRC_PLANAR)
CODES = {"float32": 0, "float16": 1, "bfloat16": 2, "uint8": 3}
NP_OF = {"float32": np.uint32, "float16": np.uint16, "bfloat16": np.uint16, "uint8": np.uint8}  # bit patterns
# which buffers are laid out how: (flow, source and reference, out, occ, valid), d = dense, s = single elements, v = wide
LAYOUTS = {"dense": "ddddd", "scalar": "sssss", "vector": "vvvvv", "mixed": "vsvsv", "mixed2": "svsvs"}

_case_cache = {}


def _case(w, h, n):
    """Inputs and references of one (size, n), computed once and never changed: uniform random bytes (smooth pictures hide
    tap mix-ups), smooth flows of up to half the frame with the special values planted in the last one, a random mask."""
    key = (w, h, n)
    if key not in _case_cache:
        seed = 1000 * w + 10 * h + n
        flows = R.warp_flow(np.random.default_rng(seed), n, h, w)
        R.plant_specials(flows[-1])
        rng = np.random.default_rng([seed, 1])
        src, ref = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        occ = (rng.random((n, h, w)) < 0.3).astype(np.uint8)
        inside = np.stack([R.inside_of(f) for f in flows])
        c = dict(w=w, h=h, n=n, flows=flows, src=src, ref=ref, occ=occ, inside=inside, s={})
        for ch in (1, 3):
            for border in R.BORDERS:
                c["s"][ch, border] = R.warp_batch(src if ch == 3 else src[..., 0], flows, border)[0]
        for a in [flows, src, ref, occ, inside] + list(c["s"].values()):
            a.setflags(write=False)
        _case_cache[key] = c
    return _case_cache[key]


def _planes(c, kind, a):
    """An (n, H, W, 3) array in the (n, P, H, RW) form of an image kind."""
    n, h, w = c["n"], c["h"], c["w"]
    if kind == "gray":
        return np.ascontiguousarray(a[..., 0] if a.ndim == 4 else a).reshape(n, 1, h, w)
    if kind == "bgr":
        return np.ascontiguousarray(a).reshape(n, 1, h, 3 * w)
    return np.ascontiguousarray(a.transpose(0, 3, 1, 2))


def _want(c, kind, border, dtype, with_occ):
    """(out bit patterns (n, P, H, RW), valid (n, 1, H, W), stats (n, 2)) as the device must give them."""
    ch = 1 if kind == "gray" else 3
    s = c["s"][ch, border]
    valid = (c["inside"] & (c["occ"] == 0 if with_occ else True)).astype(np.uint8)
    ref = c["ref"][..., 0] if ch == 1 else c["ref"]
    stats = np.array([R.stats(s[i], ref[i], valid[i]) for i in range(c["n"])], np.uint64).reshape(c["n"], 2)
    out = R.stored(s, dtype)
    out = out.view(np.uint32) if dtype == "float32" else out
    return _planes(c, kind, out), valid.reshape(c["n"], 1, c["h"], c["w"]), stats


def _up4(v):
    return (v + 3) // 4 * 4


def _geom(how, p, h, rw):
    """(lead, pitch, plane stride, image stride) in elements of a buffer of n x p planes of h rows of rw elements."""
    if how == "d":
        return 0, rw, h * rw, p * h * rw
    if how == "s":  # a base one element in, an odd pitch: every access is a single element
        pitch = rw + 1 + rw % 2
        plane = h * pitch + 1
        return 1, pitch, plane, p * plane + 3
    pitch = _up4(rw) + 4  # everything a multiple of 4 elements from a 256-byte-aligned base: the wide accesses
    plane = h * pitch + 8
    return 0, pitch, plane, p * plane + 12


class _Buf:
    """A padded device buffer of n x p planes of h rows of rw elements of `dtype`, GUARD elements in front and behind."""

    def __init__(self, eng, how, n, p, h, rw, dtype, fill, data=None):
        self.eng, self.n, self.p, self.h, self.rw, self.dtype = eng, n, p, h, rw, np.dtype(dtype)
        self.lead, self.pitch, self.plane, self.image = _geom(how, p, h, rw)
        self.host = np.full(2 * GUARD + self.lead + n * self.image + 4, fill, self.dtype)
        self.outside = np.ones(self.host.shape, bool)
        for i in range(n):
            for k in range(p):
                o = GUARD + self.lead + i * self.image + k * self.plane
                if data is not None:
                    self.host[o:o + h * self.pitch].reshape(h, self.pitch)[:, :rw] = data[i, k]
                self.outside[o:o + h * self.pitch].reshape(h, self.pitch)[:, :rw] = False
        self.fill = self.host.copy()
        self.dev = DevBuf(eng, init=self.host)

    def ptr(self):
        return self.dev.ptr((GUARD + self.lead) * self.dtype.itemsize)

    def reset(self):
        self.eng._check(self.eng._L.dfx_memcpy_h2d(self.eng._h, self.dev.ptr(), self.fill.ctypes.data, self.fill.nbytes))

    def windows(self):
        """(the (n, p, h, rw) windows, whether everything outside them still holds the fill)."""
        buf = self.dev.get(self.dtype)
        wins = np.empty((self.n, self.p, self.h, self.rw), self.dtype)
        for i in range(self.n):
            for k in range(self.p):
                o = GUARD + self.lead + i * self.image + k * self.plane
                wins[i, k] = buf[o:o + self.h * self.pitch].reshape(self.h, self.pitch)[:, :self.rw]
        return wins, bool(np.all(buf[self.outside] == self.fill[self.outside]))

    def untouched(self):
        return bool(np.all(self.dev.get(self.dtype) == self.fill))

    def close(self):
        self.dev.close()


class _Rig:
    """The device buffers of one (case, layout, image kind): inputs uploaded once, one output buffer per type."""

    def __init__(self, eng, c, layout, kind):
        self.eng, self.c, self.kind = eng, c, kind
        n, h, w = c["n"], c["h"], c["w"]
        lf, ls, lo, lc, lv = LAYOUTS[layout]
        self.p, self.rw = {"gray": (1, w), "bgr": (1, 3 * w), "planar": (3, w)}[kind]
        self.flow = _Buf(eng, lf, n, 2, h, w, F32, np.nan, c["flows"])
        self.src = _Buf(eng, ls, n, self.p, h, self.rw, np.uint8, 0x5A, _planes(c, kind, c["src"]))
        self.ref = _Buf(eng, ls, n, self.p, h, self.rw, np.uint8, 0x3C, _planes(c, kind, c["ref"]))
        self.occ = _Buf(eng, lc, n, 1, h, w, np.uint8, 1, c["occ"].reshape(n, 1, h, w))
        self.valid = _Buf(eng, lv, n, 1, h, w, np.uint8, FILL)
        fill = {np.uint8: FILL, np.uint16: 0xA5A5, np.uint32: 0xA5A5A5A5}
        self.out = {d: _Buf(eng, lo, n, self.p, h, self.rw, NP_OF[d], fill[NP_OF[d]]) for d in CODES}
        self.stats_fill = np.full(2 * n + 4, STATS_FILL, np.uint64)
        self.stats = DevBuf(eng, init=self.stats_fill)
        self.bufs = [self.flow, self.src, self.ref, self.occ, self.valid] + list(self.out.values())

    def reset_stats(self):
        e = self.eng
        e._check(e._L.dfx_memcpy_h2d(e._h, self.stats.ptr(), self.stats_fill.ctypes.data, self.stats_fill.nbytes))

    def call(self, dtype_name, border_name, with_occ, want_out, want_valid, want_stats, **over):
        out = self.out[dtype_name]
        kw = dict(d_src_ptr=self.src.ptr(), channels=1 if self.kind == "gray" else 3, layout=1 if self.kind == "planar" else 0,
                  src_pitch=self.src.pitch, src_plane_stride=self.src.plane, src_image_stride=self.src.image,
                  d_flow_ptr=self.flow.ptr(), row_pitch_floats=self.flow.pitch, plane_stride_floats=self.flow.plane,
                  flow_stride_floats=self.flow.image, n=self.c["n"], border=R.BORDERS.index(border_name),
                  out_dtype=CODES[dtype_name],
                  d_out_ptr=out.ptr() if want_out else None, out_pitch=out.pitch, out_plane_stride=out.plane,
                  out_image_stride=out.image, d_ref_ptr=self.ref.ptr(),
                  d_occ_ptr=self.occ.ptr() if with_occ else None, occ_pitch=self.occ.pitch, occ_stride=self.occ.image,
                  d_valid_ptr=self.valid.ptr() if want_valid else None, valid_pitch=self.valid.pitch,
                  valid_stride=self.valid.image, d_stats_ptr=self.stats.ptr(16) if want_stats else None)
        kw.update(over)
        self.eng.warp_device(**kw)

    def check(self, dtype, border, with_occ, want_out, want_valid, want_stats, tag):
        """One call from fill patterns, everything it wrote against the reference, everything else against the fill."""
        out = self.out[dtype]
        out.reset(), self.valid.reset(), self.reset_stats()
        self.call(dtype, border, with_occ, want_out, want_valid, want_stats)
        ref_out, ref_valid, ref_stats = _want(self.c, self.kind, border, dtype, with_occ)
        if want_out:
            got, clean = out.windows()
            bad = got != ref_out
            assert not bad.any(), (tag, int(bad.sum()), got[bad][:4], ref_out[bad][:4])
            assert clean, (tag, "an element outside the windows of out was written")
        else:
            assert out.untouched(), (tag, "out was written without being asked for")
        if want_valid:
            got, clean = self.valid.windows()
            assert np.array_equal(got, ref_valid), tag
            assert clean, (tag, "a byte outside the windows of valid was written")
        else:
            assert self.valid.untouched(), (tag, "valid was written without being asked for")
        st = self.stats.get(np.uint64)
        if want_stats:
            assert np.array_equal(st[2:-2].reshape(-1, 2), ref_stats), (tag, st[2:-2], ref_stats.ravel())
            assert np.all(st[:2] == STATS_FILL) and np.all(st[-2:] == STATS_FILL), (tag, "a word next to the statistics was written")
            assert np.array_equal(ref_stats[:, 0], ref_valid.reshape(self.c["n"], -1).sum(axis=1).astype(np.uint64))
        else:
            assert np.all(st == STATS_FILL), (tag, "the statistics were written without being asked for")

    def close(self):
        for b in self.bufs:
            b.close()
        self.stats.close()


def _combos(full):
    """(kind, dtype, border, with_occ, want_out, want_valid, want_stats)."""
    if full:
        for kind in KINDS:
            for dtype in CODES:
                for border in R.BORDERS:
                    for bits in range(8):
                        yield kind, dtype, border, bool(bits & 1), True, bool(bits & 2), bool(bits & 4)
            for border in R.BORDERS:
                for with_occ in (False, True):
                    yield kind, "uint8", border, with_occ, False, False, True  # the statistics alone
                yield kind, "uint8", border, True, False, True, False          # the valid mask alone
        return
    # every value of every axis at least once
    yield "gray", "uint8", "zero", True, True, True, True
    yield "bgr", "float32", "clamp", False, True, False, False
    yield "planar", "float16", "zero", True, True, False, True
    yield "bgr", "bfloat16", "clamp", False, True, True, False
    yield "planar", "uint8", "clamp", True, True, True, True
    yield "gray", "float32", "zero", False, False, False, True
    yield "bgr", "uint8", "zero", True, False, True, True


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_device_warp_equals_the_reference_in_every_layout(dfx, w, h, n):
    c = _case(w, h, n)
    share = c["inside"].reshape(n, -1).mean(axis=1)
    print(f"{w}x{h} n={n}: inside shares {np.round(share, 3)}")
    if w >= 65:  # neither all inside nor all outside: both branches of the sampling run in every flow
        assert np.all((0.3 <= share) & (share <= 0.9)), share
    full = (w, h) in FULL
    with dfx.FlowEngine(w, h, "farn") as eng:
        for layout in LAYOUTS:
            rigs = {}
            try:
                for combo in _combos(full):
                    kind = combo[0]
                    if kind not in rigs:
                        rigs[kind] = _Rig(eng, c, layout, kind)
                    rigs[kind].check(*combo[1:], tag=(layout,) + combo)
                for rig in rigs.values():  # nothing ever wrote to an input
                    for b in (rig.flow, rig.src, rig.ref, rig.occ):
                        got = b.dev.get(b.dtype)
                        assert np.array_equal(got.view(np.uint8), b.fill.view(np.uint8)), layout
            finally:
                for rig in rigs.values():
                    rig.close()


def test_a_second_identical_call_gives_the_same_statistics(dfx):
    w, h, n = 130, 97, 3
    c = _case(w, h, n)
    with dfx.FlowEngine(w, h, "farn") as eng:
        rig = _Rig(eng, c, "vector", "bgr")
        try:
            rig.call("uint8", "zero", True, True, True, True)
            first = rig.stats.get(np.uint64).copy()
            rig.call("uint8", "zero", True, True, True, True)  # on top of the first call's sums: the library zeroes them
            second = rig.stats.get(np.uint64)
            valid = rig.valid.windows()[0]
        finally:
            rig.close()
    ref = _want(c, "bgr", "zero", "uint8", True)[2]
    assert np.array_equal(first, second) and np.array_equal(second[2:-2].reshape(n, 2), ref)
    assert np.array_equal(ref[:, 0], valid.reshape(n, -1).sum(axis=1).astype(np.uint64)) and ref[:, 0].min() > 0
    assert ref[:, 1].min() > 0


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h, n = 65, 17, 3
    c = _case(w, h, n)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        for kind in KINDS:
            rig = _Rig(eng, c, "dense", kind)
            try:
                sp, sl, si = rig.src.pitch, rig.src.plane, rig.src.image
                fp, fl, fs = rig.flow.pitch, rig.flow.plane, rig.flow.image
                row = rig.rw
                refused = [dict(d_src_ptr=None), dict(d_flow_ptr=None),
                           dict(d_out_ptr=None, d_valid_ptr=None, d_stats_ptr=None), dict(d_ref_ptr=None), dict(n=-1),
                           dict(channels=0), dict(channels=2), dict(channels=4), dict(border=-1), dict(border=2),
                           dict(out_dtype=-1), dict(out_dtype=4),
                           dict(src_pitch=row - 1), dict(row_pitch_floats=w - 1), dict(plane_stride_floats=fp * h - 1),
                           dict(flow_stride_floats=2 * fl - 1), dict(out_pitch=row - 1),
                           dict(occ_pitch=w - 1), dict(occ_stride=w * h - 1), dict(valid_pitch=w - 1), dict(valid_stride=w * h - 1)]
                if kind == "planar":
                    refused += [dict(layout=-1), dict(layout=2), dict(src_plane_stride=sp * h - 1), dict(src_image_stride=3 * sl - 1),
                                dict(out_plane_stride=sp * h - 1), dict(out_image_stride=3 * sl - 1)]
                else:
                    refused += [dict(src_image_stride=sp * h - 1), dict(out_image_stride=sp * h - 1)]
                if kind == "bgr":
                    refused += [dict(layout=-1), dict(layout=2), dict(src_pitch=w), dict(out_pitch=w)]
                for kw in refused:
                    with pytest.raises(dfx.DfxError) as e:
                        rig.call("uint8", "zero", True, True, True, True, **kw)
                    assert e.value.status == 1, (kind, kw)
                assert rig.out["uint8"].untouched() and rig.valid.untouched(), (kind, "a refused call wrote")
                assert np.all(rig.stats.get(np.uint64) == STATS_FILL), (kind, "a refused call wrote")
                rig.call("uint8", "zero", True, True, True, True, n=0)  # DFX_OK, launches nothing
                eng.warp_device(None, 0, 0, 0, 0, 0, None, 0, 0, 0, 0, border=9, out_dtype=9)  # n = 0: nothing else is looked at
                assert rig.out["uint8"].untouched() and rig.valid.untouched(), (kind, "n = 0 wrote")
                if kind == "gray":  # the layout is ignored for one channel, the strides of absent buffers are not looked at
                    rig.call("uint8", "zero", False, False, True, False, layout=7, out_pitch=0, out_image_stride=0,
                             occ_pitch=0, occ_stride=0)
                rig.check("uint8", "zero", True, True, True, True, tag=(kind, "after the refusals"))
            finally:
                rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(eng, c, "dense", "gray")
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call("uint8", "zero", True, True, True, True)
            assert e.value.status == 4
            assert rig.out["uint8"].untouched() and rig.valid.untouched()
        finally:
            rig.close()


@pytest.mark.parametrize("algo", ["tvl1", "brox"])
def test_numpy_wrapper_on_every_flow_handle(dfx, algo):
    w, h, n = 65, 17, 3
    c = _case(w, h, n)
    with dfx.FlowEngine(w, h, algo) as eng:
        for kind in KINDS:
            img = {"gray": c["src"][..., 0], "bgr": c["src"], "planar": c["src"].transpose(0, 3, 1, 2)}[kind]
            ref = {"gray": c["ref"][..., 0], "bgr": c["ref"], "planar": c["ref"].transpose(0, 3, 1, 2)}[kind]
            layout = "chw" if kind == "planar" else "hwc"
            for dtype, name in ((np.uint8, "uint8"), (np.float32, "float32"), (np.float16, "float16"), ("bfloat16", "bfloat16")):
                border = "clamp" if name in ("float32", "bfloat16") else "zero"
                want_out, want_valid, want_stats = _want(c, kind, border, name, True)
                out, valid, stats = eng.warp(img, c["flows"], border=border, dtype=dtype, layout=layout, ref=ref, occ=c["occ"],
                                             want_valid=True, want_stats=True)
                assert out.shape == img.shape and valid.shape == (n, h, w) and stats.shape == (n, 2)
                assert stats.dtype == np.uint64 and valid.dtype == np.uint8
                got = out.view(NP_OF[name]) if name != "bfloat16" else out
                planes = got.reshape(n, 1, h, -1) if kind != "planar" else got
                assert np.array_equal(planes, want_out), (kind, name)
                assert np.array_equal(valid.reshape(n, 1, h, w), want_valid) and np.array_equal(stats, want_stats)
            only = eng.warp(img, c["flows"], layout=layout)  # the defaults: uint8, zero border, nothing else
            assert isinstance(only, np.ndarray) and only.dtype == np.uint8
            assert np.array_equal(only.reshape(n, 1, h, -1) if kind != "planar" else only, _want(c, kind, "zero", "uint8", False)[0])
        empty = eng.warp(np.zeros((0, h, w), np.uint8), np.zeros((0, 2, h, w), F32))
        assert empty.shape == (0, h, w)


def test_warp_tensor_reads_and_writes_tensors_where_they_lie(dfx):
    import torch

    w, h, n = 65, 17, 3
    c = _case(w, h, n)
    dev = torch.device("cuda", 0)
    src, ref = torch.from_numpy(c["src"].copy()).to(dev), torch.from_numpy(c["ref"].copy()).to(dev)  # (n, H, W, 3)
    flows, occ = torch.from_numpy(c["flows"].copy()).to(dev), torch.from_numpy(c["occ"].copy()).to(dev)

    def bits(t):
        if t.dtype == torch.bfloat16 or t.dtype == torch.float16:
            return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        if t.dtype == torch.float32:
            return t.contiguous().cpu().numpy().view(np.uint32)
        return t.contiguous().cpu().numpy()

    with dfx.FlowEngine(w, h, "farn") as eng:
        # a contiguous NCHW tensor: three planes in memory
        nchw, nchw_ref = src.permute(0, 3, 1, 2).contiguous(), ref.permute(0, 3, 1, 2).contiguous()
        out, valid, stats = eng.warp_tensor(nchw, flows, dtype=torch.float16, ref=nchw_ref, occ=occ, want_valid=True, want_stats=True)
        want_out, want_valid, want_stats = _want(c, "planar", "zero", "float16", True)
        assert out.shape == nchw.shape and out.is_contiguous() and out.dtype == torch.float16
        assert np.array_equal(bits(out), want_out)
        assert np.array_equal(valid.cpu().numpy().reshape(n, 1, h, w), want_valid)
        assert stats.dtype == torch.int64 and np.array_equal(stats.cpu().numpy().astype(np.uint64), want_stats)
        # the NCHW view of an NHWC batch: interleaved in memory, read and written without a copy
        view = src.permute(0, 3, 1, 2)
        out = eng.warp_tensor(view, flows, border="clamp", dtype=torch.bfloat16)
        assert out.shape == view.shape and out.stride() == view.stride() and out.dtype == torch.bfloat16
        assert np.array_equal(bits(out.permute(0, 2, 3, 1)).reshape(n, 1, h, 3 * w), _want(c, "bgr", "clamp", "bfloat16", False)[0])
        # slices of larger tensors: gray images in a padded batch, flows and masks likewise, float32 into a padded `out`
        big = torch.full((n + 2, h + 3, w + 5), 0x5A, dtype=torch.uint8, device=dev)
        big[1:n + 1, 2:h + 2, 3:w + 3] = src[..., 0]
        big_flows = torch.full((n, 2, h + 1, w + 7), float("nan"), device=dev)
        big_flows[:, :, :h, 4:w + 4] = flows
        big_out = torch.full((n, h + 2, w + 9), -7.0, device=dev)
        got = eng.warp_tensor(big[1:n + 1, 2:h + 2, 3:w + 3], big_flows[:, :, :h, 4:w + 4], dtype=torch.float32,
                              out=big_out[:, 1:h + 1, 5:w + 5])
        assert got.data_ptr() == big_out[:, 1:h + 1, 5:w + 5].data_ptr()
        assert np.array_equal(bits(got).reshape(n, 1, h, w), _want(c, "gray", "zero", "float32", False)[0])
        frame = torch.ones_like(big_out, dtype=torch.bool)
        frame[:, 1:h + 1, 5:w + 5] = False
        assert bool((big_out[frame] == -7.0).all()), "out was written outside the slice"
        # the default: uint8, an NHWC tensor as it is; `out=` in the images' memory layout
        out8 = torch.zeros_like(src)
        got = eng.warp_tensor(src, flows, out=out8, ref=ref, want_stats=True)
        assert got[0] is out8 and np.array_equal(bits(out8).reshape(n, 1, h, 3 * w), _want(c, "bgr", "zero", "uint8", False)[0])
        assert np.array_equal(got[1].cpu().numpy().astype(np.uint64), _want(c, "bgr", "zero", "uint8", False)[2])


def _pairs(n, step):
    """(a, b) of output flow i: the reference's pair rule."""
    return [((i, i + step) if step > 0 else (i - step, i)) for i in range(max(n - abs(step), 0))]


def test_warp_error_follows_the_pair_rule_and_discriminates(dfx):
    w, h = 97, 61
    clip = SynthClip(w, h, 9)
    frames = np.stack([clip.frame(t) for t in range(6)])
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        for step in (1, 2, -1):
            flows = eng.calc_optflows_planar(list(frames), step)
            got = eng.warp_error(frames, flows, step)
            pairs = _pairs(len(frames), step)
            assert got.dtype == np.float64 and got.shape == (len(pairs),) and flows.shape[0] == len(pairs)
            src, ref = np.stack([frames[b] for _, b in pairs]), np.stack([frames[a] for a, _ in pairs])
            _, valid, stats = R.warp_batch(src, flows, ref=ref)
            want = R.mean_abs_error(stats, 1)
            assert np.array_equal(got, want), (step, got, want)
            if step == 1:  # the zero flow over the same valid set: everything the flow leaves the frame by is masked out
                zero = eng.warp_error(frames, np.zeros_like(flows), step, occ=(1 - valid).astype(np.uint8))
                print(f"step 1: with the flows {np.round(got, 3)}, zero flow {np.round(zero, 3)}, valid share {np.round(valid.mean(axis=(1, 2)), 3)}")
                assert np.all(got <= 0.25 * zero), (got, zero)
        colour = np.stack([frames, frames[::-1], frames], axis=-1)  # (N, H, W, 3): three channels, the middle one reversed
        flows = eng.calc_optflows_planar(list(frames), 1)
        got = eng.warp_error(colour, flows, 1)
        _, _, stats = R.warp_batch(colour[1:], flows, ref=colour[:-1])
        assert np.array_equal(got, R.mean_abs_error(stats, 3))


def test_end_to_end_the_occlusion_mask_does_not_raise_the_error(dfx):
    import torch

    w, h, step = 130, 97, 1
    clip = SynthClip(w, h, 9)
    frames = torch.from_numpy(np.stack([clip.frame(t) for t in (0, 6, 12, 18)])).to(torch.device("cuda", 0))
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        fwd, bwd, occ_fwd, occ_bwd = eng.flow_tensor_bidir(frames, step)
        _, masked = eng.warp_tensor(frames[step:], fwd, occ=occ_fwd, ref=frames[:-step], want_stats=True)
        warped, plain = eng.warp_tensor(frames[step:], fwd, ref=frames[:-step], want_stats=True)
    masked, plain = masked.cpu().numpy().astype(np.uint64), plain.cpu().numpy().astype(np.uint64)
    e_masked, e_plain = R.mean_abs_error(masked, 1), R.mean_abs_error(plain, 1)
    print(f"130x97 tvl1 step {step}: mean absolute error masked {np.round(e_masked, 4)}, unmasked {np.round(e_plain, 4)}, "
          f"pixels {masked[:, 0]} of {plain[:, 0]}")
    assert np.all(masked[:, 0] < plain[:, 0]) and np.all(masked[:, 0] > 0)
    assert np.all(e_masked <= e_plain + 1e-9), (e_masked, e_plain)
    want = R.warp_batch(frames[step:].cpu().numpy(), fwd.cpu().numpy(), ref=frames[:-step].cpu().numpy())
    assert np.array_equal(warped.cpu().numpy(), R.quantise(want[0])) and np.array_equal(plain, want[2])
