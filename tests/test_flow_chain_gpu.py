"""The flow chain on the device (dfx_flow_chain_device, denseflow_amd/csrc/flow_chain_kernels.hip) against its NumPy
restatement (tests/flow_chain_ref.py): the chained flows bit for bit (equal bit patterns wherever the reference is not NaN,
NaN where it is: flow_chain_ref.same_bits) and valid byte for byte, every element outside the windows of an output buffer
still the fill, the inputs untouched.  n = 8 flows; L in {1, 2, 6} x hop in {1, -1, 2} x (anchors, anchor_step) in {(2, 1),
(3, 1), (2, 2), (3, 2)} wherever the link indices fit into the 8 flows (L = 6 with hop 2 would need 11: it does not), a first
link that is not flow 0, both emits, both borders, with and without masks, with and without d_valid; (1, 1), (2, 3), (5, 1),
(1, 7), 97 x 61, 130 x 97, one below / at / above the 256 pixels of a workgroup row and the 4 rows of a workgroup; a layout
that takes the single-element path (row pitch W + 3, bases one element in, odd gaps) and one that takes the 16-byte path;
special values in the first and a middle link, subnormal-scale flows and random bit patterns; the wrappers; every refusal."""
import numpy as np
import pytest

from tests import flow_chain_ref as R
from tests.test_global_motion_gpu import _Planes
from tests.warp_ref import plant_specials

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
N = 8
OUT_FILL, VALID_FILL = 0xA5A5A5A5, 0xA5
MAX_OUT = 18  # 3 anchors x 6 links
SHAPES = [(1, 1), (2, 3), (5, 1), (1, 7), (97, 61), (130, 97), (255, 5), (256, 5), (257, 5), (9, 3), (9, 4), (9, 5)]  # (w, h)


def _chains(n=N, lengths=(1, 2, 6), hops=(1, -1, 2), anchors=((2, 1), (3, 1), (2, 2), (3, 2))):
    """(L, first, hop, anchors, anchor_step) of every combination whose link indices fit into n flows; the first link is one
    flow further in than it has to be wherever that still fits."""
    for L in lengths:
        for hop in hops:
            for m, step in anchors:
                k1 = (L - 1) * hop
                first = max(0, -k1)
                if first + (m - 1) * step + max(k1, 0) >= n:
                    continue
                if first + 1 + (m - 1) * step + max(k1, 0) < n:
                    first += 1
                yield L, first, hop, m, step


def test_the_chains_of_the_grid():
    got = list(_chains())
    assert len(got) == 30 and not [c for c in got if c[0] == 6 and c[2] == 2]
    assert {c[0] for c in got} == {1, 2, 6} and {c[2] for c in got} == {1, -1, 2} and {c[3:] for c in got} == {(2, 1), (3, 1), (2, 2), (3, 2)}
    assert any(c[1] > 0 and c[2] == 1 for c in got)
    for L, first, hop, m, step in got:
        idx = [first + j * step + k * hop for j in range(m) for k in range(L)]
        assert 0 <= min(idx) and max(idx) < N and m * L <= MAX_OUT


class _Rig:
    """The device buffers of one batch of flows (N, 2, H, W), masks (N, H, W) and MAX_OUT outputs in one layout."""

    def __init__(self, eng, flows, occ, layout="vector"):
        self.eng, self.flows, self.occ_host = eng, flows, occ
        n, _, h, w = flows.shape
        self.n, self.h, self.w = n, h, w
        if layout == "scalar":  # bases one element in, a pitch of W + 3, odd gaps: single elements everywhere
            pf = w + 3
            gf = dict(lead=1, pitch=pf, plane=h * pf + 1, item=2 * (h * pf + 1) + 5)
            go = dict(lead=3, pitch=pf, plane=h * pf + 2, item=2 * (h * pf + 2) + 1)
            gm = dict(lead=1, pitch=w + 3, item=h * (w + 3) + 2)
            gv = dict(lead=1, pitch=w + 1, item=h * (w + 1) + 3)
        else:  # "vector": every base and stride a multiple of 16 bytes, rows padded, gaps between planes and flows
            pw = (w + 3) // 4 * 4 + 4
            gf = go = dict(pitch=pw, plane=h * pw + 8, item=2 * (h * pw + 8) + 12)
            gm = gv = dict(pitch=pw, item=h * pw + 8)
        self.flow = _Planes(eng, n, 2, h, w, F32, np.nan, flows, **gf)
        self.occ = _Planes(eng, n, 1, h, w, np.uint8, 1, occ.reshape(n, 1, h, w), **gm)
        self.out = _Planes(eng, MAX_OUT, 2, h, w, U32, OUT_FILL, **go)
        self.valid = _Planes(eng, MAX_OUT, 1, h, w, np.uint8, VALID_FILL, **gv)
        self.bufs = [self.flow, self.occ, self.out, self.valid]
        if layout == "scalar":
            assert self.flow.ptr() % 16 == 4 and self.flow.pitch == w + 3 and self.valid.ptr() % 4 == 1
        else:
            assert all(b.ptr() % 16 == 0 for b in self.bufs)

    def call(self, length=2, first=0, hop=1, anchors=2, anchor_step=1, emit=0, border=0, with_occ=True, want_valid=True, **over):
        kw = dict(d_flow_ptr=self.flow.ptr(), row_pitch_floats=self.flow.pitch, plane_stride_floats=self.flow.plane,
                  flow_stride_floats=self.flow.item, n=self.n, d_out_ptr=self.out.ptr(), out_row_pitch_floats=self.out.pitch,
                  out_plane_stride_floats=self.out.plane, out_flow_stride_floats=self.out.item, length=length, first=first,
                  hop=hop, anchors=anchors, anchor_step=anchor_step, emit=emit, border=border,
                  d_occ_ptr=self.occ.ptr() if with_occ else None, occ_pitch=self.occ.pitch, occ_stride=self.occ.item,
                  d_valid_ptr=self.valid.ptr() if want_valid else None, valid_pitch=self.valid.pitch,
                  valid_stride=self.valid.item)
        kw.update(over)
        self.eng.flow_chain_device(**kw)

    def check(self, tag, want, want_valid, chain, emit, border, with_occ, ask_valid=True):
        """One call against (want, want_valid) of flow_chain_ref.chain_batch."""
        L, first, hop, m, step = chain
        self.reset()
        self.call(L, first, hop, m, step, R.EMITS[emit], R.BORDERS.index(border), with_occ, ask_valid)
        e = m * (L if emit == "all" else 1)
        assert want.shape[0] == e
        got, clean = self.out.windows()
        nan = np.isnan(want)
        bad = np.where(nan, ~np.isnan(got[:e].view(F32)), got[:e] != want.view(U32))
        assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4], got[:e][bad][:4], want.view(U32)[bad][:4])
        assert R.same_bits(got[:e].view(F32), want), tag
        assert clean and (got[e:] == OUT_FILL).all(), (tag, "an element outside the windows of the outputs asked for was written")
        if ask_valid:
            got, clean = self.valid.windows()
            assert np.array_equal(got[:e, 0], want_valid), (tag, "valid", np.argwhere(got[:e, 0] != want_valid)[:4])
            assert clean and (got[e:] == VALID_FILL).all(), (tag, "a byte outside the valid planes asked for was written")
        else:
            assert self.valid.untouched(), (tag, "valid was written without being asked for")

    def reset(self):
        e = self.eng
        for b in (self.out, self.valid):
            e._check(e._L.dfx_memcpy_h2d(e._h, b.dev.ptr(), b.fill.ctypes.data, b.fill.nbytes))

    def close(self):
        for b in self.bufs:
            b.close()


def _reference(flows, occ, chains):
    """{(chain, border, with masks): chain_batch(..., emit "all")}: computed once, shared by the layouts and both emits."""
    want = {}
    for chain in chains:
        L, first, hop, m, step = chain
        for border in R.BORDERS:
            for with_occ in (False, True):
                want[chain, border, with_occ] = R.chain_batch(flows, L, first, hop, m, step, "all", border, occ if with_occ else None)
    return want


def _grid(eng, flows, occ, chains, layouts=("scalar", "vector"), tag=(), want=None):
    """chains x emit x border x masks on these flows in these layouts; every third call goes without d_valid."""
    want = _reference(flows, occ, chains) if want is None else want
    calls = 0
    for layout in layouts:
        rig = _Rig(eng, flows, occ, layout)
        try:
            for (chain, border, with_occ), (every, vevery) in want.items():
                L = chain[0]
                for emit in ("last", "all"):
                    w, v = (every, vevery) if emit == "all" else (every[L - 1::L], vevery[L - 1::L])
                    calls += 1
                    rig.check(tag + (flows.shape[3], flows.shape[2], layout, chain, emit, border, with_occ), w, v, chain, emit,
                              border, with_occ, ask_valid=calls % 3 != 0)
            assert rig.flow.untouched() and rig.occ.untouched(), (tag, layout, "the inputs were written")
        finally:
            rig.close()
    return want


@pytest.fixture(scope="module")
def eng(dfx):
    with dfx.FlowEngine(130, 97, "farn") as e:
        yield e


_WANT = {}  # (w, h): the reference of the whole grid at that shape, shared by the two layouts


@pytest.mark.parametrize("layout", ["scalar", "vector"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_the_whole_grid_at_every_shape_on_a_farneback_handle_resized(eng, w, h, layout):
    eng.set_size(w, h)
    flows, occ = R.chain_inputs(w, h)
    if (w, h) not in _WANT:
        _WANT[w, h] = _reference(flows, occ, list(_chains()))
    want = _grid(eng, flows, occ, list(_chains()), (layout,), want=_WANT[w, h])
    if (w, h) in ((97, 61), (130, 97)):  # on the reference alone: both values of valid are really exercised
        for with_occ in (False, True):
            share = want[(6, 1, 1, 2, 1), "zero", with_occ][1][5].mean()
            assert 0.2 <= share <= 0.95, (w, h, with_occ, share)


def test_a_tvl1_handle_allocates_nothing_and_its_stats_stay(dfx):
    w, h = 97, 61
    flows, occ = R.chain_inputs(w, h)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        before, stats = eng.device_bytes(), bytes(eng.stats())
        rig = _Rig(eng, flows, occ, "vector")
        try:
            held = eng.device_bytes()
            for chain in ((6, 0, 1, 3, 1), (6, 6, -1, 2, 1)):
                for emit in ("last", "all"):
                    want, wv = R.chain_batch(flows, *chain, emit, "clamp", occ)
                    rig.check(("tvl1", chain, emit), want, wv, chain, emit, "clamp", True)
            assert eng.device_bytes() == held, "the call allocated"
        finally:
            rig.close()
        assert eng.device_bytes() == before and bytes(eng.stats()) == stats, "dfx_get_stats or dfx_device_bytes changed"


def _random_bits(rng, shape):
    """Random bit patterns as float32: every class of value occurs (about 1 in 128 a NaN or an infinity, 1 in 256 subnormal)."""
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32).view(F32)


SPECIAL_CHAINS = list(_chains(lengths=(1, 2, 6), hops=(1,), anchors=((3, 1),))) + [(6, 6, -1, 2, 1), (2, 1, 2, 3, 2)]


@pytest.mark.parametrize("w,h", [(97, 61), (13, 9), (5, 1)])
def test_special_values_in_the_first_and_a_middle_link(eng, w, h):
    """NaN in u or v, +-inf, +-1e30, -0.0, a landing exactly on the last column or row and one ulp beyond (warp_ref's
    specials), in the flow a chain starts with and in one it reaches after accumulating."""
    eng.set_size(w, h)
    flows, occ = R.chain_inputs(w, h)
    for i in (0, 1, 3, 6):  # first links of the chains above, and middle links of the six-link ones
        where = plant_specials(flows[i])
    assert len(where) == 13
    want = _grid(eng, flows, occ, SPECIAL_CHAINS, tag=("specials",))
    if (w, h) == (97, 61):
        assert np.isnan(flows[0]).sum() == 2 and np.isinf(flows[3]).sum() == 2
        out = want[(6, 0, 1, 3, 1), "clamp", False][0]
        assert np.isnan(out).any() and (np.abs(out[np.isfinite(out)]) > 1e29).any()


def test_subnormal_scale_flows_and_random_bit_patterns(eng):
    w, h = 67, 7
    eng.set_size(w, h)
    rng = np.random.default_rng(480)
    flows, occ = R.chain_inputs(w, h)
    tiny = (flows.astype(np.float64) * 1e-39).astype(F32)
    assert (tiny != 0).mean() > 0.9 and (np.abs(tiny) < 1.2e-38).all()
    want = _grid(eng, tiny, occ, SPECIAL_CHAINS, tag=("subnormal",))
    out = want[(6, 0, 1, 3, 1), "zero", False][0]
    assert (out != 0).mean() > 0.9 and (np.abs(out) < 1.2e-38).all(), "the sums of subnormals are subnormals, not zero"
    bits = _random_bits(rng, (N, 2, h, w))
    assert np.isnan(bits).sum() > 20 and (np.abs(bits[np.isfinite(bits)]) < 1.2e-38).sum() > 10
    _grid(eng, bits, occ, SPECIAL_CHAINS, tag=("bits",))


def test_the_three_wrappers_agree(dfx):
    import torch

    w, h = 97, 61
    flows, occ = R.chain_inputs(w, h)
    dev = torch.device("cuda", 0)
    big = torch.full((N + 1, 2, h + 2, w + 7), float("nan"), device=dev)
    big[1:, :, 1:h + 1, 3:w + 3] = torch.from_numpy(flows).to(dev)
    view = big[1:, :, 1:h + 1, 3:w + 3]
    big_occ = torch.ones((N, h + 1, w + 3), dtype=torch.uint8, device=dev)
    big_occ[:, :h, 2:w + 2] = torch.from_numpy(occ).to(dev)
    occ_view = big_occ[:, :h, 2:w + 2]
    with dfx.FlowEngine(w, h, "farn") as eng:
        before = eng.device_bytes()
        for kw in (dict(length=6), dict(length=2, first=1, hop=2, anchors=2, anchor_step=2, emit="all", border="clamp"),
                   dict(length=3, first=7, hop=-1, anchors=None, emit="all"), dict(length=1, emit="all")):
            for o, ot in ((None, None), (occ, occ_view)):
                want, wv = R.chain_batch(flows, occ=o, **kw)
                out, valid = eng.flow_chain(flows, occ=o, **kw)
                assert R.same_bits(out, want) and np.array_equal(valid, wv), kw
                tout, tvalid = eng.flow_chain_tensor(view, occ=ot, **kw)
                assert tout.is_contiguous() and tout.shape == want.shape and tvalid.dtype == torch.uint8
                assert R.same_bits(tout.cpu().numpy(), want) and np.array_equal(tvalid.cpu().numpy(), wv), kw
        assert want.shape[0] == N  # the last setting: every flow a chain of its own
        # the raw-pointer form is what the grids above hold against the same reference; here: into a slice of a larger tensor
        into = torch.full((3, 2, h + 1, w + 5), -7.0, device=dev)
        want, wv = R.chain_batch(flows, 6, occ=occ)
        same, valid = eng.flow_chain_tensor(view, 6, occ=occ_view, out=into[:, :, 1:, 2:w + 2])
        assert same.data_ptr() == into[:, :, 1:, 2:w + 2].data_ptr()
        assert R.same_bits(same.contiguous().cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv)
        frame = torch.ones_like(into, dtype=torch.bool)
        frame[:, :, 1:, 2:w + 2] = False
        assert bool((into[frame] == -7.0).all()), "written outside the slice"
        inside = torch.zeros_like(big, dtype=torch.bool)
        inside[1:, :, 1:h + 1, 3:w + 3] = True
        assert bool(torch.isnan(big[~inside]).all()) and np.array_equal(view.cpu().numpy().view(U32), flows.view(U32))
        none, nov = eng.flow_chain_tensor(view, 9)  # no chain of nine links fits into eight flows
        assert none.shape == (0, 2, h, w) and nov.shape == (0, h, w)
        assert eng.device_bytes() == before and eng.stats().pairs == 0


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h = 97, 61
    flows, occ = R.chain_inputs(w, h)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        rig = _Rig(eng, flows, occ, "vector")
        big = 1 << 20
        try:
            before, stats = eng.device_bytes(), bytes(eng.stats())
            refused = [dict(d_flow_ptr=None), dict(d_out_ptr=None), dict(n=-1), dict(hop=0), dict(length=0), dict(length=-2),
                       dict(anchors=-1), dict(anchor_step=0), dict(anchor_step=-1),
                       dict(first=-1), dict(first=N), dict(first=7), dict(length=9), dict(anchors=8), dict(n=2, anchors=2),
                       dict(hop=-1), dict(first=1, hop=-1, length=3), dict(hop=4, length=3), dict(anchors=3, anchor_step=4),
                       dict(first=2 ** 31 - 1), dict(hop=2 ** 31 - 1, length=2 ** 31 - 1), dict(anchor_step=2 ** 31 - 1),
                       dict(hop=-2 ** 31, length=3, first=7),
                       dict(emit=-1), dict(emit=2), dict(border=-1), dict(border=2),
                       dict(d_out_ptr=rig.flow.ptr()),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=h * rig.flow.pitch - 1),
                       dict(flow_stride_floats=2 * rig.flow.plane - 1),
                       dict(out_row_pitch_floats=w - 1), dict(out_plane_stride_floats=h * rig.out.pitch - 1),
                       dict(out_flow_stride_floats=2 * rig.out.plane - 1),
                       dict(occ_pitch=w - 1), dict(occ_stride=h * rig.occ.pitch - 1),
                       dict(valid_pitch=w - 1), dict(valid_stride=h * rig.valid.pitch - 1),
                       dict(row_pitch_floats=big, plane_stride_floats=big)]  # a plane shorter than its rows
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    rig.call(**kw)
                assert e.value.status == 1, kw
            with pytest.raises(dfx.DfxError) as e:  # a NULL descriptor
                eng._check(eng._L.dfx_flow_chain_device(eng._h, None))
            assert e.value.status == 1
            assert rig.out.untouched() and rig.valid.untouched(), "a refused call wrote"
            rig.call(n=0)          # DFX_OK, launches nothing
            rig.call(anchors=0)    # likewise
            eng.flow_chain_device(None, 0, 0, 0, 0, None, 0, 0, 0, length=-3, hop=0, anchors=5, emit=9, border=7)  # n = 0
            eng.flow_chain_device(None, 0, 0, 0, 4, None, 0, 0, 0, length=-3, hop=0, anchors=0, emit=9, border=7)  # anchors = 0
            assert rig.out.untouched() and rig.valid.untouched(), "n = 0 or anchors = 0 wrote"
            # the strides of absent buffers are not looked at
            rig.call(with_occ=False, want_valid=False, occ_pitch=0, occ_stride=0, valid_pitch=0, valid_stride=0)
            chain = (6, 1, 1, 2, 1)
            want, wv = R.chain_batch(flows, *chain, "all", "zero", occ)
            rig.check("after the refusals", want, wv, chain, "all", "zero", True)
            assert eng.device_bytes() == before and bytes(eng.stats()) == stats
        finally:
            rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(eng, flows, occ, "vector")
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call()
            assert e.value.status == 4
            assert rig.out.untouched() and rig.valid.untouched()
        finally:
            rig.close()
