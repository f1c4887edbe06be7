"""The forward projection on the device (dfx_flow_project_device, denseflow_amd/csrc/flow_project_kernels.hip) against its
NumPy restatement (tests/flow_project_ref.py): out, hole and coverage bit for bit in every case, every element outside the
windows of an output buffer still the fill, the inputs untouched.  Shapes around the 32 x 8 source tile of a workgroup, the
48 x 16 LDS window and the 256 x 4 pixels of a normalising workgroup, in a layout that takes the 16-byte accesses and one
that takes single elements (and a workspace 8 mod 16); the grid of settings at 97 x 61; landings on integers and on the edges
of the landing test, special flow values and random bit patterns; special importances; all pixels onto one target, onto one
row, and smooth flows of a quarter of the frame (every tap outside the window); workspaces for one, two and all flows and
garbage in them; the wrappers; every refusal; the hole plane fed to the median fill and to the chain."""
import numpy as np
import pytest

from tests import flow_project_ref as R
from tests.devmem import DevBuf
from tests.test_global_motion_gpu import _Planes

pytestmark = pytest.mark.gpu

F32, U32, U8 = np.float32, np.uint32, np.uint8
OUT_FILL, BYTE_FILL = 0xA5A5A5A5, 0xA5
SHAPES = [(1, 1), (3, 2), (5, 1), (13, 9), (63, 5), (64, 16), (65, 17), (97, 61), (130, 97), (257, 33)]  # (w, h)
OUTPUTS = [("out", "hole", "cov"), ("out",), ("hole",), ("cov",)]


class _Rig:
    """The device buffers of one batch of flows (n, 2, H, W), importances and masks (n, H, W) and the outputs in one layout."""

    def __init__(self, eng, flows, imp, occ, layout="vector", work_flows=None):
        self.eng = eng
        n, _, h, w = flows.shape
        self.n, self.h, self.w = n, h, w
        if layout == "scalar":  # bases one element in, a pitch of W + 3, odd gaps: single elements everywhere
            pf = w + 3
            gf = dict(lead=1, pitch=pf, plane=h * pf + 1, item=2 * (h * pf + 1) + 5)
            go = dict(lead=3, pitch=pf, plane=h * pf + 2, item=2 * (h * pf + 2) + 1)
            gi = dict(lead=1, pitch=w + 1, item=h * (w + 1) + 3)
            gm = dict(lead=1, pitch=w + 3, item=h * (w + 3) + 2)
            gh = dict(lead=1, pitch=w + 1, item=h * (w + 1) + 3)
            gc = dict(lead=1, pitch=w + 2, item=h * (w + 2) + 1)
        else:  # "vector": every base and stride a multiple of 16 bytes, rows padded, gaps between planes and flows
            pw = (w + 3) // 4 * 4 + 4
            gf = go = dict(pitch=pw, plane=h * pw + 8, item=2 * (h * pw + 8) + 12)
            gi = gm = gh = gc = dict(pitch=pw, item=h * pw + 8)
        self.flow = _Planes(eng, n, 2, h, w, F32, np.nan, flows, **gf)
        self.imp = _Planes(eng, n, 1, h, w, F32, np.nan, imp.reshape(n, 1, h, w), **gi)
        self.occ = _Planes(eng, n, 1, h, w, U8, 1, occ.reshape(n, 1, h, w), **gm)
        self.out = _Planes(eng, n, 2, h, w, U32, OUT_FILL, **go)
        self.hole = _Planes(eng, n, 1, h, w, U8, BYTE_FILL, **gh)
        self.cov = _Planes(eng, n, 1, h, w, U32, OUT_FILL, **gc)
        self.per = eng.flow_project_work_bytes()
        assert self.per == 24 * w * h
        self.work_bytes = self.per * (n if work_flows is None else work_flows)
        self.work_lead = 8 if layout == "scalar" else 0
        rng = np.random.default_rng(7)
        self.garbage = rng.integers(0, 256, self.work_bytes + 32, dtype=np.uint64).astype(U8)
        self.work = DevBuf(eng, init=self.garbage)
        self.bufs = [self.flow, self.imp, self.occ, self.out, self.hole, self.cov, self.work]
        if layout == "scalar":
            assert self.flow.ptr() % 16 == 4 and self.hole.ptr() % 4 == 1 and self.work.ptr(self.work_lead) % 16 == 8
        else:
            assert all(b.ptr() % 16 == 0 for b in self.bufs)

    def call(self, t=1.0, scale=-1.0, min_weight=0.25, with_imp=False, with_occ=False, outputs=("out", "hole", "cov"), **over):
        kw = dict(d_flow_ptr=self.flow.ptr(), row_pitch_floats=self.flow.pitch, plane_stride_floats=self.flow.plane,
                  flow_stride_floats=self.flow.item, n=self.n, d_work_ptr=self.work.ptr(self.work_lead),
                  work_bytes=self.work_bytes, t=t, scale=scale, min_weight=min_weight,
                  d_out_ptr=self.out.ptr() if "out" in outputs else None, out_row_pitch_floats=self.out.pitch,
                  out_plane_stride_floats=self.out.plane, out_flow_stride_floats=self.out.item,
                  d_hole_ptr=self.hole.ptr() if "hole" in outputs else None, hole_pitch=self.hole.pitch,
                  hole_stride=self.hole.item, d_coverage_ptr=self.cov.ptr() if "cov" in outputs else None,
                  coverage_pitch_floats=self.cov.pitch, coverage_stride_floats=self.cov.item,
                  d_importance_ptr=self.imp.ptr() if with_imp else None, importance_pitch_floats=self.imp.pitch,
                  importance_stride_floats=self.imp.item, d_occ_ptr=self.occ.ptr() if with_occ else None,
                  occ_pitch=self.occ.pitch, occ_stride=self.occ.item)
        kw.update(over)
        self.eng.flow_project_device(**kw)

    def outputs_untouched(self):
        return self.out.untouched() and self.hole.untouched() and self.cov.untouched()

    def check(self, tag, want, outputs=("out", "hole", "cov"), **kw):
        """One call against want = (out, hole, coverage) of flow_project_ref."""
        self.reset()
        self.call(outputs=outputs, **kw)
        for name, buf, ref in (("out", self.out, want[0].view(U32)), ("hole", self.hole, want[1][:, None]),
                               ("cov", self.cov, want[2].view(U32)[:, None])):
            if name in outputs:
                got, clean = buf.windows()
                bad = got != ref
                assert not bad.any(), (tag, name, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])
                assert clean, (tag, name, "an element outside the windows was written")
            else:
                assert buf.untouched(), (tag, name, "written without being asked for")

    def reset(self):
        e = self.eng
        for b in (self.out, self.hole, self.cov):
            e._check(e._L.dfx_memcpy_h2d(e._h, b.dev.ptr(), b.fill.ctypes.data, b.fill.nbytes))

    def inputs_untouched(self):
        return self.flow.untouched() and self.imp.untouched() and self.occ.untouched()

    def close(self):
        for b in self.bufs:
            b.close()


class _Ref:
    """The reference of one batch, the sums shared by the calls that differ only in scale and min_weight."""

    def __init__(self, flows, imp, occ):
        self.flows, self.imp, self.occ, self.sums = flows, imp, occ, {}

    def __call__(self, t=1.0, scale=-1.0, min_weight=0.25, with_imp=False, with_occ=False):
        key = (t, with_imp, with_occ)
        if key not in self.sums:
            self.sums[key] = [R.sums(f, t, self.imp[i] if with_imp else None, self.occ[i] if with_occ else None)
                              for i, f in enumerate(self.flows)]
        res = [R.normalise(*s, scale, min_weight) for s in self.sums[key]]
        return tuple(np.stack([r[k] for r in res]) for k in range(3))


@pytest.fixture(scope="module")
def eng(dfx):
    with dfx.FlowEngine(130, 97, "farn") as e:
        yield e


def _both_layouts(eng, flows, imp, occ, cases, tag=()):
    ref = _Ref(flows, imp, occ)
    for layout in ("scalar", "vector"):
        rig = _Rig(eng, flows, imp, occ, layout)
        try:
            for k, kw in enumerate(cases):
                rig.check(tag + (layout, kw), ref(**kw), **kw)
            assert rig.inputs_untouched(), (tag, layout, "the inputs were written")
        finally:
            rig.close()
    return ref


FEW = [dict(), dict(t=0.5, scale=0.5, with_imp=True, with_occ=True), dict(t=-1.0, scale=1.0, min_weight=0.0, with_occ=True),
       dict(t=0.25, scale=-0.25, min_weight=1.0, with_imp=True)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_every_shape_on_a_farneback_handle_resized(eng, w, h):
    eng.set_size(w, h)
    flows, imp, occ = R.project_inputs(w, h)
    ref = _both_layouts(eng, flows, imp, occ, FEW, (w, h))
    if w * h >= 97 * 61:  # on the reference alone: holes, collisions and plain pixels all occur
        _, hole, cov = ref()
        assert 0.01 < hole.mean() < 0.6 and cov.max() > 1.5


def test_the_grid_of_settings(eng):
    w, h = 97, 61
    eng.set_size(w, h)
    flows, imp, occ = R.project_inputs(w, h)
    cases = [dict(t=t, scale=s, min_weight=mw, with_imp=i, with_occ=o)
             for t in (1.0, 0.5, -1.0, 0.25) for s in (-t, 1.0 - t, 1.0) for mw in (0.0, 0.25, 1.0)
             for i in (False, True) for o in (False, True)]
    assert len(cases) == 144
    ref = _Ref(flows, imp, occ)
    for layout, some in (("vector", cases), ("scalar", cases[5::9])):  # each output alone and all together, in both layouts
        rig = _Rig(eng, flows, imp, occ, layout)
        try:
            for k, kw in enumerate(some):
                rig.check((layout, kw), ref(**kw), OUTPUTS[(k + k // 4) % 4], **kw)
            assert rig.inputs_untouched()
        finally:
            rig.close()


def _random_bits(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32).view(F32)


def _plant(flows):
    """Landings and values at the edges of the arithmetic, planted into flows (n, 2, h, w) in place: per flow i, row-major
    pixel 5 k + i + 1 (modulo w * h) takes special value k in plane i % 2; the landings (exactly -1, one ulp inside it, exactly
    W or H, one ulp inside it, 0, the last column or row, a half) start from column 0 or row 0."""
    n, _, h, w = flows.shape
    one = np.nextafter
    for i in range(n):
        c = i % 2  # the plane that takes the value; the other keeps a landing inside the frame
        vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 1e-40, -1e-40, 1.1754944e-38]
        for k, v in enumerate(vals):
            flows[i, c].reshape(-1)[(5 * k + i + 1) % (w * h)] = F32(v)
        for k, land in enumerate((-1.0, one(F32(-1), F32(0)), float(w if c == 0 else h), one(F32(w if c == 0 else h), F32(0)), 0.0,
                                  float((w if c == 0 else h) - 1), 0.5)):
            # from column 0 (c = 0) or row 0 (c = 1), so that 0 + flow is the landing to the last bit at t = 1
            y, x = ((k + i) % h, 0) if c == 0 else (0, (k + i) % w)
            flows[i, c, y, x] = F32(land)
            flows[i, 1 - c, y, x] = 0.0
    return flows


@pytest.mark.parametrize("w,h", [(97, 61), (13, 9), (5, 1)])
def test_landings_and_special_flow_values(eng, w, h):
    eng.set_size(w, h)
    rng = np.random.default_rng(491)
    flows, imp, occ = R.project_inputs(w, h)
    cases = [dict(), dict(min_weight=0.0, with_imp=True), dict(t=-1.0, scale=1.0, with_occ=True), dict(t=0.25, scale=0.75, min_weight=0.0)]
    whole = np.round(flows)  # every landing exactly on an integer: one tap per source
    ref = _both_layouts(eng, whole, imp, occ, cases, ("integers",))
    assert set(np.unique(ref(min_weight=0.0)[2])) <= set(np.arange(0, 64, dtype=F32))
    _both_layouts(eng, _plant(flows.copy()), imp, occ, cases, ("specials",))
    _both_layouts(eng, (flows.astype(np.float64) * 1e-39).astype(F32), imp, occ, cases, ("subnormal",))
    bits = _random_bits(rng, flows.shape)
    _both_layouts(eng, bits, imp, occ, cases, ("bits",))
    mixed = np.where(rng.random(flows.shape) < 0.3, bits, flows)  # bit patterns among landings inside the frame
    _both_layouts(eng, mixed, _random_bits(rng, imp.shape), occ, cases, ("mixed bits",))


def test_special_importances(eng):
    w, h = 97, 61
    eng.set_size(w, h)
    flows, imp, occ = R.project_inputs(w, h)
    vals = np.array([np.nan, 0.0, -0.0, -1.0, 1e-3, 1.0 / 512, 1.0 / 513, 256.0, 257.0, 1e9, np.inf, -np.inf, 1e-40], F32)
    imp = vals[np.random.default_rng(3).integers(0, len(vals), imp.shape)]
    cases = [dict(with_imp=True, min_weight=mw) for mw in (0.0, 0.25)] + [dict(t=0.5, scale=0.5, with_imp=True, with_occ=True, min_weight=0.0)]
    ref = _both_layouts(eng, flows, imp, occ, cases)
    cov = ref(with_imp=True, min_weight=0.0)[2]
    assert cov.max() > 256.0 and (cov == 0).any()


def test_contention_and_taps_outside_the_window(eng):
    """All pixels onto one target and onto one row (every add of a flow on the same few words), and smooth random flows of a
    quarter of the frame (almost no tap within 24 pixels of where its tile's centre lands)."""
    w, h = 97, 61
    eng.set_size(w, h)
    _, imp, occ = R.project_inputs(w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    point = np.stack([40 - xx, 25 - yy]).astype(F32)
    row = np.stack([np.zeros_like(xx), 30.5 - yy]).astype(F32)
    far = R.smooth_random_flow(np.random.default_rng(5), 1, h, w, 0.25 * w, cells=12)[0]
    flows = np.stack([point, row, far])
    cases = [dict(min_weight=0.0), dict(min_weight=0.0, with_imp=True, with_occ=True), dict(t=0.5, scale=-0.5), dict(min_weight=1.0)]
    ref = _both_layouts(eng, flows, imp, occ, cases)
    out, hole, cov = ref(min_weight=0.0)
    assert cov[0, 25, 40] == w * h and (hole[0] == 0).sum() == 1 and (hole[1] == 0).sum() == 2 * w and cov[1, 30, 0] == h / 2
    assert np.abs(far).max() > 0.25 * w and 0.05 < (hole[2] == 0).mean() < 0.95


def test_the_workspace_may_hold_one_flow_or_all_and_anything(eng):
    w, h = 65, 17
    eng.set_size(w, h)
    flows, imp, occ = R.project_inputs(w, h, n=5)
    ref = _Ref(flows, imp, occ)
    kw = dict(t=0.5, scale=0.5, with_imp=True, with_occ=True)
    for layout in ("scalar", "vector"):
        for work_flows in (1, 2, 5):
            rig = _Rig(eng, flows, imp, occ, layout, work_flows)
            try:
                assert rig.work_bytes == work_flows * 24 * w * h
                for again in range(2):  # the second call finds the sums of the first in the workspace
                    rig.check((layout, work_flows, again), ref(**kw), **kw)
                rig.check((layout, work_flows, "one byte short of one more flow"), ref(), work_bytes=rig.work_bytes + rig.per - 1)
                end = rig.work_lead + rig.work_bytes
                assert np.array_equal(rig.work.get()[end:], rig.garbage[end:]), "written behind the workspace"
                assert np.array_equal(rig.work.get()[:rig.work_lead], rig.garbage[:rig.work_lead]), "written before the workspace"
            finally:
                rig.close()


def test_a_tvl1_handle_allocates_nothing_and_its_stats_stay(dfx):
    w, h = 97, 61
    flows, imp, occ = R.project_inputs(w, h)
    ref = _Ref(flows, imp, occ)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        before, stats = eng.device_bytes(), bytes(eng.stats())
        rig = _Rig(eng, flows, imp, occ, "vector")
        try:
            held = eng.device_bytes()
            for kw in FEW:
                rig.check(("tvl1", kw), ref(**kw), **kw)
            assert eng.device_bytes() == held, "the call allocated"
        finally:
            rig.close()
        assert eng.device_bytes() == before and bytes(eng.stats()) == stats, "dfx_get_stats or dfx_device_bytes changed"


def test_the_wrappers_agree(dfx):
    import torch

    w, h, n = 97, 61, 3
    flows, imp, occ = R.project_inputs(w, h)
    dev = torch.device("cuda", 0)
    big = torch.full((n + 1, 2, h + 2, w + 7), float("nan"), device=dev)
    big[1:, :, 1:h + 1, 3:w + 3] = torch.from_numpy(flows).to(dev)
    view = big[1:, :, 1:h + 1, 3:w + 3]
    big_imp = torch.full((n, h + 1, w + 5), float("nan"), device=dev)
    big_imp[:, 1:, 4:w + 4] = torch.from_numpy(imp).to(dev)
    imp_view = big_imp[:, 1:, 4:w + 4]
    big_occ = torch.ones((n, h + 1, w + 3), dtype=torch.uint8, device=dev)
    big_occ[:, :h, 2:w + 2] = torch.from_numpy(occ).to(dev)
    occ_view = big_occ[:, :h, 2:w + 2]
    with dfx.FlowEngine(w, h, "farn") as eng:
        before = eng.device_bytes()
        for kw in (dict(), dict(t=0.5), dict(t=0.5, scale=0.5, min_weight=0.0), dict(t=-1.0, scale=1.0, min_weight=1.0)):
            for (i, it), (o, ot) in (((None, None), (None, None)), ((imp, imp_view), (occ, occ_view)), ((imp, imp_view), (None, None))):
                want = R.project(flows, importance=i, occ=o, **kw)
                got = eng.flow_project(flows, importance=i, occ=o, coverage=True, **kw)
                assert all(R.same_bits(a, b) for a, b in zip(got, want)), kw
                two = eng.flow_project(flows, importance=i, occ=o, **kw)
                assert len(two) == 2 and R.same_bits(two[0], want[0]) and R.same_bits(two[1], want[1])
                tgot = eng.flow_project_tensor(view, importance=it, occ=ot, coverage=True, **kw)
                assert tgot[0].is_contiguous() and tgot[1].dtype == torch.uint8 and tgot[2].dtype == torch.float32
                assert all(R.same_bits(a.cpu().numpy(), b) for a, b in zip(tgot, want)), kw
        want = R.project(flows, t=1.0, scale=-1.0, occ=occ)
        got = eng.flow_invert(flows, occ=occ, coverage=True)
        assert all(R.same_bits(a, b) for a, b in zip(got, want))
        # into a slice of a larger tensor, with a workspace of the caller's that holds two flows and is 8 mod 16
        into = torch.full((n, 2, h + 1, w + 5), -7.0, device=dev)
        store = torch.full((2 * 3 * w * h + 1,), -1, dtype=torch.int64, device=dev)
        work = store[1:] if store.data_ptr() % 16 == 0 else store[:-1]
        same, hole = eng.flow_project_tensor(view, t=1.0, scale=-1.0, occ=occ_view, out=into[:, :, 1:, 2:w + 2], work=work)
        assert same.data_ptr() == into[:, :, 1:, 2:w + 2].data_ptr()
        assert R.same_bits(same.contiguous().cpu().numpy(), want[0]) and R.same_bits(hole.cpu().numpy(), want[1])
        frame = torch.ones_like(into, dtype=torch.bool)
        frame[:, :, 1:, 2:w + 2] = False
        assert bool((into[frame] == -7.0).all()), "written outside the slice"
        inside = torch.zeros_like(big, dtype=torch.bool)
        inside[1:, :, 1:h + 1, 3:w + 3] = True
        assert bool(torch.isnan(big[~inside]).all()) and np.array_equal(view.cpu().numpy().view(U32), flows.view(U32))
        none = eng.flow_project_tensor(view[:0], coverage=True)
        assert none[0].shape == (0, 2, h, w) and none[1].shape == (0, h, w) and none[2].shape == (0, h, w)
        assert eng.device_bytes() == before and eng.stats().pairs == 0


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h = 97, 61
    flows, imp, occ = R.project_inputs(w, h)
    nan, inf = float("nan"), float("inf")
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        rig = _Rig(eng, flows, imp, occ, "vector")
        big = 1 << 20
        try:
            before, stats = eng.device_bytes(), bytes(eng.stats())
            refused = [dict(d_flow_ptr=None), dict(d_work_ptr=None), dict(outputs=()), dict(n=-1),
                       dict(t=0.0), dict(t=-0.0), dict(t=nan), dict(t=inf), dict(t=-inf), dict(scale=nan), dict(scale=inf),
                       dict(min_weight=-1e-6), dict(min_weight=nan), dict(min_weight=inf),
                       dict(d_out_ptr=rig.flow.ptr()),
                       dict(d_work_ptr=rig.work.ptr(4)), dict(d_work_ptr=rig.work.ptr(1)),
                       dict(work_bytes=rig.per - 1), dict(work_bytes=0),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=h * rig.flow.pitch - 1),
                       dict(flow_stride_floats=2 * rig.flow.plane - 1),
                       dict(out_row_pitch_floats=w - 1), dict(out_plane_stride_floats=h * rig.out.pitch - 1),
                       dict(out_flow_stride_floats=2 * rig.out.plane - 1),
                       dict(with_imp=True, importance_pitch_floats=w - 1), dict(with_imp=True, importance_stride_floats=h * rig.imp.pitch - 1),
                       dict(with_occ=True, occ_pitch=w - 1), dict(with_occ=True, occ_stride=h * rig.occ.pitch - 1),
                       dict(hole_pitch=w - 1), dict(hole_stride=h * rig.hole.pitch - 1),
                       dict(coverage_pitch_floats=w - 1), dict(coverage_stride_floats=h * rig.cov.pitch - 1),
                       dict(row_pitch_floats=big, plane_stride_floats=big)]  # a plane shorter than its rows
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    rig.call(**kw)
                assert e.value.status == 1, kw
            with pytest.raises(dfx.DfxError) as e:  # a NULL descriptor
                eng._check(eng._L.dfx_flow_project_device(eng._h, None))
            assert e.value.status == 1
            assert rig.outputs_untouched(), "a refused call wrote"
            assert np.array_equal(rig.work.get(), rig.garbage), "a refused call wrote the workspace"
            rig.call(n=0)  # DFX_OK, launches nothing
            eng.flow_project_device(None, 0, 0, 0, 0, None, 0, t=0.0, scale=nan, min_weight=-1.0)  # n = 0 comes first
            assert rig.outputs_untouched(), "n = 0 wrote"
            # the strides of absent buffers are not looked at
            rig.call(outputs=("hole",), out_row_pitch_floats=0, out_plane_stride_floats=0, out_flow_stride_floats=0,
                     coverage_pitch_floats=0, coverage_stride_floats=0, importance_pitch_floats=0, importance_stride_floats=0,
                     occ_pitch=0, occ_stride=0)
            kw = dict(t=0.5, scale=0.5, with_imp=True, with_occ=True)
            rig.check("after the refusals", _Ref(flows, imp, occ)(**kw), **kw)
            assert eng.device_bytes() == before and bytes(eng.stats()) == stats
        finally:
            rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(eng, flows, imp, occ, "vector")
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call()
            assert e.value.status == 4
            assert rig.outputs_untouched()
        finally:
            rig.close()


def test_the_hole_plane_feeds_the_median_fill_and_the_chain(dfx):
    """The polarity: 1 = no value here.  flow_median's fill replaces exactly the holes; flow_chain loses valid where a link
    samples a hole."""
    from tests import flow_chain_ref as C
    from tests.flow_median_ref import flow_median_batch

    w, h = 97, 61
    flows, _, _ = R.project_inputs(w, h)
    with dfx.FlowEngine(w, h, "farn") as eng:
        inv, hole = eng.flow_invert(flows)
        want = R.project(flows, t=1.0, scale=-1.0)
        assert R.same_bits(inv, want[0]) and R.same_bits(hole, want[1]) and 0.01 < hole.mean() < 0.6
        filled, left = eng.flow_median(inv, 5, mask=hole, mode="fill")
        wf, wl = flow_median_batch(inv, 5, hole, "fill")
        assert R.same_bits(filled, wf) and np.array_equal(left, wl)
        keep = hole == 0
        assert np.array_equal(filled[:, 0][keep].view(U32), inv[:, 0][keep].view(U32)) and left.sum() < hole.sum()
        assert (filled[:, 0][(hole != 0) & (left == 0)] != 0).any()
        out, valid = eng.flow_chain(inv, 2, occ=hole)
        wo, wv = C.chain_batch(inv, 2, occ=hole)
        assert C.same_bits(out, wo) and np.array_equal(valid, wv)
        assert valid.shape == (2, h, w) and not valid[hole[:2] != 0].any() and valid.any()
