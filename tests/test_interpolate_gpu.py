"""The frame interpolation on the device (dfx_interpolate_device, denseflow_amd/csrc/interpolate_kernels.hip) against its NumPy
restatement (tests/interpolate_ref.py): d_out (uint8, and float32 as bit patterns) and d_source bit for bit in every case,
every element outside the windows of an output buffer still the fill, the inputs untouched.  Shapes 1 x 1, 3 x 2, 97 x 61 and
one below / at / one above the 256 x 4 pixels of a synthesis workgroup in each axis; a layout that takes the wide accesses and
one that takes single elements (odd pitches, bases one element in, a workspace 8 mod 16); gray, interleaved and planar BGR;
with and without the backward flow and the masks, passes 0 / 1 / 3, windows 3 / 5, three times; landings exactly on the last
column and row; NaN, infinities and +-1e30 in the flows and the all-holes flow; a workspace for exactly one pair and for all;
d_out only and d_source only; n = 0; every refusal; the wrappers; the blend of two dfx_warp_device outputs of the
dfx_flow_project_device flows; interpolate_frames against the held-out middle frame."""
import itertools

import numpy as np
import pytest

from tests import flow_project_ref as P
from tests import interpolate_ref as R
from tests.devmem import DevBuf
from tests.test_global_motion_gpu import _Planes

pytestmark = pytest.mark.gpu

F32, U32, U8 = np.float32, np.uint32, np.uint8
OUT_FILL, BYTE_FILL = 0xA5A5A5A5, 0xA5
SHAPES = [(1, 1), (3, 2), (97, 61), (255, 3), (256, 4), (257, 5)]  # (w, h); a synthesis workgroup owns 256 x 4 pixels
FORMS = ("gray", "il", "planar")
TS = (0.5, 0.25, 0.7)
FEW = [dict(bidir=True, masks=True, passes=3, ksize=3, t=0.5, dtype="uint8"),
       dict(bidir=False, masks=True, passes=1, ksize=5, t=0.25, dtype="float32"),
       dict(bidir=True, masks=False, passes=0, ksize=3, t=0.7, dtype="float32")]


def _inputs(w, h, form, n=2, seed=500, amp=None):
    """(img0, img1 (n, h, w[, 3]) uint8, fwd, bwd (n, 2, h, w) float32, occ_fwd, occ_bwd (n, h, w) uint8)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    shape = (n, h, w) if form == "gray" else (n, h, w, 3)
    img0, img1 = rng.integers(0, 256, shape, dtype=U8), rng.integers(0, 256, shape, dtype=U8)
    flows, _, occ = P.project_inputs(w, h, n=2 * n, seed=seed)
    if amp is not None:
        flows = flows * F32(amp)
    return img0, img1, flows[:n].copy(), flows[n:].copy(), occ[:n].copy(), occ[n:].copy()


def _planes_of(img, form):
    """(n, p, h, row elements) as _Planes takes it."""
    n, h, w = img.shape[:3]
    if form == "gray":
        return img.reshape(n, 1, h, w)
    if form == "il":
        return img.reshape(n, 1, h, 3 * w)
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2))


class _Rig:
    """The device buffers of one batch of pairs in one layout.  The two frames of a pair lie in one buffer n images apart, the
    two flows and the two masks likewise: shared strides, as a clip gives them."""

    def __init__(self, eng, inputs, form, layout="vector", passes=3, work_pairs=None, dtype="uint8"):
        img0, img1, fwd, bwd, of, ob = inputs
        self.eng, self.form, self.dtype, self.passes = eng, form, dtype, passes
        n, _, h, w = fwd.shape
        self.n, self.h, self.w = n, h, w
        p, rw = (3, w) if form == "planar" else (1, w if form == "gray" else 3 * w)
        if layout == "scalar":  # bases one element in, odd pitches, odd gaps: single elements everywhere
            gi = dict(lead=1, pitch=rw + 3, plane=h * (rw + 3) + 1, item=p * (h * (rw + 3) + 1) + 2)
            go = dict(lead=3, pitch=rw + 1, plane=h * (rw + 1) + 2, item=p * (h * (rw + 1) + 2) + 1)
            gf = dict(lead=1, pitch=w + 3, plane=h * (w + 3) + 1, item=2 * (h * (w + 3) + 1) + 5)
            gm = dict(lead=1, pitch=w + 3, item=h * (w + 3) + 2)
            gs = dict(lead=1, pitch=w + 1, item=h * (w + 1) + 3)
        else:  # "vector": every base and stride a multiple of 16 bytes (of 16 elements), rows padded, gaps between planes
            pw, pr = (w + 15) // 16 * 16 + 16, (rw + 15) // 16 * 16 + 16
            gi = go = dict(pitch=pr, plane=h * pr + 16, item=p * (h * pr + 16) + 32)
            gf = dict(pitch=pw, plane=h * pw + 16, item=2 * (h * pw + 16) + 32)
            gm = gs = dict(pitch=pw, item=h * pw + 16)
        self.p, self.rw = p, rw
        self.img = _Planes(eng, 2 * n, p, h, rw, U8, 7, np.concatenate([_planes_of(img0, form), _planes_of(img1, form)]), **gi)
        self.flow = _Planes(eng, 2 * n, 2, h, w, F32, np.nan, np.concatenate([fwd, bwd]), **gf)
        self.occ = _Planes(eng, 2 * n, 1, h, w, U8, 1, np.concatenate([of, ob]).reshape(2 * n, 1, h, w), **gm)
        self.out = _Planes(eng, n, p, h, rw, U8 if dtype == "uint8" else U32, BYTE_FILL if dtype == "uint8" else OUT_FILL, **go)
        self.source = _Planes(eng, n, 1, h, w, U8, BYTE_FILL, **gs)
        self.per = eng.interpolate_work_bytes(passes)
        self.work_bytes = self.per * (n if work_pairs is None else work_pairs)
        self.work_lead = 8 if layout == "scalar" else 0
        self.garbage = np.random.default_rng(7).integers(0, 256, self.work_bytes + 32, dtype=np.uint64).astype(U8)
        self.work = DevBuf(eng, init=self.garbage)
        self.bufs = [self.img, self.flow, self.occ, self.out, self.source, self.work]
        if layout == "scalar":
            assert self.out.ptr() % (4 if dtype == "uint8" else 16) != 0 and self.source.ptr() % 4 == 1
            assert self.work.ptr(self.work_lead) % 16 == 8
        else:
            assert all(b.ptr() % 16 == 0 for b in self.bufs)

    def call(self, bidir=True, masks=False, ksize=3, t=0.5, min_weight=0.25, outputs=("out", "source"), **over):
        n = self.n
        kw = dict(d_img0_ptr=self.img.ptr(), d_img1_ptr=self.img.ptr() + n * self.img.item, channels=1 if self.form == "gray" else 3,
                  layout=1 if self.form == "planar" else 0, img_pitch=self.img.pitch, img_plane_stride=self.img.plane if self.p == 3 else 0,
                  img_image_stride=self.img.item, d_fwd_ptr=self.flow.ptr(),
                  d_bwd_ptr=self.flow.ptr() + 4 * n * self.flow.item if bidir else None, row_pitch_floats=self.flow.pitch,
                  plane_stride_floats=self.flow.plane, flow_stride_floats=self.flow.item, n=n,
                  d_work_ptr=self.work.ptr(self.work_lead), work_bytes=self.work_bytes, t=t, min_weight=min_weight,
                  fill_passes=self.passes, ksize=ksize, d_occ_fwd_ptr=self.occ.ptr() if masks else None,
                  d_occ_bwd_ptr=self.occ.ptr() + n * self.occ.item if masks and bidir else None, occ_pitch=self.occ.pitch,
                  occ_stride=self.occ.item, out_dtype=3 if self.dtype == "uint8" else 0,
                  d_out_ptr=self.out.ptr() if "out" in outputs else None, out_pitch=self.out.pitch,
                  out_plane_stride=self.out.plane if self.p == 3 else 0, out_image_stride=self.out.item,
                  d_source_ptr=self.source.ptr() if "source" in outputs else None, source_pitch=self.source.pitch,
                  source_stride=self.source.item)
        kw.update(over)
        self.eng.interpolate_device(**kw)

    def reset(self):
        e = self.eng
        for b in (self.out, self.source):
            e._check(e._L.dfx_memcpy_h2d(e._h, b.dev.ptr(), b.fill.ctypes.data, b.fill.nbytes))

    def outputs_untouched(self):
        return self.out.untouched() and self.source.untouched()

    def inputs_untouched(self):
        return self.img.untouched() and self.flow.untouched() and self.occ.untouched()

    def check(self, tag, want, outputs=("out", "source"), **kw):
        """One call against want = (o (n, h, w[, 3]) float32, source (n, h, w)) of interpolate_ref."""
        self.reset()
        self.call(outputs=outputs, **kw)
        o = _planes_of(R.stored(want[0], self.dtype), self.form)
        for name, buf, ref in (("out", self.out, o if self.dtype == "uint8" else o.view(U32)), ("source", self.source, want[1][:, None])):
            if name in outputs:
                got, clean = buf.windows()
                bad = got != ref
                assert not bad.any(), (tag, name, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], ref[bad][:4])
                assert clean, (tag, name, "an element outside the windows was written")
            else:
                assert buf.untouched(), (tag, name, "written without being asked for")

    def close(self):
        for b in self.bufs:
            b.close()


def _want(inputs, bidir=True, masks=False, passes=3, ksize=3, t=0.5, min_weight=0.25):
    img0, img1, fwd, bwd, of, ob = inputs
    return R.interpolate_batch(img0, img1, fwd, bwd if bidir else None, of if masks else None, ob if masks and bidir else None,
                               t=t, fill_passes=passes, ksize=ksize, min_weight=min_weight)


def _run(eng, inputs, form, cases, layouts=("vector", "scalar"), tag=()):
    """Every case in every layout; the reference of a case is computed once."""
    for case in cases:
        case = dict(case)
        dtype = case.pop("dtype", "uint8")
        want = _want(inputs, **case)
        passes = case.pop("passes", 3)
        for layout in layouts:
            rig = _Rig(eng, inputs, form, layout, passes, dtype=dtype)
            try:
                rig.check(tag + (form, layout, dtype, passes, case), want, **case)
                assert rig.inputs_untouched(), (tag, layout, "the inputs were written")
            finally:
                rig.close()
        yield want


@pytest.fixture(scope="module")
def eng(dfx):
    with dfx.FlowEngine(97, 61, "farn") as e:
        yield e


@pytest.mark.parametrize("w,h", SHAPES)
def test_shapes_image_forms_and_access_widths(dfx, w, h):
    with dfx.FlowEngine(w, h, "farn") as e:
        for form in FORMS:
            inputs = _inputs(w, h, form, n=2)
            list(_run(e, inputs, form, FEW))


@pytest.mark.parametrize("bidir,masks", [(False, False), (False, True), (True, False), (True, True)])
def test_the_grid_of_call_forms(eng, bidir, masks):
    inputs = _inputs(97, 61, "gray", n=2)
    second_tier = 0
    for k, (passes, ksize, t) in enumerate(itertools.product((0, 1, 3), (3, 5), TS)):
        case = dict(bidir=bidir, masks=masks, passes=passes, ksize=ksize, t=t, dtype=("uint8", "float32")[k % 2])
        (want,) = _run(eng, inputs, "gray", [case], layouts=("vector",))
        assert passes > 0 or (want[1] <= 3).all()
        second_tier += int((want[1] >= 4).sum())
    assert bidir or second_tier > 0, "with the forward flow alone every hole is reached by the second tier only"


@pytest.mark.parametrize("form", ["gray", "il"])
def test_landings_on_the_last_column_and_row(eng, form):
    """A constant flow (2, 2) at t = 0.5 gives G0 = (-1, -1) and G1 = (+1, +1): side 1 of column W - 2 and row H - 2 samples
    exactly column W - 1 and row H - 1, one pixel further leaves the frame; (4, -4) at t = 0.25 does the same with side 0's
    column 0 and side 1's last column."""
    w, h = 97, 61
    inputs = list(_inputs(w, h, form, n=2))
    for (u, v), t in (((2.0, 2.0), 0.5), ((4.0, -4.0), 0.25), ((-4.0, 8.0), 0.25)):
        inputs[2] = np.broadcast_to(np.array([u, v], F32)[None, :, None, None], (2, 2, h, w)).copy()
        inputs[3] = -inputs[2]
        for bidir in (False, True):
            (want,) = _run(eng, inputs, form, [dict(bidir=bidir, passes=1, t=t, dtype="float32")])
            assert (want[1] == 0).any() and (want[1] != 0).any()


@pytest.mark.parametrize("w,h", [(13, 9), (97, 61)])
def test_special_flow_values_and_the_all_holes_flow(dfx, w, h):
    inputs = list(_inputs(w, h, "planar", n=2))
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 1e-40, float(w), -float(h)]
    for f in (inputs[2], inputs[3]):
        for k, v in enumerate(vals):
            f[k % 2, k % 2].reshape(-1)[(11 * k + 3) % (w * h)] = F32(v)
    with dfx.FlowEngine(w, h, "farn") as e:
        list(_run(e, inputs, "planar", FEW))
        inputs[2][...] = 1e4  # nothing lands: every pixel is a hole of both projections and falls back to its own bytes
        inputs[3][...] = -1e4
        for want in _run(e, inputs, "planar", [dict(bidir=True, passes=3), dict(bidir=False, passes=0, dtype="float32")]):
            assert (want[1] == 3).all()
        inputs[2][0] = np.nan
        for want in _run(e, inputs, "planar", [dict(bidir=False, passes=1)]):
            assert (want[1] == 3).all()


@pytest.mark.parametrize("passes", [0, 1, 3])
def test_a_workspace_for_one_pair_and_for_all(eng, passes):
    inputs = _inputs(97, 61, "il", n=3, amp=3.0)
    case = dict(bidir=passes != 1, masks=True, t=0.25)
    want = _want(inputs, passes=passes, **case)
    for layout, pairs in (("vector", 1), ("scalar", 1), ("vector", 2), ("scalar", 3), ("vector", 5)):
        rig = _Rig(eng, inputs, "il", layout, passes, work_pairs=pairs)
        try:
            rig.check((layout, pairs, passes), want, **case)
        finally:
            rig.close()


def test_out_only_source_only_and_no_pairs(eng):
    inputs = _inputs(97, 61, "gray", n=2)
    want = _want(inputs, masks=True)
    rig = _Rig(eng, inputs, "gray", "scalar")
    try:
        rig.check("out only", want, outputs=("out",), masks=True)
        rig.check("source only", want, outputs=("source",), masks=True)
        # the strides of absent buffers are not looked at
        rig.check("source only, no strides", want, outputs=("source",), masks=True, out_pitch=0, out_plane_stride=0, out_image_stride=0)
        rig.check("out only, no strides", _want(inputs), outputs=("out",), source_pitch=0, source_stride=0, occ_pitch=0, occ_stride=0)
    finally:
        rig.close()


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    w, h = 97, 61
    inputs = _inputs(w, h, "planar", n=2)
    nan, inf = float("nan"), float("inf")
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        rig = _Rig(eng, inputs, "planar", "vector")
        big = 1 << 20
        try:
            before, stats = eng.device_bytes(), bytes(eng.stats())
            refused = [dict(d_img0_ptr=None), dict(d_img1_ptr=None), dict(d_fwd_ptr=None), dict(d_work_ptr=None), dict(outputs=()),
                       dict(n=-1), dict(bidir=False, d_occ_bwd_ptr=rig.occ.ptr()),
                       dict(t=0.0), dict(t=-0.0), dict(t=1.0), dict(t=-0.5), dict(t=1.5), dict(t=nan), dict(t=inf), dict(t=-inf),
                       dict(min_weight=-1e-6), dict(min_weight=nan), dict(min_weight=inf),
                       dict(fill_passes=-1), dict(fill_passes=17), dict(ksize=1), dict(ksize=4), dict(ksize=7),
                       dict(out_dtype=1), dict(out_dtype=2), dict(out_dtype=4), dict(out_dtype=-1),
                       dict(channels=0), dict(channels=2), dict(channels=4), dict(layout=2), dict(layout=-1),
                       dict(d_work_ptr=rig.work.ptr(4)), dict(d_work_ptr=rig.work.ptr(1)),
                       dict(work_bytes=rig.per - 1), dict(work_bytes=0),
                       dict(img_pitch=w - 1), dict(img_plane_stride=h * rig.img.pitch - 1), dict(img_image_stride=3 * rig.img.plane - 1),
                       dict(layout=0, img_pitch=3 * w - 1), dict(layout=0, img_image_stride=h * rig.img.pitch - 1),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=h * rig.flow.pitch - 1),
                       dict(flow_stride_floats=2 * rig.flow.plane - 1),
                       dict(masks=True, occ_pitch=w - 1), dict(masks=True, occ_stride=h * rig.occ.pitch - 1),
                       dict(masks=True, bidir=False, occ_pitch=w - 1),
                       dict(out_pitch=w - 1), dict(out_plane_stride=h * rig.out.pitch - 1), dict(out_image_stride=3 * rig.out.plane - 1),
                       dict(source_pitch=w - 1), dict(source_stride=h * rig.source.pitch - 1),
                       dict(row_pitch_floats=big, plane_stride_floats=big)]  # a plane shorter than its rows
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    rig.call(**kw)
                assert e.value.status == 1, kw
            with pytest.raises(dfx.DfxError) as e:  # a NULL descriptor
                eng._check(eng._L.dfx_interpolate_device(eng._h, None))
            assert e.value.status == 1
            assert eng._L.dfx_interpolate_work_bytes(eng._h, None) == 0 and eng.interpolate_work_bytes(17) == 0
            assert rig.outputs_untouched(), "a refused call wrote"
            assert np.array_equal(rig.work.get(), rig.garbage), "a refused call wrote the workspace"
            rig.call(n=0)  # DFX_OK, launches nothing
            eng.interpolate_device(None, None, 0, 0, 0, 0, 0, None, None, 0, 0, 0, 0, None, 0, t=nan, fill_passes=-1)  # n = 0 comes first
            assert rig.outputs_untouched(), "n = 0 wrote"
            assert np.array_equal(rig.work.get(), rig.garbage), "n = 0 wrote the workspace"
            rig.check("after the refusals", _want(inputs, masks=True, t=0.7), masks=True, t=0.7)
            assert eng.device_bytes() == before and bytes(eng.stats()) == stats, "dfx_get_stats or dfx_device_bytes changed"
        finally:
            rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(eng, inputs, "planar", "vector")
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call()
            assert e.value.status == 4
            assert rig.outputs_untouched()
        finally:
            rig.close()


def test_the_wrappers_agree(dfx):
    import torch

    w, h, n, s = 97, 61, 3, 2
    rng = np.random.default_rng(50)
    clip = rng.integers(0, 256, (n + s, h, w, 3), dtype=U8)
    _, _, fwd, bwd, of, ob = _inputs(w, h, "il", n=n)
    dev = torch.device("cuda", 0)
    with dfx.FlowEngine(w, h, "farn") as eng:
        before = eng.device_bytes()
        for kw in (dict(), dict(t=0.25, fill_passes=0), dict(t=0.7, fill_passes=1, ksize=5, min_weight=0.0)):
            want = R.interpolate_batch(clip[:n], clip[s:], fwd, bwd, of, ob, **kw)
            got, source = eng.interpolate(clip[:n], clip[s:], fwd, bwd, occ_fwd=of, occ_bwd=ob, want_source=True, **kw)
            assert got.dtype == U8 and np.array_equal(got, R.stored(want[0], "uint8")) and np.array_equal(source, want[1])
            chw = np.ascontiguousarray(clip.transpose(0, 3, 1, 2))
            got = eng.interpolate(chw[:n], chw[s:], fwd, bwd, occ_fwd=of, occ_bwd=ob, layout="chw", dtype=np.float32, **kw)
            assert R.same_bits(got, np.ascontiguousarray(want[0].transpose(0, 3, 1, 2)))
            want1 = R.interpolate_batch(clip[:n, ..., 1], clip[s:, ..., 1], fwd, **kw)
            got = eng.interpolate(clip[:n, ..., 1], clip[s:, ..., 1], fwd, **kw)
            assert np.array_equal(got, R.stored(want1[0], "uint8"))
        # tensors: the two frames of a pair are slices of one strided clip, read without a copy
        big = torch.full((n + s, h + 2, w + 5, 3), 9, dtype=torch.uint8, device=dev)
        big[:, 1:h + 1, 2:w + 2] = torch.from_numpy(clip).to(dev)
        view = big[:, 1:h + 1, 2:w + 2]
        tf = torch.full((2, n, 2, h + 1, w + 3), float("nan"), device=dev)
        tf[0, :, :, :h, 3:], tf[1, :, :, :h, 3:] = torch.from_numpy(fwd).to(dev), torch.from_numpy(bwd).to(dev)
        tm = torch.ones((2, n, h, w + 4), dtype=torch.uint8, device=dev)
        tm[0, :, :, :w], tm[1, :, :, :w] = torch.from_numpy(of).to(dev), torch.from_numpy(ob).to(dev)
        want = R.interpolate_batch(clip[:n], clip[s:], fwd, bwd, of, ob, t=0.25)
        i0, i1 = view[:n], view[s:]
        assert i0.stride() == i1.stride() and not i0.is_contiguous()
        got, source = eng.interpolate_tensor(i0, i1, tf[0, :, :, :h, 3:], tf[1, :, :, :h, 3:], t=0.25, occ_fwd=tm[0, :, :, :w],
                                             occ_bwd=tm[1, :, :, :w], want_source=True)
        assert got.shape == (n, h, w, 3) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.stored(want[0], "uint8")) and np.array_equal(source.cpu().numpy(), want[1])
        # into a slice of a larger tensor, as float32, with a workspace of the caller's for two pairs that is 8 mod 16
        into = torch.full((n, h + 1, w + 2, 3), -7.0, device=dev)
        per = eng.interpolate_work_bytes(3)
        store = torch.zeros((2 * per // 8 + 2,), dtype=torch.int64, device=dev)
        work = store[1:] if store.data_ptr() % 16 == 0 else store[:-1]
        same = eng.interpolate_tensor(i0, i1, tf[0, :, :, :h, 3:], tf[1, :, :, :h, 3:], t=0.25, occ_fwd=tm[0, :, :, :w],
                                      occ_bwd=tm[1, :, :, :w], dtype=torch.float32, out=into[:, 1:, 1:w + 1], work=work)
        assert same.data_ptr() == into[:, 1:, 1:w + 1].data_ptr()
        assert R.same_bits(same.contiguous().cpu().numpy(), want[0])
        frame = torch.ones_like(into, dtype=torch.bool)
        frame[:, 1:, 1:w + 1] = False
        assert bool((into[frame] == -7.0).all()), "written outside the slice"
        assert bool((big[:, 0] == 9).all()) and np.array_equal(view.cpu().numpy(), clip), "the frames were written"
        # forward flow only, planar memory under a channels-last shape
        planar = torch.from_numpy(np.ascontiguousarray(clip.transpose(0, 3, 1, 2))).to(dev).permute(0, 2, 3, 1)
        want = R.interpolate_batch(clip[:n], clip[s:], fwd, t=0.7, fill_passes=1)
        got = eng.interpolate_tensor(planar[:n], planar[s:], tf[0, :, :, :h, 3:], t=0.7, fill_passes=1)
        assert got.shape == (n, h, w, 3) and np.array_equal(got.cpu().numpy(), R.stored(want[0], "uint8"))
        none = eng.interpolate_tensor(i0[:0], i1[:0], tf[0, :0, :, :h, 3:], want_source=True)
        assert none[0].shape == (0, h, w, 3) and none[1].shape == (0, h, w)
        assert eng.device_bytes() == before and eng.stats().pairs == 0


@pytest.mark.parametrize("form,layout", [("gray", "hwc"), ("il", "hwc"), ("planar", "chw")])
def test_the_call_is_the_blend_of_two_warps_of_the_projected_flows(eng, form, layout):
    """Where source is 0 both sides are primary: the stored float32 value is s0 + t (s1 - s0) of dfx_warp_device's float32
    samples of the two frames at the flows dfx_flow_project_device gives, clamped."""
    w, h, n = 97, 61, 2
    img0, img1, fwd, bwd, of, ob = _inputs(w, h, form, n=n, amp=2.0)
    if form == "planar":
        img0, img1 = (np.ascontiguousarray(a.transpose(0, 3, 1, 2)) for a in (img0, img1))
    for t in (0.5, 0.25):
        t32 = F32(t)
        t1 = F32(1) - t32
        out, source = eng.interpolate(img0, img1, fwd, bwd, t=t, occ_fwd=of, occ_bwd=ob, layout=layout, dtype=np.float32,
                                      want_source=True)
        g0, h0 = eng.flow_project(fwd, t=t, scale=float(-t32), occ=of)
        g1, h1 = eng.flow_project(bwd, t=float(t1), scale=float(-t1), occ=ob)
        s0 = eng.warp(img0, g0, dtype=np.float32, layout=layout)
        s1 = eng.warp(img1, g1, dtype=np.float32, layout=layout)
        blend = np.minimum(np.maximum(s0 + t32 * (s1 - s0), F32(0)), F32(255))
        both = source == 0
        assert 0.2 < both.mean() < 1.0 and not (both & ((h0 != 0) | (h1 != 0))).any()
        pick = both if form == "gray" else (both[:, None] if form == "planar" else both[..., None])
        pick = np.broadcast_to(pick, out.shape)
        assert np.array_equal(out[pick].view(U32), blend[pick].view(U32))


@pytest.mark.parametrize("algo", ["farn", "tvl1"])
def test_interpolate_frames_beats_the_plain_blend_on_the_held_out_frame(dfx, algo):
    from denseflow_amd.synth import SynthClip

    clip = SynthClip(97, 61, 9)
    f0, truth, f2 = clip.frames(3)
    with dfx.FlowEngine(97, 61, algo) as e:
        got = e.interpolate_frames([f0, truth, f2], step=2, ts=(0.5, 0.25))
    assert got.shape == (1, 2, 61, 97) and got.dtype == U8
    err, blend = R.mean_abs_error(got[0, 0], truth), R.mean_abs_error(R.plain_blend(f0, f2, 0.5), truth)
    print(f"interpolate_frames, {algo}, SynthClip(97, 61, 9) 0, 2 -> 1: interpolated {err:.3f}, plain blend {blend:.3f} grey levels")
    assert err < 0.5 * blend
    assert not np.array_equal(got[0, 0], got[0, 1])
