"""The flow median on the device (dfx_flow_median_device, denseflow_amd/csrc/flow_median_kernels.hip) against its NumPy
restatement (tests/flow_median_ref.py): u, v as bit patterns and mask_out byte for byte, every element outside the windows
of an output buffer still the fill, the inputs untouched.  ksize {3, 5} x mode {all, fill} x masks {none, random 30 %, blobs,
all ones, all zeros}; shapes narrower than the window, 97 x 61 and 130 x 97, and one below / at / above the kernel's 64 x 16
tile in each direction; three flows with gaps between them in a layout that takes the single-element path (row pitch W + 3,
bases one element in) and one that takes the 16-byte path; special values and random bit patterns; the wrappers; every
refusal."""
import numpy as np
import pytest

from tests import flow_median_ref as R
from tests.devmem import DevBuf
from tests.test_global_motion_gpu import _Planes

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
TILE_W, TILE_H = 64, 16  # FM_TILE_W, FM_TILE_H of flow_median_kernels.h
OUT_FILL, MASK_FILL = 0xA5A5A5A5, 0xA5
MASKS = ["random", "blobs", "ones", "zeros"]
TINY = [(1, 1), (2, 3), (5, 1), (1, 7), (3, 3)]  # (w, h): windows wider than the frame
TILES = [(TILE_W - 1, 9), (TILE_W, 9), (TILE_W + 1, 9), (9, TILE_H - 1), (9, TILE_H), (9, TILE_H + 1), (9, 2 * TILE_H + 1)]


def _random_bits(rng, shape):
    """Random bit patterns as float32: every class of value occurs (about 1 in 128 a NaN or an infinity, 1 in 256 subnormal)."""
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32).view(F32)


def _mask(rng, kind, n, h, w):
    if kind == "random":
        return (rng.random((n, h, w)) < 0.3).astype(np.uint8)
    if kind == "blobs":
        m = np.stack([R.blob_mask(rng, h, w) for _ in range(n)])
        return (m * rng.integers(1, 256, (n, h, w))).astype(np.uint8)  # any nonzero byte excludes
    return np.full((n, h, w), 1 if kind == "ones" else 0, np.uint8)


class _Rig:
    """The device buffers of one batch of flows (n, 2, H, W) and optional masks (n, H, W) in one layout."""

    def __init__(self, eng, flows, masks=None, layout="vector"):
        self.eng, self.flows, self.masks = eng, flows, masks
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
        self.mask = _Planes(eng, n, 1, h, w, np.uint8, 1, masks.reshape(n, 1, h, w), **gm) if masks is not None else None
        self.out = _Planes(eng, n, 2, h, w, U32, OUT_FILL, **go)
        self.mask_out = _Planes(eng, n, 1, h, w, np.uint8, MASK_FILL, **gv)
        self.bufs = [b for b in (self.flow, self.mask, self.out, self.mask_out) if b is not None]
        if layout == "scalar":
            assert self.flow.ptr() % 16 == 4 and self.flow.pitch == w + 3 and self.mask_out.ptr() % 4 == 1
        else:
            assert all(b.ptr() % 16 == 0 for b in self.bufs)

    def call(self, ksize=5, mode=R.ALL, with_mask=True, want_mask_out=True, **over):
        m = self.mask if with_mask else None
        mo = self.mask_out if (want_mask_out and m is not None) else None
        kw = dict(d_flow_ptr=self.flow.ptr(), row_pitch_floats=self.flow.pitch, plane_stride_floats=self.flow.plane,
                  flow_stride_floats=self.flow.item, n=self.n, d_out_ptr=self.out.ptr(), out_row_pitch_floats=self.out.pitch,
                  out_plane_stride_floats=self.out.plane, out_flow_stride_floats=self.out.item, ksize=ksize, mode=mode,
                  d_mask_ptr=m.ptr() if m else None, mask_pitch=m.pitch if m else 0, mask_stride=m.item if m else 0,
                  d_mask_out_ptr=mo.ptr() if mo else None, mask_out_pitch=self.mask_out.pitch,
                  mask_out_stride=self.mask_out.item)
        kw.update(over)
        self.eng.flow_median_device(**kw)

    def check(self, tag, ksize, mode="all", with_mask=True, want_mask_out=True):
        with_mask = with_mask and self.mask is not None
        self.reset()
        self.call(ksize, R.MODES[mode], with_mask, want_mask_out)
        want, want_mo = R.flow_median_batch(self.flows, ksize, self.masks if with_mask else None, mode)
        got, clean = self.out.windows()
        bad = got != want.view(U32)
        assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want.view(U32)[bad][:4])
        assert clean, (tag, "an element outside the windows of out was written")
        if with_mask and want_mask_out:
            got, clean = self.mask_out.windows()
            assert np.array_equal(got[:, 0], want_mo), (tag, "mask_out")
            assert clean, (tag, "a byte outside the windows of mask_out was written")
        else:
            assert self.mask_out.untouched(), (tag, "mask_out was written without being asked for")
        assert self.flow.untouched(), (tag, "the flows were written")
        if self.mask is not None:
            assert self.mask.untouched(), (tag, "the masks were written")
        return want, want_mo

    def reset(self):
        e = self.eng
        for b in (self.out, self.mask_out):
            e._check(e._L.dfx_memcpy_h2d(e._h, b.dev.ptr(), b.fill.ctypes.data, b.fill.nbytes))

    def close(self):
        for b in self.bufs:
            b.close()


def _grid(eng, flows, rng, layouts=("scalar", "vector"), kinds=MASKS, tag=()):
    """ksize x mode x masks (and no mask) on these flows in these layouts."""
    n, _, h, w = flows.shape
    for layout in layouts:
        rig = _Rig(eng, flows, None, layout)
        try:
            for ksize in (3, 5):
                rig.check(tag + (w, h, layout, ksize, "no mask"), ksize)
        finally:
            rig.close()
        for kind in kinds:
            rig = _Rig(eng, flows, _mask(rng, kind, n, h, w), layout)
            try:
                for ksize in (3, 5):
                    for mode in ("all", "fill"):
                        rig.check(tag + (w, h, layout, ksize, mode, kind), ksize, mode)
            finally:
                rig.close()


def test_the_whole_grid_at_97x61_on_a_tvl1_handle(dfx):
    rng = np.random.default_rng(9761)
    flows = rng.standard_normal((3, 2, 61, 97)).astype(F32)
    flows[1] = np.rint(flows[1] * 4) / 4  # many ties, -0 among them
    with dfx.FlowEngine(97, 61, "tvl1") as eng:
        before, stats = eng.device_bytes(), bytes(eng.stats())
        _grid(eng, flows, rng)
        rig = _Rig(eng, flows, _mask(rng, "blobs", 3, 61, 97), "vector")
        try:
            held = eng.device_bytes()
            rig.check("without mask_out", 5, "fill", want_mask_out=False)
            rig.check("a mask that is there but not passed", 3, "all", with_mask=False)
            assert eng.device_bytes() == held, "the call allocated"
        finally:
            rig.close()
        assert eng.device_bytes() == before and bytes(eng.stats()) == stats, "dfx_get_stats or dfx_device_bytes changed"


def test_every_shape_on_a_farneback_handle_resized(dfx):
    """One handle, dfx_set_size per shape: frames narrower than the window, 130 x 97, and the tile's edges in both directions."""
    rng = np.random.default_rng(13097)
    with dfx.FlowEngine(130, 97, "farn") as eng:
        flows = rng.standard_normal((3, 2, 97, 130)).astype(F32)
        _grid(eng, flows, rng, kinds=["blobs"])
        for w, h in TINY + TILES:
            eng.set_size(w, h)
            flows = (np.rint(rng.standard_normal((3, 2, h, w)) * 8) / 8).astype(F32)
            _grid(eng, flows, rng, kinds=["random", "ones"] if (w, h) in TINY else ["random"])


def test_special_values_and_random_bit_patterns(dfx):
    rng = np.random.default_rng(77)
    special = R.special_field()  # (2, 6, 7)
    with dfx.FlowEngine(7, 6, "farn") as eng:
        flows = np.stack([special, special[::-1].copy(), special[:, ::-1, :].copy()])
        _grid(eng, flows, rng, kinds=["random", "zeros"], tag=("special",))
        eng.set_size(TILE_W + 3, TILE_H + 3)
        flows = _random_bits(rng, (3, 2, TILE_H + 3, TILE_W + 3))
        assert np.isnan(flows).sum() > 20 and (np.abs(flows[np.isfinite(flows)]) < 1.2e-38).sum() > 10
        flows.view(U32)[0, 0, 4, 5:9] = 0x7FFFFFFF  # real samples whose key is the excluded key
        _grid(eng, flows, rng, kinds=["random", "blobs"], tag=("bits",))


def test_numpy_wrapper_and_passes(dfx):
    rng = np.random.default_rng(21)
    flows = rng.standard_normal((2, 2, 21, 21)).astype(F32)
    mask = np.zeros((2, 21, 21), np.uint8)
    mask[0, 7:14, 7:14] = 1
    mask[1, 2:19, 3:20] = 7
    with dfx.FlowEngine(21, 21, "tvl1") as eng:
        before = eng.device_bytes()
        for ksize, mode, passes in ((5, "fill", 1), (5, "fill", 2), (5, "fill", 3), (3, "fill", 4), (3, "all", 3), (5, "all", 2)):
            out, mo = eng.flow_median(flows, ksize, mask, mode, passes)
            want, want_mo = R.flow_median_batch(flows, ksize, mask, mode, passes)
            assert np.array_equal(out.view(U32), want.view(U32)) and np.array_equal(mo, want_mo), (ksize, mode, passes)
        out, mo = eng.flow_median(flows, 5, mask, "fill", 64)  # stops once the mask is empty
        want, want_mo = R.flow_median_batch(flows, 5, mask, "fill", 64)
        assert np.array_equal(out.view(U32), want.view(U32)) and not mo.any() and not want_mo.any()
        out, none = eng.flow_median(flows, 3, passes=2)
        assert none is None and np.array_equal(out.view(U32), R.flow_median_batch(flows, 3, None, "all", 2)[0].view(U32))
        empty = eng.flow_median(np.zeros((0, 2, 21, 21), F32))
        assert empty[0].shape == (0, 2, 21, 21) and empty[1] is None
        assert eng.device_bytes() == before and eng.stats().pairs == 0


def test_torch_wrapper_two_fill_passes_on_a_strided_slice(dfx):
    import torch

    rng = np.random.default_rng(5)
    h, w = 61, 97
    flows = rng.standard_normal((3, 2, h, w)).astype(F32)
    masks = np.stack([R.blob_mask(rng, h, w, 0.35) for _ in range(3)])
    masks[0, 20:31, 40:51] = 1  # an 11 x 11 hole: its 3 x 3 core is still without a value after two passes of r = 2
    want, want_mo = R.flow_median_batch(flows, 5, masks, "fill", 2)
    assert want_mo.any(), "two passes must not be enough here, or the early stop is all this checks"
    dev = torch.device("cuda", 0)
    big = torch.full((3, 2, h + 2, w + 7), float("nan"), device=dev)
    big[:, :, 1:h + 1, 3:w + 3] = torch.from_numpy(flows).to(dev)
    view = big[:, :, 1:h + 1, 3:w + 3]
    big_mask = torch.ones((3, h + 1, w + 3), dtype=torch.uint8, device=dev)
    big_mask[:, :h, 2:w + 2] = torch.from_numpy(masks).to(dev)
    into = torch.full((3, 2, h + 1, w + 5), -7.0, device=dev)
    with dfx.FlowEngine(w, h, "farn") as eng:
        out, mo = eng.flow_median_tensor(view, 5, big_mask[:, :h, 2:w + 2], "fill", 2)
        assert out.is_contiguous() and out.shape == (3, 2, h, w) and mo.dtype == torch.uint8 and mo.shape == (3, h, w)
        assert np.array_equal(out.cpu().numpy().view(U32), want.view(U32))
        assert np.array_equal(mo.cpu().numpy(), want_mo)
        # into a slice, one and three passes (the last pass writes `out` itself), nothing outside it changes
        for passes in (1, 3):
            ref, ref_mo = R.flow_median_batch(flows, 3, masks, "all", passes)
            same, mo = eng.flow_median_tensor(view, 3, big_mask[:, :h, 2:w + 2], "all", passes, out=into[:, :, 1:, 2:w + 2])
            assert same.data_ptr() == into[:, :, 1:, 2:w + 2].data_ptr()
            assert np.array_equal(same.contiguous().cpu().numpy().view(U32), ref.view(U32)), passes
            assert np.array_equal(mo.cpu().numpy(), ref_mo), passes
        frame = torch.ones_like(into, dtype=torch.bool)
        frame[:, :, 1:, 2:w + 2] = False
        assert bool((into[frame] == -7.0).all()), "written outside the slice"
        plain, none = eng.flow_median_tensor(view, 5)
        assert none is None
        assert np.array_equal(plain.cpu().numpy().view(U32), R.flow_median_batch(flows, 5)[0].view(U32))
        inside = torch.zeros_like(big, dtype=torch.bool)
        inside[:, :, 1:h + 1, 3:w + 3] = True
        assert bool(torch.isnan(big[~inside]).all()) and np.array_equal(view.cpu().numpy().view(U32), flows.view(U32))


def test_every_refusal_returns_its_status_and_leaves_the_handle_usable(dfx):
    rng = np.random.default_rng(3)
    w, h = 97, 61
    flows = rng.standard_normal((3, 2, h, w)).astype(F32)
    masks = _mask(rng, "blobs", 3, h, w)
    with dfx.FlowEngine(w, h, "tvl1") as eng:
        rig = _Rig(eng, flows, masks, "vector")
        big = 1 << 20
        try:
            refused = [dict(d_flow_ptr=None), dict(d_out_ptr=None), dict(n=-1), dict(ksize=1), dict(ksize=4), dict(ksize=7),
                       dict(ksize=0), dict(ksize=-5), dict(mode=-1), dict(mode=2),
                       dict(mode=R.FILL, d_mask_ptr=None, d_mask_out_ptr=None), dict(d_mask_ptr=None),  # mask_out without mask
                       dict(d_out_ptr=rig.flow.ptr()), dict(d_mask_out_ptr=rig.mask.ptr()),
                       dict(row_pitch_floats=w - 1), dict(plane_stride_floats=h * rig.flow.pitch - 1),
                       dict(flow_stride_floats=2 * rig.flow.plane - 1),
                       dict(out_row_pitch_floats=w - 1), dict(out_plane_stride_floats=h * rig.out.pitch - 1),
                       dict(out_flow_stride_floats=2 * rig.out.plane - 1),
                       dict(mask_pitch=w - 1), dict(mask_stride=h * rig.mask.pitch - 1),
                       dict(mask_out_pitch=w - 1), dict(mask_out_stride=h * rig.mask_out.pitch - 1),
                       dict(row_pitch_floats=big, plane_stride_floats=big)]  # a plane shorter than its rows
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    rig.call(**kw)
                assert e.value.status == 1, kw
            with pytest.raises(dfx.DfxError) as e:  # a NULL descriptor
                eng._check(eng._L.dfx_flow_median_device(eng._h, None))
            assert e.value.status == 1
            assert rig.out.untouched() and rig.mask_out.untouched(), "a refused call wrote"
            rig.call(n=0)  # DFX_OK, launches nothing
            eng.flow_median_device(None, 0, 0, 0, 0, None, 0, 0, 0, ksize=9, mode=7)  # n = 0: nothing else is looked at
            assert rig.out.untouched() and rig.mask_out.untouched(), "n = 0 wrote"
            # the strides of absent buffers are not looked at
            rig.call(with_mask=False, mask_pitch=0, mask_stride=0, mask_out_pitch=0, mask_out_stride=0)
            rig.check("after the refusals", 5, "fill")
        finally:
            rig.close()
    with dfx.FlowEngine(w, h, "frames") as eng:
        rig = _Rig(eng, flows, masks, "vector")
        try:
            with pytest.raises(dfx.DfxError) as e:
                rig.call()
            assert e.value.status == 4
            assert rig.out.untouched() and rig.mask_out.untouched()
        finally:
            rig.close()
