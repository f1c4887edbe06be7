"""Batches of more than 65535 items through every launcher that puts the item index into grid.z: a launch takes at most 65535
(DFX_GRID_YZ_MAX, denseflow_amd/csrc/dfx_device.h; 32767 pairs for the interpolation, whose fill passes run over two flows per
pair), and a larger batch goes in several launches, each with every per-item pointer moved on by its first item.  One test per
launcher, driven through the raw *_device entry point, with n = c, c + 1 and 2 c + 1 items of 5 x 3 pixels (one full launch; a
second launch of exactly one item; three launches) in two layouts: "offset" (bases one element in; pitch, plane stride and
item stride odd and larger than dense: single elements, and a wrong stride lands in a gap) and "vector" (every base and stride
a multiple of 16 bytes, padded: the wide accesses).

Item i is base item i % 7 (tests/many_items_cases.py), the reference is the per-op NumPy reference on the 7 base items, and
what is compared are bit patterns, without a tolerance: every output plane and every per-item scalar (the global-motion
records, the warp statistics, the PNG bounds, the histogram sums, flow_colour's max2 words) of all n items, every element
outside the windows against the fill, the inputs against what was uploaded.  A mismatch names its first items as (i, i % 7,
i // c): the launch it fell in.  Before a handle is touched every test asserts on its reference alone that the base items
give pairwise different results (many_items_cases.check_distinct).

dfx_fb_check_device checks one direction, so its launches hold 65535 flows; the two-direction form (32767 flows per launch)
is only reached from the engines' own batches, which max_batch bounds.  The workspaces of flow_project, splat and interpolate
hold all n items, so that the cap of the grid and not the workspace sets the waves; one more case has a workspace for c + 1
items at n = 2 c + 1."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

from tests import many_items_cases as M
from tests.devmem import DevBuf

pytestmark = pytest.mark.gpu

F32, F64, U8, U32, U64, I64 = np.float32, np.float64, np.uint8, np.uint32, np.uint64, np.int64
W, H, K = M.W, M.H, M.K
G = 16  # guard elements in front of and behind every buffer
FILL = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}
LAYOUTS = ["offset", "vector"]
WARP_U8, PLANAR_F32 = 3, 0


class Win:
    """n items, each a window of `shape` elements `strides` apart, `item` elements from one item to the next, the first `lead`
    elements into a device buffer; every element outside the windows is `fill`.  data[idx[i]] is item i."""

    def __init__(self, eng, n, shape, strides, item, lead, dtype, fill=None, data=None, idx=None):
        self.dtype = np.dtype(dtype)
        self.n, self.shape, self.strides, self.item = n, tuple(shape), tuple(strides), item
        self.first = G + lead
        span = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
        assert item >= 1 and all(s >= 1 for s in shape)
        fill = FILL[self.dtype.itemsize] if fill is None else fill
        self.host = np.full(self.first + (n - 1) * item + span + G, fill, self.dtype)
        self.blank = self.host[:1].copy()
        if data is not None:
            self.view(self.host)[...] = np.asarray(data, self.dtype).reshape((-1,) + self.shape)[idx]
        self.dev = DevBuf(eng, init=self.host)
        if len(shape) == 3:
            self.plane, self.pitch = strides[0], strides[1]

    def view(self, buf):
        es = self.dtype.itemsize
        assert buf.dtype == self.dtype and buf.shape == self.host.shape
        return as_strided(buf[self.first:], (self.n,) + self.shape, (self.item * es,) + tuple(s * es for s in self.strides))

    def ptr(self):
        return self.dev.ptr(self.first * self.dtype.itemsize)

    def untouched(self):
        return bool(np.array_equal(M.bits(self.dev.get(self.dtype)), M.bits(self.host)))

    def check(self, tag, ref, idx, c, per, any_nan=False):
        """The n windows against ref[idx] as bit patterns (any_nan: a NaN of the reference stands for any NaN, as the per-op
        test has it), everything else against the fill."""
        buf = self.dev.get(self.dtype)
        got = np.ascontiguousarray(self.view(buf))
        want = M.bits(np.asarray(ref).reshape((-1,) + self.shape))[idx]
        assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
        bad = got != want
        if any_nan:
            nan = np.isnan(want.view(F32))
            bad = np.where(nan, ~np.isnan(got.view(F32)), bad)
        if bad.any():
            items = np.flatnonzero(bad.reshape(self.n, -1).any(1))
            first = [(int(i), int(i) % per, int(i) // c) for i in items[:6]]
            i = items[0]
            raise AssertionError((tag, f"{len(items)} of {self.n} items differ; the first as (i, i % {per}, launch i // {c})", first,
                                  "got", got[i][bad[i]][:4], "want", want[i][bad[i]][:4]))
        self.view(buf)[...] = self.blank[0]
        assert np.array_equal(M.bits(buf), M.bits(np.full(buf.shape, self.blank[0], self.dtype))), \
            (tag, "an element outside the windows was written")

    def close(self):
        self.dev.close()


def _geom(layout, k, h, roww, p, itemsize):
    """(lead, pitch, plane, item) in elements of p planes of h rows of roww elements; k varies the gaps between buffers."""
    if layout == "offset":
        pitch = (roww + 1) | 1
        plane = (h * pitch + 1 + k % 3) | 1
        item = (p * plane + 1 + k % 2) | 1
        assert pitch > roww and plane > h * pitch and item > p * plane and pitch % 2 and plane % 2 and item % 2
        return 1, pitch, plane, item
    q = 16 // itemsize
    pitch = (roww // q + 1) * q
    plane = h * pitch + q
    return 0, pitch, plane, p * plane + q


class Rig:
    """The buffers of one call; closes them all."""

    def __init__(self, eng, op, kn, layout, n=None):
        self.eng, self.op, self.layout = eng, op, layout
        self.c, self.per = M.chunk(op), M.period(op)
        self.n = M.counts(self.c)[kn] if n is None else n
        self.idx = np.arange(self.n) % self.per
        self.tag = (op, layout, self.n)
        self.wins, self.inputs, self.k = [], [], 0

    def planes(self, p, roww, dtype, data=None, fill=None, h=H, n=None, idx=None, like=None):
        """n items of p planes of h rows of roww elements.  With data an input ((K, p, h, roww) base items; the padding is NaN
        or 0xFF, so a read of it would show), without an output (bit patterns; the fill).  like: a buffer whose strides this
        one shares."""
        dtype = np.dtype(dtype)
        lead, pitch, plane, item = like.geom if like else _geom(self.layout, self.k, h, roww, p, dtype.itemsize)
        self.k += 1
        if data is not None and fill is None:
            fill = np.nan if dtype == F32 else 0xFF
        w = Win(self.eng, self.n if n is None else n, (p, h, roww), (plane, pitch, 1), item, lead, dtype, fill, data,
                self.idx if idx is None else idx)
        w.geom = (lead, pitch, plane, item)
        if self.layout == "vector":
            assert w.ptr() % 16 == 0 and (pitch * dtype.itemsize) % 16 == 0 and (item * dtype.itemsize) % 16 == 0
        else:
            assert w.ptr() % (2 * dtype.itemsize) == dtype.itemsize
        return self.add(w, data is not None)

    def dense(self, per_item, dtype, lead=0, n=None):
        """n x per_item words back to back (per-item scalars), `lead` elements in."""
        return self.add(Win(self.eng, self.n if n is None else n, (per_item,), (1,), per_item, lead, dtype), False)

    def add(self, w, is_input):
        self.wins.append(w)
        if is_input:
            self.inputs.append(w)
        return w

    def work(self, per, items, offset):
        """A workspace of per * items bytes of garbage, `offset` bytes in."""
        nbytes = per * items
        w = DevBuf(self.eng, nbytes=nbytes + 32)
        self.wins.append(w)
        return w.ptr(offset), nbytes

    def check(self, win, name, ref, **kw):
        win.check(self.tag + (name,), ref, kw.pop("idx", self.idx), self.c, self.per, **kw)

    def inputs_untouched(self):
        for w in self.inputs:
            assert w.untouched(), (self.tag, "an input was written")

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for w in self.wins:
            w.close()


@pytest.fixture(scope="module")
def eng(dfx, oracle):  # the oracle first: its worker pool exists before the HIP runtime starts
    with dfx.FlowEngine(97, 61, "farn") as e:
        e.set_size(W, H)
        yield e


def _hwc(a):
    """(K, H, W, 3) images as one plane of rows of 3 W bytes."""
    return a.reshape(len(a), 1, a.shape[1], 3 * a.shape[2])


both = pytest.mark.parametrize("layout", LAYOUTS)
three = pytest.mark.parametrize("kn", [0, 1, 2], ids=["c", "c+1", "2c+1"])


@both
@three
def test_fb_check(eng, kn, layout):
    ref, b = M.check_distinct("fb_check"), M.base()
    with Rig(eng, "fb_check", kn, layout) as r:
        fwd = r.planes(2, W, F32, b["flows"])
        bwd = r.planes(2, W, F32, b["back"], like=fwd)
        occ, err = r.planes(1, W, U8), r.planes(1, W, U32)
        assert (fwd.pitch, fwd.plane, fwd.item) == (bwd.pitch, bwd.plane, bwd.item)
        eng.fb_check_device(fwd.ptr(), bwd.ptr(), fwd.pitch, fwd.plane, fwd.item, r.n, *M.FB_ALPHAS, occ.ptr(), occ.pitch, occ.item,
                            err.ptr(), err.pitch, err.item)
        r.check(occ, "occ", ref["occ"])
        r.check(err, "err", ref["err"])
        r.inputs_untouched()


@both
@three
def test_warp(eng, kn, layout):
    ref, b = M.check_distinct("warp"), M.base()
    with Rig(eng, "warp", kn, layout) as r:
        src = r.planes(1, 3 * W, U8, _hwc(b["bgr"]))
        cmp_ = r.planes(1, 3 * W, U8, _hwc(b["bgr1"]), like=src)
        flow, occ = r.planes(2, W, F32, b["flows"]), r.planes(1, W, U8, b["masks"])
        out, valid, stats = r.planes(1, 3 * W, U32), r.planes(1, W, U8), r.dense(2, U64)
        assert (src.pitch, src.item) == (cmp_.pitch, cmp_.item)  # the reference images share the sources' strides
        eng.warp_device(src.ptr(), 3, 0, src.pitch, 0, src.item, flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, border=0,
                        out_dtype=PLANAR_F32, d_out_ptr=out.ptr(), out_pitch=out.pitch, out_plane_stride=0, out_image_stride=out.item,
                        d_ref_ptr=cmp_.ptr(), d_occ_ptr=occ.ptr(), occ_pitch=occ.pitch, occ_stride=occ.item, d_valid_ptr=valid.ptr(),
                        valid_pitch=valid.pitch, valid_stride=valid.item, d_stats_ptr=stats.ptr())
        r.check(out, "out", ref["out"])
        r.check(valid, "valid", ref["valid"])
        r.check(stats, "stats", ref["stats"])
        r.inputs_untouched()


@both
@three
@pytest.mark.parametrize("emit", ["last", "all"])
def test_flow_chain(eng, emit, kn, layout):
    """n anchors over a periodic list of n + 2 flows; under "all" an anchor's three chains lie one output stride apart."""
    ref, b = M.check_distinct("flow_chain"), M.base()
    L = M.CHAIN_LENGTH
    with Rig(eng, "flow_chain", kn, layout) as r:
        n_flows = r.n + L - 1
        fidx = np.arange(n_flows) % K
        flow = r.planes(2, W, F32, b["small"], n=n_flows, idx=fidx)
        occ = r.planes(1, W, U8, b["sparse"], n=n_flows, idx=fidx)
        per = L if emit == "all" else 1
        out, valid = r.planes(2, W, U32, n=r.n * per), r.planes(1, W, U8, n=r.n * per)
        eng.flow_chain_device(flow.ptr(), flow.pitch, flow.plane, flow.item, n_flows, out.ptr(), out.pitch, out.plane, out.item, L,
                              first=0, hop=1, anchors=r.n, anchor_step=1, emit=int(emit == "all"), border=0, d_occ_ptr=occ.ptr(),
                              occ_pitch=occ.pitch, occ_stride=occ.item, d_valid_ptr=valid.ptr(), valid_pitch=valid.pitch,
                              valid_stride=valid.item)
        # output e = anchor e // per, link e % per: reference row (e // per) % 7 * per + e % per
        e = np.arange(r.n * per)
        idx = (e // per) % K * per + e % per
        r.c = r.c * per  # outputs per launch
        r.check(out, emit, ref[emit], idx=idx, any_nan=True)
        r.check(valid, emit + "_valid", ref[emit + "_valid"], idx=idx)
        r.inputs_untouched()


@both
@three
def test_flow_median(eng, kn, layout):
    ref, b = M.check_distinct("flow_median"), M.base()
    with Rig(eng, "flow_median", kn, layout) as r:
        flow, mask = r.planes(2, W, F32, b["flows"]), r.planes(1, W, U8, b["dense"])
        out, mask_out = r.planes(2, W, U32), r.planes(1, W, U8)
        eng.flow_median_device(flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, out.ptr(), out.pitch, out.plane, out.item,
                               ksize=M.MEDIAN_KSIZE, mode=1, d_mask_ptr=mask.ptr(), mask_pitch=mask.pitch, mask_stride=mask.item,
                               d_mask_out_ptr=mask_out.ptr(), mask_out_pitch=mask_out.pitch, mask_out_stride=mask_out.item)
        r.check(out, "out", ref["out"])
        r.check(mask_out, "mask_out", ref["mask_out"])
        r.inputs_untouched()


@both
@three
def test_global_motion(eng, kn, layout):
    ref, b = M.check_distinct("global_motion"), M.base()
    size = ref["rec"].dtype.itemsize
    with Rig(eng, "global_motion", kn, layout) as r:
        flow, mask = r.planes(2, W, F32, b["flows"]), r.planes(1, W, U8, b["masks"])
        out, moving, rec = r.planes(2, W, U32), r.planes(1, W, U8), r.dense(size, U8)
        eng.global_motion_device(flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, rec.ptr(), M.GM["model"], M.GM["rounds"],
                                 M.GM["thr"], M.GM["growth"], mask.ptr(), mask.pitch, mask.item, out.ptr(), out.pitch, out.plane,
                                 out.item, moving.ptr(), moving.pitch, moving.item)
        r.check(rec, "records", ref["rec"].view(U8).reshape(K, size))
        r.check(out, "out", ref["out"])
        r.check(moving, "moving", ref["moving"])
        r.inputs_untouched()


@both
@three
@pytest.mark.parametrize("norm", ["flow", "batch"])
def test_flow_colour(eng, norm, kn, layout):
    """The last flow of the batch is not periodic: it alone has the largest magnitude, so that under "batch" every image,
    those of the first launch too, depends on what the last launch measured."""
    ref, b = M.check_distinct("flow_colour"), M.base()
    with Rig(eng, "flow_colour", kn, layout) as r:
        idx = r.idx.copy()
        idx[-1] = K
        flow = r.planes(2, W, F32, np.concatenate([b["flows"], b["last"][None]]), idx=idx)
        mask = r.planes(1, W, U8, np.concatenate([b["masks"], b["masks"][3:4]]), idx=idx)
        out = r.planes(1, 3 * W, U8)
        max2 = r.add(Win(eng, 1, (r.n + 1,), (1,), r.n + 1, 0, U32), False)
        eng.flow_colour_device(flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, out.ptr(), out.pitch, 0, out.item,
                               norm={"flow": 1, "batch": 2}[norm], d_max2_ptr=max2.ptr(), order=1, layout=0,
                               unknown=M.COLOUR_UNKNOWN, d_mask_ptr=mask.ptr(), mask_pitch=mask.pitch, mask_stride=mask.item)
        r.check(out, norm, ref[norm], idx=idx)
        m2 = ref[norm + "_max2"]
        words = np.concatenate([m2[idx], m2[K + 1:]])  # the n per-flow words, then the batch's
        got = max2.dev.get(U32)[max2.first:max2.first + r.n + 1]
        bad = np.flatnonzero(got != words.view(U32))
        assert not len(bad), (r.tag, "max2", [(int(i), int(i) % K, int(i) // r.c) for i in bad[:6]], got[bad][:4], words.view(U32)[bad][:4])
        r.check(max2, "max2", words[None], idx=np.zeros(1, I64))
        r.inputs_untouched()


@both
@three
def test_flow_hist(eng, kn, layout):
    ref, b = M.check_distinct("flow_hist"), M.base()
    D, CH, CW = ref["out"].shape[1:]
    assert (CH, CW) == (1, 2)
    with Rig(eng, "flow_hist", kn, layout) as r:
        flow, mask = r.planes(2, W, F32, b["flows"]), r.planes(1, W, U8, b["masks"])
        if layout == "vector":  # (n, D, CH, CW) with padded rows and planes
            lead, col, row = 0, 1, CW + 3
            slot = CH * row + 5
            item = D * slot + 7
        else:  # (n, CH, CW, D) with padded cells, one float in
            lead, slot, col = 1, 1, D + 2
            row = CW * col + 3
            item = CH * row + 1
        out = r.add(Win(eng, r.n, (D, CH, CW), (slot, row, col), item, lead, U32), False)
        sums = r.add(Win(eng, r.n, (CH * CW * D,), (1,), CH * CW * D + (3 if layout == "offset" else 2), 0, U64), False)
        eng.flow_hist_device(flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, M.HIST["kinds"], M.HIST["cell"], M.HIST["bins"],
                             M.HIST["still_thr"], {"none": 0, "l1": 1, "l1_sqrt": 2, "l2": 3}[M.HIST["norm"]], sums.ptr(), sums.item,
                             out.ptr(), slot, col, row, item, mask.ptr(), mask.pitch, mask.item)
        r.check(sums, "sums", ref["sums"])
        r.check(out, "out", ref["out"])
        r.inputs_untouched()


WORK = pytest.mark.parametrize("kn,work_items", [(0, None), (1, None), (2, None), (2, 1)], ids=["c", "c+1", "2c+1", "2c+1-work-c+1"])


def _work_items(r, work_items):
    """A workspace for all n items, or for c + 1 of them."""
    return r.n if work_items is None else r.c + 1


@both
@WORK
def test_flow_project(eng, kn, work_items, layout):
    ref, b = M.check_distinct("flow_project"), M.base()
    with Rig(eng, "flow_project", kn, layout) as r:
        flow, imp, occ = r.planes(2, W, F32, b["flows"]), r.planes(1, W, F32, b["imp"]), r.planes(1, W, U8, b["masks"])
        out, hole, cov = r.planes(2, W, U32), r.planes(1, W, U8), r.planes(1, W, U32)
        work, work_bytes = r.work(eng.flow_project_work_bytes(), _work_items(r, work_items), 8 if layout == "offset" else 0)
        eng.flow_project_device(flow.ptr(), flow.pitch, flow.plane, flow.item, r.n, work, work_bytes, M.PROJECT["t"],
                                M.PROJECT["scale"], M.PROJECT["min_weight"], out.ptr(), out.pitch, out.plane, out.item, hole.ptr(),
                                hole.pitch, hole.item, cov.ptr(), cov.pitch, cov.item, imp.ptr(), imp.pitch, imp.item, occ.ptr(),
                                occ.pitch, occ.item)
        r.check(out, "out", ref["out"])
        r.check(hole, "hole", ref["hole"])
        r.check(cov, "cov", ref["cov"])
        r.inputs_untouched()


@both
@WORK
def test_splat(eng, kn, work_items, layout):
    ref, b = M.check_distinct("splat"), M.base()
    with Rig(eng, "splat", kn, layout) as r:
        src, flow = r.planes(1, 3 * W, U8, _hwc(b["bgr"])), r.planes(2, W, F32, b["flows"])
        imp, occ = r.planes(1, W, F32, b["imp"]), r.planes(1, W, U8, b["masks"])
        out, hole, cov = r.planes(1, 3 * W, U32), r.planes(1, W, U8), r.planes(1, W, U32)
        work, work_bytes = r.work(eng.splat_work_bytes(3), _work_items(r, work_items), 8 if layout == "offset" else 0)
        eng.splat_device(d_src_ptr=src.ptr(), src_dtype=WARP_U8, channels=3, layout=0, src_pitch=src.pitch, src_plane_stride=0,
                         src_image_stride=src.item, d_flow_ptr=flow.ptr(), row_pitch_floats=flow.pitch,
                         plane_stride_floats=flow.plane, flow_stride_floats=flow.item, n=r.n, d_work_ptr=work, work_bytes=work_bytes,
                         t=M.SPLAT["t"], min_weight=M.SPLAT["min_weight"], mode=0, hole_mode=0, out_dtype=PLANAR_F32,
                         d_out_ptr=out.ptr(), out_pitch=out.pitch, out_plane_stride=0, out_image_stride=out.item,
                         d_hole_ptr=hole.ptr(), hole_pitch=hole.pitch, hole_stride=hole.item, d_coverage_ptr=cov.ptr(),
                         coverage_pitch_floats=cov.pitch, coverage_stride_floats=cov.item, d_importance_ptr=imp.ptr(),
                         importance_pitch_floats=imp.pitch, importance_stride_floats=imp.item, d_occ_ptr=occ.ptr(),
                         occ_pitch=occ.pitch, occ_stride=occ.item)
        r.check(out, "out", ref["out"])
        r.check(hole, "hole", ref["hole"])
        r.check(cov, "cov", ref["cov"])
        r.inputs_untouched()


@both
@WORK
def test_interpolate(eng, kn, work_items, layout):
    """Pair i is base item i % 6: 7 divides the 32767 pairs of a launch (many_items_cases.period)."""
    ref, b = M.check_distinct("interpolate"), M.base()
    with Rig(eng, "interpolate", kn, layout) as r:
        assert r.per == 6 and r.c == 32767
        img0, fwd, of = r.planes(1, 3 * W, U8, _hwc(b["bgr"])), r.planes(2, W, F32, b["flows"]), r.planes(1, W, U8, b["masks"])
        img1, bwd = r.planes(1, 3 * W, U8, _hwc(b["bgr1"]), like=img0), r.planes(2, W, F32, b["back"], like=fwd)
        ob = r.planes(1, W, U8, b["masks_b"], like=of)
        out, source = r.planes(1, 3 * W, U8), r.planes(1, W, U8)
        assert (img0.pitch, img0.item, fwd.pitch, fwd.plane, fwd.item, of.pitch, of.item) == \
            (img1.pitch, img1.item, bwd.pitch, bwd.plane, bwd.item, ob.pitch, ob.item)  # one set of strides per kind
        work, work_bytes = r.work(eng.interpolate_work_bytes(M.INTERP["fill_passes"]), _work_items(r, work_items),
                                  8 if layout == "offset" else 0)
        eng.interpolate_device(img0.ptr(), img1.ptr(), 3, 0, img0.pitch, 0, img0.item, fwd.ptr(), bwd.ptr(), fwd.pitch, fwd.plane,
                               fwd.item, r.n, work, work_bytes, M.INTERP["t"], M.INTERP["min_weight"], M.INTERP["fill_passes"],
                               M.INTERP["ksize"], of.ptr(), ob.ptr(), of.pitch, of.item, WARP_U8, out.ptr(), out.pitch, 0, out.item,
                               source.ptr(), source.pitch, source.item)
        r.check(out, "out", ref["out"])
        r.check(source, "source", ref["source"])
        r.inputs_untouched()


def _dense_flows(r, scale=1.0):
    """The (H, W, 2) flows of the bounding calls: dense rows, a flow stride of the layout."""
    stride = 2 * W * H + (3 if r.layout == "offset" else 2)  # 30 floats: 33 (single elements), 32 (16-byte multiples)
    return r.add(Win(r.eng, r.n, (2 * W * H,), (1,), stride, 1 if r.layout == "offset" else 0, F32, np.nan,
                     M.hwc_flows(scale).reshape(K, -1), r.idx), True)


@both
@three
def test_flow_to_u8(eng, kn, layout):
    ref = M.check_distinct("flow_to_u8")
    with Rig(eng, "flow_to_u8", kn, layout) as r:
        flow, x = _dense_flows(r), r.planes(1, W, U8)
        y = r.planes(1, W, U8, like=x)
        assert (x.pitch, x.item) == (y.pitch, y.item)
        eng.flow_to_u8_device(flow.ptr(), flow.item, r.n, *M.U8_BOUNDS, x.ptr(), y.ptr(), x.pitch, x.item)
        r.check(x, "x", ref["x"])
        r.check(y, "y", ref["y"])
        r.inputs_untouched()


@both
@three
def test_flow_to_png(eng, kn, layout):
    """The planes, and the two bounds per flow.  A 5 x 3 frame has the bounds (4, 4) and (12, 4) and no other: both occur and
    no shift of the batch maps them onto themselves (many_items_cases.check_distinct); the planes differ pairwise."""
    ref = M.check_distinct("flow_to_png")
    with Rig(eng, "flow_to_png", kn, layout) as r:
        flow, x, bounds = _dense_flows(r, M.PNG_SCALE), r.planes(1, W, U8), r.dense(2, U64)
        y = r.planes(1, W, U8, like=x)
        assert (x.pitch, x.item) == (y.pitch, y.item)
        eng.flow_to_png_device(flow.ptr(), flow.item, r.n, x.ptr(), y.ptr(), x.pitch, x.item, bounds.ptr())
        r.check(bounds, "bounds", ref["bounds"])
        r.check(x, "x", ref["x"])
        r.check(y, "y", ref["y"])
        r.inputs_untouched()


@both
@three
def test_prepare_frames(eng, kn, layout):
    """Both launchers of the frame preparation: 4 x 2 B, G, R sources to 5 x 3 gray frames, and to 5 x 3 B, G, R frames."""
    ref, b = M.check_distinct("prepare"), M.base()
    with Rig(eng, "prepare", kn, layout) as r:
        src = r.planes(1, 3 * M.SW, U8, _hwc(b["source"]), h=M.SH)
        gray, bgr = r.planes(1, W, U8), r.planes(1, 3 * W, U8)
        eng.prepare_frames_device(src.ptr(), src.pitch, src.item, M.SW, M.SH, 3, r.n, gray.ptr(), gray.pitch, gray.item)
        eng.prepare_frames_bgr_device(src.ptr(), src.pitch, src.item, M.SW, M.SH, r.n, bgr.ptr(), bgr.pitch, bgr.item)
        r.check(gray, "gray", ref["gray"])
        r.check(bgr, "bgr", ref["bgr"])
        r.inputs_untouched()
