"""The inputs and references of tests/test_many_items_gpu.py: batches of more than 65535 items (flows, frames, anchors) through
the launchers that put the item index into grid.z and walk a larger batch in several launches.

Everything is 5 x 3 pixels: one workgroup per item, a quad tail of one pixel, clamped taps on every side.  K = 7 distinct base
items of every kind of input are made with a fixed seed; item i of a batch is base item i % 7 (i % 6 where a launch holds
32767 items: period()), so the phase shifts at every launch boundary, and the NumPy references (the ones the per-op GPU tests
use) run on the 7 base items only: expected[i] = ref[i % 7].  Base item 5 holds a NaN flow value and a masked pixel.

distinct() is the discrimination check: the 7 reference items of every compared output are pairwise different, so an item
that slips by one in either direction is a mismatch.  It runs on reference output alone (tests/test_many_items_ref.py runs it
without a GPU)."""
import functools

import numpy as np

from tests import fb_check_ref, flow_chain_ref, flow_colour_ref, flow_hist_ref, flow_median_ref, flow_project_ref
from tests import global_motion_ref, interpolate_ref, splat_ref, warp_ref

F32, U8, U32, I64 = np.float32, np.uint8, np.uint32, np.int64
K = 7
W, H = 5, 3
SW, SH = 4, 2            # the source size of the frame preparation
GRID_MAX = 65535         # DFX_GRID_YZ_MAX of denseflow_amd/csrc/dfx_device.h
SEED = 65535


def counts(c):
    """One full launch, a second launch of exactly one item, three launches."""
    return [c, c + 1, 2 * c + 1]


def bits(a):
    """An array as unsigned words of its element size: what is compared."""
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        return a.view(U8).reshape(a.shape + (a.dtype.itemsize,))
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def distinct(name, ref):
    """The K items of a reference output are pairwise different (NaNs compared by their bits)."""
    b = bits(ref).reshape(len(ref), -1)
    assert len(b) >= K, name
    same = [(i, j) for i in range(len(b)) for j in range(i + 1, len(b)) if np.array_equal(b[i], b[j])]
    assert not same, (name, "items that do not differ", same)


@functools.lru_cache(maxsize=None)
def base():
    """The K base items of every kind of input, read-only."""
    rng = np.random.default_rng(SEED)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    flows = np.empty((K, 2, H, W), F32)
    for i in range(K):  # a small affine (camera) part that differs per item, noise, and a few larger vectors
        a = rng.uniform(-0.15, 0.15, 6)
        flows[i, 0] = a[0] * 4 + a[1] * xx + a[2] * yy
        flows[i, 1] = a[3] * 4 + a[4] * xx + a[5] * yy
    flows += rng.normal(0, 0.1, flows.shape).astype(F32)
    big = rng.random((K, 1, H, W)) < 0.3
    flows += np.where(big, rng.uniform(-2.5, 2.5, flows.shape), 0).astype(F32)
    back = (-flows + rng.normal(0, 0.15, flows.shape) + np.where(rng.random((K, 1, H, W)) < 0.3, 1.0, 0.0)).astype(F32)
    masks = (rng.random((K, H, W)) < 0.25).astype(U8) * rng.integers(1, 256, (K, H, W)).astype(U8)
    masks_b = (rng.random((K, H, W)) < 0.25).astype(U8)
    dense = (rng.random((K, H, W)) < 0.8).astype(U8) * rng.integers(1, 256, (K, H, W)).astype(U8)  # whole windows masked
    sparse = np.zeros((K, H, W), U8)  # one masked pixel per item: a link's four taps spread it over a frame this small
    for i, (y, x) in enumerate([(0, 0), (0, 4), (2, 0), (0, 2), (2, 4), (2, 3), (1, 0)]):
        sparse[i, y, x] = 1 + i
    # towards the centre, so that most chains of three links stay in the frame (12 of the 15 pixels lie on its edge)
    pull = rng.uniform(0.05, 0.3, (K, 2, 1, 1))
    small = (pull * np.stack([2 - xx, 1 - yy]) + rng.normal(0, 0.08, flows.shape)).astype(F32)
    flows[5, 0, 1, 2] = small[5, 0, 1, 2] = np.nan
    masks[5, 2, 3] = dense[5, 2, 3] = 1
    imp = rng.uniform(0.1, 4.0, (K, H, W)).astype(F32)
    gray = rng.integers(0, 256, (K, H, W), dtype=U8)
    gray1 = rng.integers(0, 256, (K, H, W), dtype=U8)
    bgr = rng.integers(0, 256, (K, H, W, 3), dtype=U8)
    bgr1 = rng.integers(0, 256, (K, H, W, 3), dtype=U8)
    source = rng.integers(0, 256, (K, SH, SW, 3), dtype=U8)
    payload = rng.uniform(-16, 16, (K, 2, H, W)).astype(F32)
    # the one item that is not periodic (flow_colour): larger than every base item
    last = (flows[3] * F32(1.5) + F32(4.0)).astype(F32)
    d = dict(flows=flows, small=small, back=back, masks=masks, masks_b=masks_b, dense=dense, sparse=sparse, imp=imp, gray=gray, gray1=gray1, bgr=bgr, bgr1=bgr1,
             source=source, payload=payload, last=last)
    for a in d.values():
        a.setflags(write=False)
    return d


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


FB_ALPHAS = (0.05, 0.5)


@functools.lru_cache(maxsize=None)
def fb_check():
    b = base()
    occ, err = fb_check_ref.fb_check_batch(b["flows"], b["back"], *FB_ALPHAS)
    return _frozen(dict(occ=occ, err=err))


@functools.lru_cache(maxsize=None)
def warp():
    """3-channel interleaved images, border zero, with masks: float32 samples, valid, {count, sad} against bgr1."""
    b = base()
    s, valid, stats = warp_ref.warp_batch(b["bgr"], b["flows"], "zero", b["masks"], b["bgr1"])
    return _frozen(dict(out=warp_ref.stored(s, "float32"), valid=valid, stats=stats))


CHAIN_LENGTH = 3


@functools.lru_cache(maxsize=None)
def flow_chain():
    """The list of anchors + length - 1 flows is periodic, flow k being base flow k % 7: the chain from anchor j then depends
    on j % 7 only.  {emit: (chains (7 or 7 x 3, 2, H, W), valid)} from 7 anchors over 9 flows."""
    b = base()
    idx = np.arange(K + CHAIN_LENGTH - 1) % K
    every, valid = flow_chain_ref.chain_batch(b["small"][idx], CHAIN_LENGTH, 0, 1, K, 1, "all", "zero", b["sparse"][idx])
    L = CHAIN_LENGTH
    return _frozen(dict(all=every.reshape(K, L, 2, H, W), all_valid=valid.reshape(K, L, H, W), last=every[L - 1::L],
                        last_valid=valid[L - 1::L]))


MEDIAN_KSIZE = 3


@functools.lru_cache(maxsize=None)
def flow_median():
    b = base()
    out, mask_out = flow_median_ref.flow_median_batch(b["flows"], MEDIAN_KSIZE, b["dense"], "fill")
    return _frozen(dict(out=out, mask_out=mask_out))


GM = dict(model=global_motion_ref.AFFINE, rounds=3, thr=0.25, growth=2.0)


@functools.lru_cache(maxsize=None)
def global_motion():
    """out, moving and the result records (denseflow_amd.engine.GM_RESULT_DTYPE, the working words zero on return)."""
    from denseflow_amd.engine import GM_RESULT_DTYPE

    b = base()
    refs = [global_motion_ref.global_motion(b["flows"][i], b["masks"][i], GM["model"], GM["rounds"], GM["thr"], GM["growth"])
            for i in range(K)]
    rec = np.zeros(K, GM_RESULT_DTYPE)
    for i, r in enumerate(refs):
        for f in ("a", "p", "valid", "inliers", "status", "sums"):
            rec[f][i] = r[f]
        rec["rounds"][i] = GM["rounds"]
    return _frozen(dict(out=np.stack([r["out"] for r in refs]), moving=np.stack([r["moving"] for r in refs]), rec=rec))


COLOUR_UNKNOWN = (17, 99, 201)


@functools.lru_cache(maxsize=None)
def flow_colour():
    """{norm: (images (8, H, W, 3), max2 (8 + 1))} of the 7 base flows and, as item 7, the one that is not periodic: the last
    flow of a batch, the only one with the largest magnitude.  Under "batch" every other image depends on it."""
    b = base()
    flows = np.concatenate([b["flows"], b["last"][None]])
    masks = np.concatenate([b["masks"], b["masks"][3:4]])
    out = {}
    for norm in ("flow", "batch"):
        img, m2 = flow_colour_ref.flow_colour(flows, norm, None, masks, "rgb", "hwc", COLOUR_UNKNOWN)
        out[norm], out[norm + "_max2"] = img, m2
    assert m2[K] == m2[K + 1] > m2[:K].max(), "the last flow is not the only one with the largest magnitude"
    return _frozen(out)


HIST = dict(kinds=7, cell=4, bins=8, still_thr=0.4, norm="l2")


@functools.lru_cache(maxsize=None)
def flow_hist():
    b = base()
    vals, sums = flow_hist_ref.flow_hist(b["flows"], HIST["kinds"], HIST["cell"], HIST["bins"], HIST["still_thr"], HIST["norm"],
                                         b["masks"])
    assert sums.shape[1:3] == (1, 2)
    return _frozen(dict(out=vals, sums=sums))


PROJECT = dict(t=0.5, scale=-0.5, min_weight=0.25)


@functools.lru_cache(maxsize=None)
def flow_project():
    b = base()
    out, hole, cov = flow_project_ref.project(b["flows"], PROJECT["t"], PROJECT["scale"], b["imp"], b["masks"], PROJECT["min_weight"])
    return _frozen(dict(out=out, hole=hole, cov=cov))


SPLAT = dict(t=0.5, min_weight=0.25)


@functools.lru_cache(maxsize=None)
def splat():
    """3-channel interleaved 8-bit sources, float32 out: the source is offset in bytes, the output in floats."""
    b = base()
    out, hole, cov = splat_ref.splat(b["bgr"], b["flows"], SPLAT["t"], b["imp"], b["masks"], "mean", "zero", SPLAT["min_weight"], F32)
    return _frozen(dict(out=out, hole=hole, cov=cov))


INTERP = dict(t=0.5, fill_passes=1, ksize=3, min_weight=0.25)


@functools.lru_cache(maxsize=None)
def interpolate():
    b = base()
    o, source = interpolate_ref.interpolate_batch(b["bgr"], b["bgr1"], b["flows"], b["back"], b["masks"], b["masks_b"], **INTERP)
    return _frozen(dict(out=interpolate_ref.stored(o, "uint8"), source=source))


U8_BOUNDS = (-1.5, 1.5)


def hwc_flows(scale=1.0):
    """The base flows, times scale, as the bounding calls take them: dense (H, W, 2)."""
    return np.ascontiguousarray((base()["flows"] * F32(scale)).transpose(0, 2, 3, 1))


@functools.lru_cache(maxsize=None)
def flow_to_u8():
    from oracle import oracle_py

    oracle_py.build()
    res = [oracle_py.flow_to_u8(f, *U8_BOUNDS) for f in hwc_flows()]
    return _frozen(dict(x=np.stack([r[0] for r in res]), y=np.stack([r[1] for r in res])))


PNG_SCALE = 2.0  # some of the flows beyond 127 / 128 of 4 pixels: the two bounds a 5 x 3 frame can have both occur


@functools.lru_cache(maxsize=None)
def flow_to_png():
    from oracle import oracle_py

    oracle_py.build()
    res = [oracle_py.flow_to_png_planes(f) for f in hwc_flows(PNG_SCALE)]
    return _frozen(dict(x=np.stack([r[0] for r in res]), y=np.stack([r[1] for r in res]),
                        bounds=np.array([r[2] for r in res], np.float64)))


@functools.lru_cache(maxsize=None)
def prepare():
    """The 4 x 2 B, G, R sources as 5 x 3 gray frames, and resized as they are (every channel on its own)."""
    from oracle import oracle_py

    oracle_py.build()
    src = base()["source"]
    gray = np.stack([oracle_py.prepare_frame(s, W, H) for s in src])
    bgr = np.stack([np.stack([oracle_py.prepare_frame(np.ascontiguousarray(s[..., c]), W, H) for c in range(3)], -1) for s in src])
    return _frozen(dict(gray=gray, bgr=bgr))


REFERENCES = dict(fb_check=fb_check, warp=warp, flow_chain=flow_chain, flow_median=flow_median, global_motion=global_motion,
                  flow_colour=flow_colour, flow_hist=flow_hist, flow_project=flow_project, splat=splat, interpolate=interpolate,
                  flow_to_u8=flow_to_u8, flow_to_png=flow_to_png, prepare=prepare)


def period(op):
    """Item i of a batch is base item i % period(op).  7, but 6 (base items 0 .. 5) where the launches hold 32767 items:
    32767 = 7 x 31 x 151, and with a period of 7 every launch would begin on base item 0, so that a launch that starts over at
    the front of the batch would go unseen.  65535 % 7 = 1 and 32767 % 6 = 1: the phase moves on by one at every boundary."""
    return 6 if op == "interpolate" else K


def chunk(op):
    """The most items a launch of the op takes."""
    return GRID_MAX // 2 if op == "interpolate" else GRID_MAX


def no_shift_maps_onto_itself(name, ref):
    """The K items, repeated, look different after a shift by 1 .. K - 1 items (K is prime: it is enough that two differ)."""
    b = bits(ref).reshape(len(ref), -1)
    assert len(b) == K and not [s for s in range(1, K) if np.array_equal(np.roll(b, s, 0), b)], (name, "a shift goes unseen")


def check_distinct(op):
    """Every compared output of an op: its K (flow_colour: K + 1) reference items pairwise different.  The one exception is
    arithmetic: a 5 x 3 frame has the two pairs of PNG bounds (4, 4) and (12, 4) and no other (the bound is a multiple of 4 of
    at most 128 / 127 of the frame's extent, and a multiple of 8 moves on by 4).  Both occur, no shift of the batch by 1 .. 6
    items gives the same bounds, and the planes, which the bounds scale, are pairwise different as everywhere."""
    ref = REFERENCES[op]()
    for name, a in ref.items():
        if op == "flow_colour" and name.endswith("_max2"):
            a = a[:K + 1]  # the per-flow words; the last word is the batch maximum, the last flow's own
        if (op, name) == ("flow_to_png", "bounds"):
            assert {tuple(x) for x in a} == {(4.0, 4.0), (12.0, 4.0)}
            no_shift_maps_onto_itself((op, name), a)
        else:
            distinct((op, name), a)
    return ref
