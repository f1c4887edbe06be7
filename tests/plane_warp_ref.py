"""NumPy reference of dfx_warp_planes_device (include/dfx.h, section (0.5.4)): the backward warp of float32 / float16 /
bfloat16 planes, and of opaque 1-, 2- or 4-byte elements, by a flow.  The header's text, in float32 with every operation
rounded on its own:

    px = (float)x + fu;  py = (float)y + fv
    inside = px >= 0 && py >= 0 && px <= W-1 && py <= H-1
    DFX_WARP_BORDER_ZERO : take = inside
    DFX_WARP_BORDER_CLAMP: take = px and py both not NaN;  px = min(max(px, 0), W-1), py likewise (infinities clamp)
    valid(x, y) = inside && (d_occ == NULL || occ[y][x] == 0)
    bilinear, where take:
        x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
        every tap P is converted exactly to float32
        per channel: t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s = t + ay*(b - t)
        stored as float32, or converted once as the typed planes convert (tests/reduced_ref.py)
    nearest, where take:
        xn = (int)rintf(px), yn = (int)rintf(py); the element P[yn][xn] is copied as a bit pattern
    DFX_WARP_INVALID_ZERO: every pixel is written; a pixel without take gets all-zero bits in every channel
    DFX_WARP_INVALID_KEEP: a pixel is written only where valid

warp() is the vectorised form, warp_loop() the same pixel by pixel in NumPy scalars; tests/test_plane_warp_ref.py holds the
two equal.  Arrays are channels-last inside ((H, W, C)); to_hwc / from_hwc move a (C, H, W) source there and back.  A half
type travels as uint16 bit patterns; "bfloat16" has no NumPy type of its own."""
import numpy as np

from tests import reduced_ref

F32 = np.float32
BORDERS = ("zero", "clamp")
SAMPLES = ("bilinear", "nearest")
FLOATS = ("float32", "float16", "bfloat16")
BYTES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}  # what DFX_PLANAR_F32 / _F16 / _BF16 / DFX_WARP_U8 name


def to_f32(a, dtype):
    """The exact float32 value of every element of a source of that dtype (float32 array, or uint16 bits of a half type)."""
    if dtype == "float32":
        return np.asarray(a, F32)
    bits = np.asarray(a).view(np.uint16)
    if dtype == "float16":
        return bits.view(np.float16).astype(F32)  # exact: subnormals kept
    assert dtype == "bfloat16"
    return reduced_ref.bf16_bits_to_f32(bits)


def stored(s, dtype):
    """What the device stores for the float32 samples s: float32 itself, or the uint16 bits of float16 / bfloat16."""
    if dtype == "float32":
        return np.asarray(s, F32)
    return reduced_ref.reduce_bits(s, dtype).reshape(np.shape(s))


def take_of(px, py, W, H, border):
    """(inside, take, px, py) of float32 positions in a W x H image; px, py clamped under "clamp" and (0, 0) where not take."""
    assert border in BORDERS
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    inside = (px >= F32(0)) & (py >= F32(0)) & (px <= F32(W - 1)) & (py <= F32(H - 1))
    if border == "zero":
        take = inside
        pxs, pys = np.where(take, px, F32(0)), np.where(take, py, F32(0))
    else:
        take = ~(np.isnan(px) | np.isnan(py))
        pxs = np.minimum(np.maximum(np.where(take, px, F32(0)), F32(0)), F32(W - 1))
        pys = np.minimum(np.maximum(np.where(take, py, F32(0)), F32(0)), F32(H - 1))
    return inside, take, pxs.astype(F32), pys.astype(F32)


def position(flow, border):
    """take_of the positions flow (2, H, W) names: px = (float)x + fu, py = (float)y + fv."""
    flow = np.asarray(flow, F32)
    _, H, W = flow.shape
    with np.errstate(invalid="ignore", over="ignore"):  # a flow of random bits may be a signalling NaN or overflow the sum
        px = np.arange(W, dtype=F32)[None, :] + flow[0]
        py = np.arange(H, dtype=F32)[:, None] + flow[1]
    return take_of(px, py, W, H, border)


def valid_of(flow, occ=None):
    inside = position(flow, "zero")[0]
    return (inside if occ is None else inside & (np.asarray(occ) == 0)).astype(np.uint8)


def bilinear_at(P, px, py):
    """The float32 samples (..., C) of the float32 planes P (H, W, C) at positions take_of has prepared."""
    P = np.asarray(P, F32)
    H, W, _ = P.shape
    fx, fy = np.floor(px), np.floor(py)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = (px - fx)[..., None], (py - fy)[..., None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = P[y0, x0] + ax * (P[y0, x1] - P[y0, x0])
        b = P[y1, x0] + ax * (P[y1, x1] - P[y1, x0])
        s = t + ay * (b - t)
    assert s.dtype == F32
    return s


def bilinear(P, flow, border):
    """(s, take): the float32 samples (H, W, C) of the float32 planes P (H, W, C), unmasked, and take (H, W)."""
    _, take, px, py = position(flow, border)
    return bilinear_at(P, px, py), take


def nearest_at(px, py):
    """(xn, yn) of positions take_of has prepared: rintf, ties to even."""
    return np.rint(px).astype(np.int64), np.rint(py).astype(np.int64)


def nearest(P, flow, border):
    """(e, take): the elements (H, W, C) of P (H, W, C; any dtype) at the rounded positions, and take (H, W)."""
    P = np.asarray(P)
    _, take, px, py = position(flow, border)
    xn, yn = nearest_at(px, py)
    return P[yn, xn], take


def warp(src, flow, sample="bilinear", border="zero", invalid="zero", src_dtype="float32", out_dtype=None, occ=None, out=None):
    """(stored, valid) for one source (H, W, C): `stored` has the source's shape — float32, the uint16 bits of a half type,
    or, for nearest, the source's own dtype — and valid is (H, W) uint8.  invalid="keep" writes into a copy of `out`."""
    assert sample in SAMPLES and invalid in ("zero", "keep")
    valid = valid_of(flow, occ)
    if sample == "bilinear":
        out_dtype = out_dtype or src_dtype
        assert src_dtype in FLOATS and out_dtype in FLOATS
        s, take = bilinear(to_f32(src, src_dtype), flow, border)
        new = stored(s, out_dtype)
    else:
        assert out_dtype in (None, src_dtype)
        new, take = nearest(src, flow, border)
    if invalid == "zero":
        res = np.where(take[..., None], new, np.zeros((), new.dtype))
    else:
        assert out is not None and out.shape == new.shape and out.dtype == new.dtype
        res = np.where((valid != 0)[..., None], new, out)
    return res.astype(new.dtype), valid


def warp_loop(src, flow, sample="bilinear", border="zero", invalid="zero", src_dtype="float32", out_dtype=None, occ=None, out=None):
    """The same, pixel by pixel in NumPy float32 scalars."""
    flow = np.asarray(flow, F32)
    _, H, W = flow.shape
    src = np.asarray(src)
    C = src.shape[2]
    if sample == "bilinear":
        out_dtype = out_dtype or src_dtype
        P = to_f32(src, src_dtype)
        res = np.zeros((H, W, C), F32 if out_dtype == "float32" else np.uint16)
    else:
        P = src
        res = np.zeros((H, W, C), src.dtype)
    if invalid == "keep":
        res = out.copy()
    valid = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            px, py = F32(x) + flow[0, y, x], F32(y) + flow[1, y, x]
            inside = bool(px >= F32(0) and py >= F32(0) and px <= F32(W - 1) and py <= F32(H - 1))
            valid[y, x] = 1 if inside and (occ is None or occ[y][x] == 0) else 0
            take = inside
            if border == "clamp":
                take = not (np.isnan(px) or np.isnan(py))
                if take:
                    px, py = min(max(px, F32(0)), F32(W - 1)), min(max(py, F32(0)), F32(H - 1))
            if invalid == "keep" and not valid[y, x]:
                continue
            if not take:
                res[y, x] = 0
                continue
            if sample == "nearest":
                res[y, x] = P[int(np.rint(py)), int(np.rint(px))]
                continue
            fx, fy = np.floor(px), np.floor(py)
            x0, y0 = int(fx), int(fy)
            ax, ay = F32(px - fx), F32(py - fy)
            x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
            for c in range(C):
                p00, p01, p10, p11 = P[y0, x0, c], P[y0, x1, c], P[y1, x0, c], P[y1, x1, c]
                with np.errstate(invalid="ignore", over="ignore"):
                    t = F32(p00 + F32(ax * F32(p01 - p00)))
                    b = F32(p10 + F32(ax * F32(p11 - p10)))
                    s = F32(t + F32(ay * F32(b - t)))
                res[y, x, c] = s if out_dtype == "float32" else stored(np.array([s], F32), out_dtype)[0]
    return res, valid


def to_hwc(a, layout):
    """One source as the reference takes it: (C, H, W) for "chw", (H, W, C) for "hwc"."""
    a = np.asarray(a)
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)) if layout == "chw" else a


def from_hwc(a, layout):
    return np.ascontiguousarray(np.moveaxis(a, -1, 0)) if layout == "chw" else a


def warp_batch(src, flows, layout="chw", occ=None, out=None, **kw):
    """warp over n sources (n, C, H, W) or (n, H, W, C) and flows (n, 2, H, W): (stored (n, ...) in the sources' layout,
    valid (n, H, W))."""
    res = [warp(to_hwc(src[i], layout), flows[i], occ=None if occ is None else occ[i],
                out=None if out is None else to_hwc(out[i], layout), **kw) for i in range(len(src))]
    return np.stack([from_hwc(r[0], layout) for r in res]), np.stack([r[1] for r in res])


def same(a, b, dtype):
    """Whether two stored results agree: bit for bit, except that two NaNs of a float type agree whatever their bits.
    dtype: "float32" / "float16" / "bfloat16" for bilinear results, None for nearest ones (every byte compared)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if dtype is None:
        return bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))
    if dtype == "float32":
        ua, ub = a.view(np.uint32), b.view(np.uint32)  # float32 values, or the uint32 that holds their bits
        return bool(np.all((ua == ub) | (np.isnan(ua.view(F32)) & np.isnan(ub.view(F32)))))
    na, nb = reduced_ref.is_nan_bits(a, dtype), reduced_ref.is_nan_bits(b, dtype)
    return bool(np.all((a == b) | (na & nb)))
