"""NumPy reference of the backward warp of 8-bit images by a flow (include/dfx.h, dfx_warp_device; the kernel is
denseflow_amd/csrc/warp_kernels.hip).  Float32 throughout, one rounding per operation, no fused multiply-add:

    px = (float)x + fu;  py = (float)y + fv
    inside = px >= 0 and py >= 0 and px <= W-1 and py <= H-1             (false for NaN / inf; before any int conversion)
    "zero" : not inside -> every channel's sample is 0
    "clamp": px or py NaN -> sample 0; otherwise px = min(max(px, 0), W-1), py likewise (infinities clamp)
    x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
    per channel, P = float(byte): t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s = t + ay*(b - t)
    stored: s (float32), s rounded once to float16 / bfloat16 (tests/reduced_ref.py), or q = uint8(rint(s)) (ties to even)
    valid = inside (unclamped in either mode) and (no occlusion mask or occ == 0)
    statistics over the pixels with valid == 1: count += 1, sad += sum over channels |ref - q|

warp is the vectorised form, warp_loop a plain scalar loop of the same text (tests/test_warp_ref.py holds them against each
other).  Images are (H, W) or (H, W, C) uint8 arrays, flows (2, H, W) float32 with plane 0 = u, plane 1 = v.  Neither form
touches the floating-point error state: a position that is not sampled is replaced by 0 before floor() and the conversion to
int see it, so the whole of either runs under np.errstate(all="raise")."""
import numpy as np

from tests import reduced_ref
from tests.fb_check_ref import smooth_flow

F32 = np.float32
BORDERS = ("zero", "clamp")
DTYPES = ("uint8", "float32", "float16", "bfloat16")


def inside_of(flow):
    """Where the target of flow (2, H, W) stays in the frame: the `inside` test."""
    flow = np.asarray(flow, F32)
    _, H, W = flow.shape
    px = np.arange(W, dtype=F32)[None, :] + flow[0]
    py = np.arange(H, dtype=F32)[:, None] + flow[1]
    return (px >= F32(0)) & (py >= F32(0)) & (px <= F32(W - 1)) & (py <= F32(H - 1))


def warp(src, flow, border="zero", occ=None):
    """(s, valid): the float32 samples in the shape of src, and the (H, W) uint8 valid mask."""
    assert border in BORDERS
    src, flow = np.asarray(src, np.uint8), np.asarray(flow, F32)
    _, H, W = flow.shape
    P = src.reshape(H, W, -1).astype(F32)
    px = np.arange(W, dtype=F32)[None, :] + flow[0]
    py = np.arange(H, dtype=F32)[:, None] + flow[1]
    inside = (px >= F32(0)) & (py >= F32(0)) & (px <= F32(W - 1)) & (py <= F32(H - 1))
    if border == "zero":
        take = inside
        pxs, pys = np.where(take, px, F32(0)), np.where(take, py, F32(0))
    else:
        take = ~(np.isnan(px) | np.isnan(py))
        pxs = np.minimum(np.maximum(np.where(take, px, F32(0)), F32(0)), F32(W - 1))
        pys = np.minimum(np.maximum(np.where(take, py, F32(0)), F32(0)), F32(H - 1))
    fx, fy = np.floor(pxs), np.floor(pys)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    ax, ay = (pxs - fx)[..., None], (pys - fy)[..., None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    t = P[y0, x0] + ax * (P[y0, x1] - P[y0, x0])
    b = P[y1, x0] + ax * (P[y1, x1] - P[y1, x0])
    s = t + ay * (b - t)
    assert s.dtype == F32
    s = np.where(take[..., None], s, F32(0)).astype(F32)
    valid = inside if occ is None else inside & (np.asarray(occ) == 0)
    return s.reshape(src.shape), valid.astype(np.uint8)


def warp_loop(src, flow, border="zero", occ=None):
    """The same, pixel by pixel in NumPy float32 scalars."""
    assert border in BORDERS
    src, flow = np.asarray(src, np.uint8), np.asarray(flow, F32)
    _, H, W = flow.shape
    P = src.reshape(H, W, -1)
    C = P.shape[2]
    s = np.zeros((H, W, C), F32)
    valid = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            px, py = F32(x) + flow[0, y, x], F32(y) + flow[1, y, x]
            inside = bool(px >= F32(0) and py >= F32(0) and px <= F32(W - 1) and py <= F32(H - 1))
            valid[y, x] = 1 if inside and (occ is None or occ[y][x] == 0) else 0
            if border == "zero":
                if not inside:
                    continue
            else:
                if np.isnan(px) or np.isnan(py):
                    continue
                px, py = min(max(px, F32(0)), F32(W - 1)), min(max(py, F32(0)), F32(H - 1))
            fx, fy = np.floor(px), np.floor(py)
            x0, y0 = int(fx), int(fy)
            ax, ay = px - fx, py - fy
            x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
            for c in range(C):
                p00, p01, p10, p11 = F32(P[y0, x0, c]), F32(P[y0, x1, c]), F32(P[y1, x0, c]), F32(P[y1, x1, c])
                t = p00 + ax * (p01 - p00)
                b = p10 + ax * (p11 - p10)
                s[y, x, c] = t + ay * (b - t)
    return s.reshape(src.shape), valid


def quantise(s):
    """q = (uint8)rintf(s): round to nearest, ties to even."""
    return np.rint(np.asarray(s, F32)).astype(np.uint8)


def stored(s, dtype):
    """What the device stores for the samples s: uint8, float32, or the uint16 bit patterns of float16 / bfloat16."""
    if dtype == "uint8":
        return quantise(s)
    if dtype == "float32":
        return np.asarray(s, F32)
    return reduced_ref.reduce_bits(s, dtype).reshape(np.shape(s))


def stats(s, ref, valid):
    """(count, sad) over the pixels with valid == 1: Python ints."""
    H, W = valid.shape
    d = np.abs(quantise(s).reshape(H, W, -1).astype(np.int64) - np.asarray(ref, np.uint8).reshape(H, W, -1).astype(np.int64))
    return int(valid.sum()), int((d.sum(axis=2) * (valid != 0)).sum())


def warp_batch(src, flows, border="zero", occ=None, ref=None):
    """warp over n images (n, H, W[, C]) and flows (n, 2, H, W): (s (n, ...) float32, valid (n, H, W) uint8, stats (n, 2)
    uint64 or None without ref)."""
    src, flows = np.asarray(src, np.uint8), np.asarray(flows, F32)
    res = [warp(src[i], flows[i], border, None if occ is None else occ[i]) for i in range(len(src))]
    s = np.stack([r[0] for r in res]) if res else np.empty(src.shape, F32)
    valid = np.stack([r[1] for r in res]) if res else np.empty(flows.shape[:1] + flows.shape[2:], np.uint8)
    st = None
    if ref is not None:
        st = np.array([stats(s[i], ref[i], valid[i]) for i in range(len(src))], np.uint64).reshape(len(src), 2)
    return s, valid, st


def mean_abs_error(st, channels):
    """sad / (count * channels) per row of an (n, 2) statistics array, in float64 (NaN where count is 0)."""
    st = np.asarray(st)
    cnt, sad = st[:, 0].astype(np.float64), st[:, 1].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cnt > 0, sad / (cnt * channels), np.nan)


def warp_flow(rng, n, h, w):
    """n smooth random flows whose horizontal magnitude is up to about half the width and whose vertical one about half the
    height, so that a good share of the targets stays inside at any aspect ratio."""
    f = smooth_flow(rng, n, h, w, 1.0)
    f[:, 0] *= F32(0.5 * w)
    f[:, 1] *= F32(0.5 * h)
    return f


SPECIALS = ["nan_u", "nan_v", "+inf", "-inf", "1e30", "-1e30", "-0.0", "last_col", "last_col+", "last_row", "last_row+",
            "last_both", "last_both+"]


def plant_specials(flow):
    """Plants the special values at fixed pixels of flow (2, H, W), in place: special k goes to the pixel with row-major index
    7 * k + 3 (modulo W * H: tiny sizes hold only the last few).  Returns {name: (x, y)}.
      nan_u / nan_v: never reach a conversion; sample 0 in both modes, valid 0
      +-inf / +-1e30: never reach a conversion unclamped; "zero": 0, "clamp": the edge pixel; valid 0
      -0.0         : a flow of (-0.0, -0.0): inside, the pixel itself
      last_col     : px exactly W - 1 (inside, x1 clamps); last_row: py exactly H - 1; last_both: both
      ...+         : the same one ulp beyond (outside; "clamp" comes back to the last column / row)"""
    _, H, W = flow.shape
    where = {}
    for k, name in enumerate(SPECIALS):
        y, x = divmod((7 * k + 3) % (W * H), W)
        where[name] = (x, y)
        far_x = np.nextafter(F32(W - 1), F32(np.inf)) - F32(x)
        far_y = np.nextafter(F32(H - 1), F32(np.inf)) - F32(y)
        u, v = {"nan_u": (np.nan, 0.25), "nan_v": (0.25, np.nan), "+inf": (np.inf, 0.0), "-inf": (0.0, -np.inf),
                "1e30": (1e30, 0.0), "-1e30": (0.0, -1e30), "-0.0": (-0.0, -0.0), "last_col": (W - 1 - x, 0.0),
                "last_col+": (far_x, 0.0), "last_row": (0.0, H - 1 - y), "last_row+": (0.0, far_y),
                "last_both": (W - 1 - x, H - 1 - y), "last_both+": (far_x, far_y)}[name]
        flow[0, y, x], flow[1, y, x] = u, v
        if name.endswith("+"):  # the flows really land one ulp beyond the last column / row
            if "row" not in name:
                assert F32(x) + flow[0, y, x] == np.nextafter(F32(W - 1), F32(np.inf))
            if "col" not in name:
                assert F32(y) + flow[1, y, x] == np.nextafter(F32(H - 1), F32(np.inf))
    return where
