"""NumPy reference of the forward warp (splat) of images and float payloads along a flow (include/dfx.h, dfx_splat_device; the
kernels are denseflow_amd/csrc/splat_kernels.hip).  All float operations are float32, each rounded on its own, with no fused
multiply-add.  The skip rules, the landing test, the importance, the tap geometry and the weights are those of
dfx_flow_project_device (tests/flow_project_ref.py), word for word.  For source pixel (x, y) of source i with flow (fu, fv)
and payload v_c, c = 0 .. channels-1:

    skip the pixel if d_occ != NULL and occ[y][x] != 0
    px = (float)x + t*fu;   py = (float)y + t*fv
    skip unless px > -1 && px < W && py > -1 && py < H     (false for NaN; tested before any conversion to int)
    iq = 256                                                 without d_importance
         imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)
         (iq = 0 contributes nothing)
    x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)      0 .. 256;   y0, by likewise
    payload, DFX_WARP_U8 source:    q_c = the byte
    payload, DFX_PLANAR_F32 source: skip the pixel unless every channel has fabsf(v_c) <= 32768.f (false for NaN)
                                    q_c = (int)rintf(v_c * 256.f)
    taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with column weights {256 - bx, bx} and row weights {256 - by, by};
    a tap outside [0, W) x [0, H) is dropped;  wt = wx * wy * iq   (uint64; the four wx*wy add up to 65536 exactly)
    Wsum[tap] += wt (uint64);   S_c[tap] += wt * q_c   (int64; two's-complement wrap on both sides)

Per target pixel, after all source pixels of source i:

    Wmin = max(1, (uint64)llrint((double)min_weight * 16777216.0))       2^24 = full coverage at importance 1
    hole = Wsum < Wmin
    DFX_SPLAT_MEAN: r_c = (double)S_c / (double)Wsum
    DFX_SPLAT_SUM:  r_c = (double)S_c / 16777216.0
    a DFX_PLANAR_F32 source: r_c = r_c * (1.0 / 256.0)                   (in double)
    out_dtype DFX_PLANAR_F32: out_c = (float)r_c;   DFX_WARP_U8: out_c = (uint8_t)llrint(r_c)
    in a hole: DFX_SPLAT_HOLE_ZERO writes +0.0f / byte 0;  DFX_SPLAT_HOLE_KEEP does not write the pixel of d_out
    hole plane (uint8, optional): 0 / 1
    coverage plane (float32, optional): (float)((double)Wsum / 16777216.0)

splat is the vectorised form (np.add.at on int64), splat_loop a plain scalar loop of the same text over Python integers
(tests/test_splat_ref.py holds them against each other); the loop may visit the source pixels in any `order`.  Wsum is
accumulated as int64 bits and read as uint64."""
import numpy as np

from tests.flow_project_ref import FULL, project_inputs, same_bits, wmin_of  # noqa: F401  (same_bits: re-exported)

F32, F64, I64, U64, U8 = np.float32, np.float64, np.int64, np.uint64, np.uint8
PAYLOAD_MAX = F32(32768)


def payload(v):
    """The payload rule of a float32 source (C, H, W): (q int64 (C, H, W), ok bool (H, W)); a pixel that is not ok is skipped."""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        ok = (np.abs(v) <= PAYLOAD_MAX).all(axis=0)  # False for NaN
        q = np.rint(np.where(ok[None], v, F32(0)) * F32(256)).astype(I64)
    return q, ok


def sums(q, ok, flow, t, importance=None, occ=None):
    """(Wsum uint64 (H, W), S int64 (C, H, W)) of one source's integer payload q (C, H, W): the vectorised scatter."""
    C, H, W = q.shape
    t = F32(t)
    fu, fv = flow[0].astype(F32, copy=False), flow[1].astype(F32, copy=False)
    with np.errstate(all="ignore"):
        px = np.arange(W, dtype=F32)[None, :] + t * fu
        py = np.arange(H, dtype=F32)[:, None] + t * fv
        live = (px > F32(-1)) & (px < F32(W)) & (py > F32(-1)) & (py < F32(H)) & ok
        if occ is not None:
            live &= occ == 0
        iq = np.full((H, W), 256, I64)
        if importance is not None:
            imp = importance.astype(F32, copy=False)
            live &= imp > F32(0)
            iq = np.where(live, np.rint(np.minimum(np.where(live, imp, F32(1)), F32(256)) * F32(256)), 0).astype(I64)
        pxs, pys = np.where(live, px, F32(0)), np.where(live, py, F32(0))
        fx, fy = np.floor(pxs), np.floor(pys)
        bx = np.rint((pxs - fx) * F32(256)).astype(I64)
        by = np.rint((pys - fy) * F32(256)).astype(I64)
        x0, y0 = fx.astype(I64), fy.astype(I64)
    ws, s = np.zeros(H * W, I64), np.zeros((C, H * W), I64)
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = x0 + i, y0 + j
            wx = bx if i else 256 - bx
            wy = by if j else 256 - by
            hit = live & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            wt = (wx * wy * iq)[hit]
            at = (ty * W + tx)[hit]
            with np.errstate(over="ignore"):
                np.add.at(ws, at, wt)
                for c in range(C):
                    np.add.at(s[c], at, wt * q[c][hit])
    return ws.view(U64).reshape(H, W), s.reshape(C, H, W)


def sums_loop(q, ok, flow, t, importance=None, occ=None, order=None):
    """sums as a plain scalar loop over the source pixels, visited in `order` (a sequence of y * W + x; row-major without
    one); Python integers reduced modulo 2^64 at the end."""
    C, H, W = q.shape
    t = F32(t)
    ws = [0] * (H * W)
    s = [[0] * (H * W) for _ in range(C)]
    with np.errstate(all="ignore"):
        for k in (range(H * W) if order is None else order):
            y, x = divmod(int(k), W)
            if occ is not None and occ[y, x] != 0:
                continue
            if not ok[y, x]:
                continue
            fu, fv = F32(flow[0, y, x]), F32(flow[1, y, x])
            px = F32(x) + F32(t * fu)
            py = F32(y) + F32(t * fv)
            if not (px > F32(-1) and px < F32(W) and py > F32(-1) and py < F32(H)):
                continue
            iq = 256
            if importance is not None:
                imp = F32(importance[y, x])
                if not imp > F32(0):
                    continue
                iq = int(np.rint(F32(min(imp, F32(256))) * F32(256)))
            fx, fy = np.floor(px), np.floor(py)
            bx = int(np.rint(F32(F32(px - fx) * F32(256))))
            by = int(np.rint(F32(F32(py - fy) * F32(256))))
            x0, y0 = int(fx), int(fy)
            for j in (0, 1):
                for i in (0, 1):
                    tx, ty = x0 + i, y0 + j
                    if tx < 0 or tx >= W or ty < 0 or ty >= H:
                        continue
                    wt = (bx if i else 256 - bx) * (by if j else 256 - by) * iq
                    ws[ty * W + tx] += wt
                    for c in range(C):
                        s[c][ty * W + tx] += wt * int(q[c, y, x])
    m = (1 << 64) - 1
    as_u64 = lambda vals: np.array([v & m for v in vals], dtype=U64)
    return as_u64(ws).reshape(H, W), np.stack([as_u64(r).view(I64) for r in s]).reshape(C, H, W)


def normalise(ws, s, f32_source, mode="mean", min_weight=0.25, out_u8=False):
    """(r (C, H, W) float32 or uint8 with 0 in the holes, hole (H, W) uint8, coverage (H, W) float32) of one source's sums."""
    assert mode in ("mean", "sum") and not (out_u8 and (f32_source or mode != "mean"))
    hole = ws < U64(wmin_of(min_weight))
    d = ws.astype(F64)
    with np.errstate(all="ignore"):
        r = s.astype(F64) / d[None] if mode == "mean" else s.astype(F64) / FULL
        if f32_source:
            r = r * (1.0 / 256.0)
        r = np.where(hole[None], 0.0, r)
        out = np.rint(r).astype(U8) if out_u8 else r.astype(F32)
    return out, hole.astype(U8), (d / FULL).astype(F32)


def channels_first(images, layout="hwc", as_u8=None):
    """(the (n, C, H, W) view of images given as the binding takes them, whether they are 8-bit).  as_u8: the array has the
    shape of 8-bit images whatever its dtype (the float32 output of an 8-bit source)."""
    a = np.asarray(images)
    u8 = a.dtype == U8 if as_u8 is None else as_u8
    if not u8:
        assert a.dtype == F32 and a.ndim == 4 and 1 <= a.shape[1] <= 4
        return a, False
    if a.ndim == 3:
        return a[:, None], True
    return (a if layout == "chw" else a.transpose(0, 3, 1, 2)), True


def splat(images, flows, t=1.0, importance=None, occ=None, mode="mean", holes="zero", min_weight=0.25, dtype=None, layout="hwc",
          out=None, loop=False, order=None):
    """(out in the images' shape, hole (n, H, W) uint8, coverage (n, H, W) float32).  images: uint8 (n, H, W), (n, H, W, 3)
    or — layout "chw" — (n, 3, H, W), or float32 (n, C, H, W); flows (n, 2, H, W).  dtype None: uint8 for uint8 images in
    "mean", float32 otherwise.  holes "keep": out is required, is copied, and keeps its values in the holes."""
    assert holes in ("zero", "keep")
    flows = np.asarray(flows, F32)
    img, u8 = channels_first(images, layout)
    n, C, H, W = img.shape
    if dtype is None:
        dtype = U8 if u8 and mode == "mean" else F32
    out_u8 = np.dtype(dtype) == U8
    res = np.zeros((n, C, H, W), U8 if out_u8 else F32) if holes == "zero" else channels_first(out, layout, u8)[0].copy()
    assert res.dtype == (U8 if out_u8 else F32) and res.shape == img.shape
    hole, cov = np.empty((n, H, W), U8), np.empty((n, H, W), F32)
    for i in range(n):
        q, ok = (img[i].astype(I64), np.ones((H, W), bool)) if u8 else payload(img[i])
        imp_i, occ_i = None if importance is None else importance[i], None if occ is None else occ[i]
        ws, s = sums_loop(q, ok, flows[i], t, imp_i, occ_i, order) if loop else sums(q, ok, flows[i], t, imp_i, occ_i)
        r, hole[i], cov[i] = normalise(ws, s, not u8, mode, min_weight, out_u8)
        res[i] = np.where(hole[i][None] != 0, res[i], r) if holes == "keep" else r
    a = np.asarray(images)
    if u8 and a.ndim == 3:
        res = res[:, 0]
    elif u8 and layout != "chw":
        res = res.transpose(0, 2, 3, 1)
    return np.ascontiguousarray(res), hole, cov


def splat_loop(images, flows, **kw):
    return splat(images, flows, loop=True, **kw)


def splat_inputs(w, h, n=3, seed=530):
    """(gray (n, h, w) uint8, bgr (n, h, w, 3) uint8, payload (n, 4, h, w) float32, flows (n, 2, h, w), importance (n, h, w),
    occ (n, h, w)) of the GPU tests: textured images, a payload of mixed magnitudes within +-16, and project_inputs' flows,
    importances and masks."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    flows, imp, occ = project_inputs(w, h, n, seed)
    yy, xx = np.mgrid[0:h, 0:w]
    bgr = np.stack([np.stack([128 + 90 * np.sin(xx / (3.0 + c) + i) * np.cos(yy / (2.0 + c)) for c in range(3)], -1) for i in range(n)])
    bgr = np.clip(bgr + rng.normal(0, 12, bgr.shape), 0, 255).astype(U8)
    gray = np.ascontiguousarray(bgr[..., 1])
    pay = (rng.standard_normal((n, 4, h, w)) * np.array([16, 1, 1 / 64.0, 4])[None, :, None, None]).astype(F32)
    pay = np.clip(pay, -16, 16).astype(F32)
    return gray, np.ascontiguousarray(bgr), pay, flows, imp, occ


# the payload values at the edges of the rule: (value, taken, q)
def payload_edges():
    big = PAYLOAD_MAX
    tiny = np.frombuffer(np.uint32(1).tobytes(), F32)[0]  # the smallest subnormal
    return [(big, True, 8388608), (-big, True, -8388608), (np.nextafter(big, F32(np.inf)), False, 0),
            (np.nextafter(-big, F32(-np.inf)), False, 0), (F32(np.nan), False, 0), (F32(np.inf), False, 0),
            (F32(-np.inf), False, 0), (F32(-0.0), True, 0), (tiny, True, 0), (-tiny, True, 0), (F32(1e-39), True, 0),
            (F32(0.001953125), True, 0), (F32(0.005859375), True, 2), (F32(1.0), True, 256), (F32(-2.5), True, -640)]
