"""NumPy reference of the forward projection of flows (include/dfx.h, dfx_flow_project_device; the kernels are
denseflow_amd/csrc/flow_project_kernels.hip).  All float operations are float32, each rounded on its own, with no fused
multiply-add.  For source pixel (x, y) of flow i with flow (fu, fv):

    skip the pixel if d_occ != NULL and occ[y][x] != 0
    px = (float)x + t*fu;   py = (float)y + t*fv
    skip unless px > -1 && px < W && py > -1 && py < H     (false for NaN; tested before any conversion to int)
    iq = 256                                                 without d_importance
         imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)
         (iq = 0 contributes nothing)
    x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)      0 .. 256;   y0, by likewise
    qu = (int)rintf(fminf(fmaxf(fu * 256.f, -8388608.f), 8388608.f));   qv likewise
    taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with column weights {256 - bx, bx} and row weights {256 - by, by};
    a tap outside [0, W) x [0, H) is dropped;  wt = wx * wy * iq   (uint64; the four wx*wy add up to 65536 exactly)
    Wsum[tap] += wt (uint64);   Su[tap] += wt * qu;   Sv[tap] += wt * qv   (int64; two's-complement wrap on both sides)

Per target pixel q, after all sources of the flow:

    Wmin = max(1, (uint64)llrint((double)min_weight * 16777216.0))       2^24 = full coverage at importance 1
    hole = Wsum < Wmin
    out_u = hole ? +0.0f : (float)(((double)Su / (double)Wsum) * ((double)scale / 256.0));   out_v likewise
    hole plane (uint8, optional): 0 / 1
    coverage plane (float32, optional): (float)((double)Wsum / 16777216.0)

A product min_weight * 16777216.0 of 2^63 or more gives Wmin = 2^63.  project is the vectorised form (np.add.at on int64),
project_loop a plain scalar loop of the same text (tests/test_flow_project_ref.py holds them against each other).  The sums
are kept in int64 / uint64 arrays whose adds wrap as the device's do; Wsum is accumulated as int64 bits and read as uint64."""
import numpy as np

F32, F64, I64, U64, U32 = np.float32, np.float64, np.int64, np.uint64, np.uint32
FULL = 16777216.0  # 2^24: the weight of one source of importance 1


def wmin_of(min_weight):
    m = F64(F32(min_weight)) * FULL
    if m >= 9223372036854775808.0:
        return 1 << 63
    return max(1, int(np.rint(m)))


def sums(flow, t, importance=None, occ=None):
    """(Wsum uint64, Su int64, Sv int64), each (H, W), of one flow (2, H, W): the vectorised scatter."""
    _, H, W = flow.shape
    t = F32(t)
    fu, fv = flow[0].astype(F32, copy=False), flow[1].astype(F32, copy=False)
    with np.errstate(all="ignore"):
        px = np.arange(W, dtype=F32)[None, :] + t * fu
        py = np.arange(H, dtype=F32)[:, None] + t * fv
        live = (px > F32(-1)) & (px < F32(W)) & (py > F32(-1)) & (py < F32(H))
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
        fus, fvs = np.where(live, fu, F32(0)), np.where(live, fv, F32(0))
        qu = np.rint(np.minimum(np.maximum(fus * F32(256), F32(-8388608)), F32(8388608))).astype(I64)
        qv = np.rint(np.minimum(np.maximum(fvs * F32(256), F32(-8388608)), F32(8388608))).astype(I64)
    ws, su, sv = np.zeros(H * W, I64), np.zeros(H * W, I64), np.zeros(H * W, I64)
    for j in (0, 1):
        for i in (0, 1):
            tx, ty = x0 + i, y0 + j
            wx = bx if i else 256 - bx
            wy = by if j else 256 - by
            ok = live & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            wt = (wx * wy * iq)[ok]
            at = (ty * W + tx)[ok]
            with np.errstate(over="ignore"):
                np.add.at(ws, at, wt)
                np.add.at(su, at, wt * qu[ok])
                np.add.at(sv, at, wt * qv[ok])
    return ws.view(U64).reshape(H, W), su.reshape(H, W), sv.reshape(H, W)


def sums_loop(flow, t, importance=None, occ=None):
    """sums as a plain scalar loop over the source pixels; Python integers reduced modulo 2^64 at the end."""
    _, H, W = flow.shape
    t = F32(t)
    ws = [[0] * W for _ in range(H)]
    su = [[0] * W for _ in range(H)]
    sv = [[0] * W for _ in range(H)]
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                if occ is not None and occ[y, x] != 0:
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
                qu = int(np.rint(min(max(F32(fu * F32(256)), F32(-8388608)), F32(8388608))))
                qv = int(np.rint(min(max(F32(fv * F32(256)), F32(-8388608)), F32(8388608))))
                for j in (0, 1):
                    for i in (0, 1):
                        tx, ty = x0 + i, y0 + j
                        if tx < 0 or tx >= W or ty < 0 or ty >= H:
                            continue
                        wt = (bx if i else 256 - bx) * (by if j else 256 - by) * iq
                        ws[ty][tx] += wt
                        su[ty][tx] += wt * qu
                        sv[ty][tx] += wt * qv
    m = (1 << 64) - 1
    as_u64 = lambda rows: np.array([[v & m for v in r] for r in rows], dtype=U64).reshape(H, W)
    return as_u64(ws), as_u64(su).view(I64), as_u64(sv).view(I64)


def normalise(ws, su, sv, scale, min_weight):
    """(out (2, H, W) float32, hole (H, W) uint8, coverage (H, W) float32) of the sums of one flow."""
    hole = ws < U64(wmin_of(min_weight))
    d = ws.astype(F64)
    sc = F64(F32(scale)) / 256.0
    with np.errstate(all="ignore"):
        u = ((su.astype(F64) / d) * sc).astype(F32)
        v = ((sv.astype(F64) / d) * sc).astype(F32)
    out = np.stack([np.where(hole, F32(0), u), np.where(hole, F32(0), v)]).astype(F32)
    return out, hole.astype(np.uint8), (d / FULL).astype(F32)


def project(flows, t=1.0, scale=None, importance=None, occ=None, min_weight=0.25, loop=False):
    """(out (N, 2, H, W), hole (N, H, W), coverage (N, H, W)) of flows (N, 2, H, W); scale None is -t."""
    flows = np.asarray(flows, F32)
    n, _, H, W = flows.shape
    scale = -F32(t) if scale is None else scale
    out, hole, cov = np.empty((n, 2, H, W), F32), np.empty((n, H, W), np.uint8), np.empty((n, H, W), F32)
    f = sums_loop if loop else sums
    for i in range(n):
        s = f(flows[i], t, None if importance is None else importance[i], None if occ is None else occ[i])
        out[i], hole[i], cov[i] = normalise(*s, scale, min_weight)
    return out, hole, cov


def project_loop(flows, **kw):
    return project(flows, loop=True, **kw)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and bool(
        np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)))


def smooth_random_flow(rng, n, h, w, amp, cells=4):
    """n smooth random flows of amplitude about `amp` pixels: bilinear upsampling of a cells x cells grid of normals."""
    gy, gx = np.linspace(0, cells - 1, h), np.linspace(0, cells - 1, w)
    y0, x0 = np.minimum(gy.astype(int), cells - 2), np.minimum(gx.astype(int), cells - 2)
    ay, ax = (gy - y0)[:, None], (gx - x0)[None, :]
    g = rng.standard_normal((n, 2, cells, cells)) * amp
    def at(dy, dx):
        return g[:, :, (y0 + dy)[:, None], (x0 + dx)[None, :]]
    f = (at(0, 0) * (1 - ax) + at(0, 1) * ax) * (1 - ay) + (at(1, 0) * (1 - ax) + at(1, 1) * ax) * ay
    return f.astype(F32)


def project_inputs(w, h, n=3, seed=490):
    """(flows (n, 2, h, w), importance (n, h, w), occ (n, h, w)) of the GPU tests: smooth flows of a few pixels with noise of a
    fraction of a pixel, importances between 0.1 and 4, a tenth of the pixels masked."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    flows = smooth_random_flow(rng, n, h, w, max(1.0, 0.06 * max(w, h))) + (rng.standard_normal((n, 2, h, w)) * 0.2).astype(F32)
    imp = np.exp(rng.uniform(np.log(0.1), np.log(4.0), (n, h, w))).astype(F32)
    occ = (rng.random((n, h, w)) < 0.1).astype(np.uint8) * rng.integers(1, 256, (n, h, w)).astype(np.uint8)
    return flows.astype(F32), imp, occ
