"""The arithmetic of dfx_global_motion_device (include/dfx.h, denseflow_amd/csrc/global_motion_kernels.hip) restated in
NumPy: a robust parametric fit of the dominant (camera) motion of a flow, the flow with that motion removed, and the mask of
the pixels that do not follow it.  The sums are integers (exact, independent of the order), the solve is float64 with every
operation on its own, the per-pixel arithmetic float32 with every operation on its own: the device agrees with this file bit
for bit."""
import numpy as np

F32 = np.float32
TRANSLATION, AFFINE = 0, 1
MODELS = {"translation": TRANSLATION, "affine": AFFINE}
SUM_NAMES = ("S1", "Sx", "Sy", "Sxx", "Sxy", "Syy", "Su", "Sxu", "Syu", "Sv", "Sxv", "Syv")
MAX_ROUNDS = 8
LIMIT = F32(4096.0)  # |u|, |v| below this: |q| <= 2^20


def coords(w, h):
    """Doubled, centred integer coordinates: xc (1, W), yc (H, 1) as int64."""
    xc = 2 * np.arange(w, dtype=np.int64)[None, :] - (w - 1)
    yc = 2 * np.arange(h, dtype=np.int64)[:, None] - (h - 1)
    return xc, yc


def ok_of(flow, mask=None):
    """(H, W) bool: |u| < 4096 and |v| < 4096 (false for NaN and either infinity) and, with a mask, mask == 0."""
    u, v = flow[0], flow[1]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(u) < LIMIT) & (np.abs(v) < LIMIT)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    return ok


def thresholds(thr, growth, rounds):
    """t_k, k = 0 .. rounds - 1: thr multiplied rounds - 1 - k times by growth, in float32."""
    out = []
    for k in range(rounds):
        t = F32(thr)
        with np.errstate(over="ignore"):
            for _ in range(rounds - 1 - k):
                t = F32(t * F32(growth))
        out.append(t)
    return out


def residual(flow, p):
    """(ru, rv): the flow minus the model p (float32[6], centred doubled coordinates), every operation on its own."""
    h, w = flow.shape[1:]
    xc, yc = coords(w, h)
    xf, yf = xc.astype(F32), yc.astype(F32)
    p = np.asarray(p, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        ru = flow[0] - ((p[0] + p[1] * xf) + p[2] * yf)
        rv = flow[1] - ((p[3] + p[4] * xf) + p[5] * yf)
    return ru.astype(F32), rv.astype(F32)


def within(flow, p, t):
    """(H, W) bool: ru*ru + rv*rv <= t*t in float32 (false for NaN)."""
    ru, rv = residual(flow, p)
    with np.errstate(invalid="ignore", over="ignore"):
        return (ru * ru + rv * rv) <= F32(t) * F32(t)


def sums_of(flow, inl):
    """The twelve int64 sums over the pixels of `inl`."""
    h, w = flow.shape[1:]
    xc, yc = coords(w, h)
    with np.errstate(invalid="ignore", over="ignore"):
        qu = np.where(inl, np.rint(np.where(inl, flow[0], 0) * F32(256.0)), 0).astype(np.int64)
        qv = np.where(inl, np.rint(np.where(inl, flow[1], 0) * F32(256.0)), 0).astype(np.int64)
    one = inl.astype(np.int64)
    X, Y = xc * one, yc * one
    return np.array([one.sum(), X.sum(), Y.sum(), (X * xc).sum(), (X * yc).sum(), (Y * yc).sum(),
                     qu.sum(), (xc * qu).sum(), (yc * qu).sum(), qv.sum(), (xc * qv).sum(), (yc * qv).sum()], np.int64)


def solve(sums, model):
    """(P float64[6] or None when the round is degenerate): the closed-form solve, in the header's order of operations."""
    S1, Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = (np.float64(int(s)) for s in sums)
    q = np.float64(256.0)
    if model == TRANSLATION:
        if S1 < 1:
            return None
        z = np.float64(0.0)
        return np.array([Su / S1 / q, z, z, Sv / S1 / q, z, z], np.float64)
    if S1 < 3:
        return None
    c00 = Sxx * Syy - Sxy * Sxy
    c01 = Sy * Sxy - Sx * Syy
    c02 = Sx * Sxy - Sy * Sxx
    c11 = S1 * Syy - Sy * Sy
    c12 = Sx * Sy - S1 * Sxy
    c22 = S1 * Sxx - Sx * Sx
    det = (S1 * c00 + Sx * c01) + Sy * c02
    if not det > 0:
        return None
    d = det * q
    P = []
    for A, B, Cc in ((Su, Sxu, Syu), (Sv, Sxv, Syv)):
        P += [((c00 * A + c01 * B) + c02 * Cc) / d, ((c01 * A + c11 * B) + c12 * Cc) / d, ((c02 * A + c12 * B) + c22 * Cc) / d]
    return np.array(P, np.float64)


def pixel_origin(P, w, h):
    """a[6]: the model in pixel coordinates, u_cam(x, y) = a0 + a1 x + a2 y, v_cam = a3 + a4 x + a5 y (float64)."""
    P = np.asarray(P, np.float64)
    wm, hm = np.float64(w - 1), np.float64(h - 1)
    a = []
    for o in (0, 3):
        a += [(P[o] - P[o + 1] * wm) - P[o + 2] * hm, np.float64(2.0) * P[o + 1], np.float64(2.0) * P[o + 2]]
    return np.array(a, np.float64)


def global_motion(flow, mask=None, model=AFFINE, rounds=5, thr=0.5, growth=2.0):
    """One flow (2, H, W) float32 -> dict(a, p, valid, inliers[8], status, rounds, sums, out (2, H, W), moving (H, W))."""
    flow = np.asarray(flow, F32)
    assert flow.ndim == 3 and flow.shape[0] == 2 and 1 <= rounds <= MAX_ROUNDS
    h, w = flow.shape[1:]
    ok = ok_of(flow, mask)
    ts = thresholds(thr, growth, rounds)
    P, p = np.zeros(6, np.float64), np.zeros(6, F32)
    inliers, status, sums = np.zeros(MAX_ROUNDS, np.uint64), 0, None
    for k in range(rounds):
        inl = ok if k == 0 else ok & within(flow, p, ts[k])
        sums = sums_of(flow, inl)
        inliers[k] = sums[0]
        new = solve(sums, model)
        if new is None:
            status |= 1 << k
        else:
            P = new
            with np.errstate(over="ignore"):
                p = P.astype(F32)
    ru, rv = residual(flow, p)
    moving = (~(ok & within(flow, p, F32(thr)))).astype(np.uint8)
    return dict(a=pixel_origin(P, w, h), p=p, P=P, valid=np.uint64(ok.sum()), inliers=inliers, status=status, rounds=rounds,
                sums=sums, out=np.stack([ru, rv]), moving=moving)


def camera_flow(a, w, h):
    """(2, H, W) float64: the model a (pixel origin) evaluated on the pixel grid."""
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    return np.stack([a[0] + a[1] * x + a[2] * y, a[3] + a[4] * x + a[5] * y])


def synth_case(w, h, seed, dt, fg=0.30, sigma=0.05):
    """(flow (2, H, W) float32, background (H, W) bool, true background flow (2, H, W) float64): SynthClip's exactly affine
    camera flow over dt frames, a rectangle of `fg` of the area at (W // 5, H // 4) moving by (-2.25, 1.25) * dt, Gaussian
    noise of sigma from default_rng(seed)."""
    from denseflow_amd.synth import SynthClip

    bg = SynthClip(w, h, seed).true_flow(0, dt).astype(np.float64).transpose(2, 0, 1)
    area = fg * w * h
    rw = min(int(np.sqrt(area * w / h)), w - w // 5)
    rh = min(int(area / rw), h - h // 4)
    back = np.ones((h, w), bool)
    back[h // 4:h // 4 + rh, w // 5:w // 5 + rw] = False
    flow = bg.copy()
    flow[0][~back], flow[1][~back] = -2.25 * dt, 1.25 * dt
    flow += np.random.default_rng(seed).normal(0.0, sigma, flow.shape)
    return flow.astype(F32), back, bg
