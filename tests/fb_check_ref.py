"""NumPy reference of the forward-backward consistency check (include/dfx.h, dfx_fb_check_device; the kernel is
denseflow_amd/csrc/fb_check_kernels.hip).  Float32 throughout, one rounding per operation, no fused multiply-add:

    px = (float)x + fu;  py = (float)y + fv
    inside = px >= 0 and py >= 0 and px <= W-1 and py <= H-1            (false for NaN / inf; before any int conversion)
    outside: occ = 1, err = +inf
    inside : x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
             per plane P of B: t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s = t + ay*(b - t)
             du = fu + su, dv = fv + sv;  err = du*du + dv*dv
             mag = (fu*fu + fv*fv) + (su*su + sv*sv);  thr = alpha1*mag + alpha2;  occ = 0 if err <= thr else 1

fb_check is the vectorised form, fb_check_loop a plain scalar loop of the same text (tests/test_fb_check_ref.py holds them
against each other).  Flows are (2, H, W) float32 arrays, plane 0 = u, plane 1 = v."""
import numpy as np

F32 = np.float32
ALPHA1, ALPHA2 = 0.01, 0.5  # UnFlow's constants (restated from memory, rated MED)


def fb_check(fwd, bwd, alpha1=ALPHA1, alpha2=ALPHA2):
    """(occ uint8 (H, W), err float32 (H, W)) of flow fwd checked against flow bwd."""
    fwd, bwd = np.asarray(fwd, F32), np.asarray(bwd, F32)
    _, H, W = fwd.shape
    a1, a2 = F32(alpha1), F32(alpha2)
    fu, fv = fwd[0], fwd[1]
    with np.errstate(all="ignore"):
        px = np.arange(W, dtype=F32)[None, :] + fu
        py = np.arange(H, dtype=F32)[:, None] + fv
        inside = (px >= F32(0)) & (py >= F32(0)) & (px <= F32(W - 1)) & (py <= F32(H - 1))
        pxi, pyi = np.where(inside, px, F32(0)), np.where(inside, py, F32(0))
        fx, fy = np.floor(pxi), np.floor(pyi)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        ax, ay = pxi - fx, pyi - fy
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        s = []
        for P in (bwd[0], bwd[1]):
            t = P[y0, x0] + ax * (P[y0, x1] - P[y0, x0])
            b = P[y1, x0] + ax * (P[y1, x1] - P[y1, x0])
            s.append(t + ay * (b - t))
        su, sv = s
        du, dv = fu + su, fv + sv
        err = du * du + dv * dv
        mag = (fu * fu + fv * fv) + (su * su + sv * sv)
        thr = a1 * mag + a2
        occ = np.where(err <= thr, 0, 1)
    assert err.dtype == F32 and thr.dtype == F32
    err = np.where(inside, err, F32(np.inf)).astype(F32)
    occ = np.where(inside, occ, 1).astype(np.uint8)
    return occ, err


def fb_check_loop(fwd, bwd, alpha1=ALPHA1, alpha2=ALPHA2):
    """The same, pixel by pixel in NumPy float32 scalars."""
    fwd, bwd = np.asarray(fwd, F32), np.asarray(bwd, F32)
    _, H, W = fwd.shape
    a1, a2 = F32(alpha1), F32(alpha2)
    occ = np.ones((H, W), np.uint8)
    err = np.full((H, W), np.inf, F32)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                fu, fv = fwd[0, y, x], fwd[1, y, x]
                px, py = F32(x) + fu, F32(y) + fv
                if not (px >= F32(0) and py >= F32(0) and px <= F32(W - 1) and py <= F32(H - 1)):
                    continue
                x0, y0 = int(np.floor(px)), int(np.floor(py))
                ax, ay = px - F32(x0), py - F32(y0)
                x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                s = []
                for P in (bwd[0], bwd[1]):
                    t = P[y0, x0] + ax * (P[y0, x1] - P[y0, x0])
                    b = P[y1, x0] + ax * (P[y1, x1] - P[y1, x0])
                    s.append(t + ay * (b - t))
                su, sv = s
                du, dv = fu + su, fv + sv
                e = du * du + dv * dv
                mag = (fu * fu + fv * fv) + (su * su + sv * sv)
                thr = a1 * mag + a2
                err[y, x] = e
                occ[y, x] = 0 if e <= thr else 1
    return occ, err


def fb_check_batch(fwd, bwd, alpha1=ALPHA1, alpha2=ALPHA2):
    """fb_check over (n, 2, H, W) arrays: (occ (n, H, W) uint8, err (n, H, W) float32)."""
    res = [fb_check(f, b, alpha1, alpha2) for f, b in zip(fwd, bwd)]
    shape = np.asarray(fwd).shape
    if not res:
        return np.empty((0,) + shape[2:], np.uint8), np.empty((0,) + shape[2:], F32)
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def out_of_frame(fwd):
    """Where flow fwd (2, H, W) leaves the frame (the `inside` test, negated)."""
    fwd = np.asarray(fwd, F32)
    _, H, W = fwd.shape
    with np.errstate(all="ignore"):
        px = np.arange(W, dtype=F32)[None, :] + fwd[0]
        py = np.arange(H, dtype=F32)[:, None] + fwd[1]
        return ~((px >= F32(0)) & (py >= F32(0)) & (px <= F32(W - 1)) & (py <= F32(H - 1)))


def smooth_flow(rng, n, h, w, mag):
    """n smooth random (2, H, W) float32 flow fields of magnitude up to about `mag`: a bilinear blow-up of a coarse random
    grid, so that neighbouring pixels land on neighbouring taps and a large share leaves the frame."""
    gh, gw = max(h // 16, 1) + 1, max(w // 16, 1) + 1
    grid = rng.uniform(-mag, mag, (n, 2, gh, gw))
    ys, xs = np.linspace(0, gh - 1, h), np.linspace(0, gw - 1, w)
    y0, x0 = np.minimum(ys.astype(int), gh - 2), np.minimum(xs.astype(int), gw - 2)
    ay, ax = (ys - y0)[:, None], (xs - x0)[None, :]
    g = lambda dy, dx: grid[:, :, y0 + dy][:, :, :, x0 + dx]  # noqa: E731
    out = (g(0, 0) * (1 - ax) + g(0, 1) * ax) * (1 - ay) + (g(1, 0) * (1 - ax) + g(1, 1) * ax) * ay
    return out.astype(F32)


SPECIALS = ["nan_u", "nan_v", "+inf", "-inf", "1e30", "-1e30", "-0.0", "last_col", "last_row", "last_both", "nan_b"]


def plant_specials(fwd, bwd):
    """Plants the special values at fixed pixels of flow pair (fwd, bwd), both (2, H, W), in place: special k goes to the
    pixel with row-major index 7 * k + 3 (modulo W * H: tiny sizes hold only the last few).  Returns {name: (x, y)}.
      nan_u / nan_v / +-inf / +-1e30: never reach a conversion, occ = 1, err = +inf
      -0.0        : a flow of (-0.0, -0.0): inside
      last_col    : px exactly W - 1 (inside, x1 clamps); last_row: py exactly H - 1; last_both: both
      nan_b       : a zero forward flow onto a NaN in bwd: inside, err NaN, occ = 1"""
    _, H, W = fwd.shape
    where = {}
    for k, name in enumerate(SPECIALS):
        y, x = divmod((7 * k + 3) % (W * H), W)
        where[name] = (x, y)
        u, v = {"nan_u": (np.nan, 0.25), "nan_v": (0.25, np.nan), "+inf": (np.inf, 0.0), "-inf": (0.0, -np.inf),
                "1e30": (1e30, 0.0), "-1e30": (0.0, -1e30), "-0.0": (-0.0, -0.0), "last_col": (W - 1 - x, 0.0),
                "last_row": (0.0, H - 1 - y), "last_both": (W - 1 - x, H - 1 - y), "nan_b": (0.0, 0.0)}[name]
        fwd[0, y, x], fwd[1, y, x] = u, v
        if name == "nan_b":
            bwd[0, y, x] = np.nan
    return where
