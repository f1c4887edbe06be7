"""NumPy reference of the colour coding of flows (include/dfx.h, dfx_flow_colour_device; the kernels are
denseflow_amd/csrc/flow_colour_kernels.hip): the Middlebury wheel of Baker et al. 2011, unknown pixels marked and left out
of the normalisation.  Float32 throughout, one rounding per operation, no fused multiply-add, IEEE / and sqrtf, subnormals
kept:

    wheel   : 55 RGB entries from the segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; read as W/255.0f
    known   = (mask == NULL || mask[y][x] == 0) && |u| <= 1e9f && |v| <= 1e9f          (false for NaN and both infinities)
    r2 = u*u + v*v;  M2_i = max of r2 over the known pixels of flow i (+0 if none);  MB2 = max_i M2_i
    R = max_rad (FIXED), sqrtf(M2_i) (FLOW), sqrtf(MB2) (BATCH)
    D = R + 0x1p-23f;  un = u / D;  vn = v / D;  rad = sqrtf(un*un + vn*vn)
    FLOW and BATCH: rad = fminf(rad, 1.0f)
    a = atan2_turns(-vn, -un):
        ax = |x|, ay = |y|, mx = max(ax, ay), mn = min(ax, ay)
        t = mx > 0 ? mn / mx : 0
        s = t*t
        p = c5;  p = p*s + c4;  ... ;  p = p*s + c0      (multiply, then add, each rounded)
        r = t*p
        if (ay > ax)    r = 1.5707964f - r
        if (signbit(x)) r = 3.1415927f - r
        if (signbit(y)) r = -r
        a = r * 0.31830987f
    fk = (a + 1.0f) * 27.0f
    fk = fminf(fmaxf(fk, 0.0f), 54.0f)
    k0 = (int)floorf(fk)
    f  = fk - (float)k0
    k1 = (k0 == 54) ? 0 : k0 + 1
    per channel: c0 = W[k0]/255, c1 = W[k1]/255
        col = (1.0f - f)*c0 + f*c1
        rad <= 1: col = 1.0f - rad*(1.0f - col);  otherwise col = col*0.75f
        byte = (uint8) fminf(fmaxf(floorf(255.0f*col), 0.0f), 255.0f)
    unknown pixels: unknown[3], in the output's channel order
    blend (with a frame, every pixel): out_c = (alpha256*byte_c + (256 - alpha256)*frame_c + 128) >> 8

Every array operation below is on float32 arrays with float32 scalars, so NumPy rounds each one to float32 on its own.
Flows are (n, 2, H, W) float32, plane 0 = u, plane 1 = v; masks (n, H, W) uint8, nonzero = unknown."""
import numpy as np

F32 = np.float32
NORMS = {"fixed": 0, "flow": 1, "batch": 2}
SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))
UNKNOWN_THRESH = F32(1e9)  # Middlebury's UNKNOWN_FLOW_THRESH
EPS = F32(2.0 ** -23)
COEFFS = tuple(F32(float.fromhex(c)) for c in ("0x1.fffd5cp-1", "-0x1.54a3a4p-2", "0x1.8ca306p-3", "-0x1.ddcd90p-4",
                                                "0x1.b0bae2p-5", "-0x1.81b21cp-7"))  # c0 .. c5
HALF_PI, PI, INV_PI = F32(1.5707964), F32(3.1415927), F32(0.31830987)


def colour_wheel():
    """The (55, 3) uint8 RGB wheel."""
    rows = []
    for name, L in SEGMENTS:
        for j in range(L):
            g = 255 * j // L
            rows.append({"RY": (255, g, 0), "YG": (255 - g, 255, 0), "GC": (0, 255, g), "CB": (0, 255 - g, 255),
                         "BM": (g, 0, 255), "MR": (255, 0, 255 - g)}[name])
    return np.array(rows, np.uint8)


def atan2_turns(y, x):
    """atan2(y, x) / pi of float32 arrays, in half-turns, by the polynomial of the text."""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    with np.errstate(all="ignore"):
        t = np.where(mx > F32(0), mn / np.where(mx > F32(0), mx, F32(1)), F32(0)).astype(F32)
        s = t * t
        p = np.full(s.shape, COEFFS[5], F32)
        for c in COEFFS[4::-1]:
            p = p * s
            p = p + c
        r = t * p
        r = np.where(ay > ax, HALF_PI - r, r)
        r = np.where(np.signbit(x), PI - r, r)
        r = np.where(np.signbit(y), -r, r)
        a = r * INV_PI
    assert a.dtype == F32
    return a


def known(flows, mask=None):
    """(n, H, W) bool: the pixels that take part."""
    flows = np.asarray(flows, F32)
    with np.errstate(all="ignore"):
        k = (np.abs(flows[:, 0]) <= UNKNOWN_THRESH) & (np.abs(flows[:, 1]) <= UNKNOWN_THRESH)
    if mask is not None:
        k &= np.asarray(mask) == 0
    return k


def max2(flows, mask=None):
    """The n + 1 float32 words M2_0 .. M2_{n-1}, MB2."""
    flows = np.asarray(flows, F32)
    n = flows.shape[0]
    k = known(flows, mask)
    with np.errstate(all="ignore"):
        r2 = flows[:, 0] * flows[:, 0] + flows[:, 1] * flows[:, 1]
    assert r2.dtype == F32
    out = np.zeros(n + 1, F32)
    for i in range(n):
        if k[i].any():
            out[i] = r2[i][k[i]].max()
    out[n] = out[:n].max() if n else F32(0)
    return out


def colour_bytes(u, v, R, measured):
    """RGB bytes (..., 3) of known flow vectors (u, v) under radius R (float32, broadcast against u)."""
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    wheel = colour_wheel().astype(F32) / F32(255.0)
    with np.errstate(all="ignore"):
        D = (np.asarray(R, F32) + EPS).astype(F32)
        un, vn = u / D, v / D
        rad = np.sqrt(un * un + vn * vn)
        if measured:
            rad = np.minimum(rad, F32(1.0))
        a = atan2_turns(-vn, -un)
        fk = (a + F32(1.0)) * F32(27.0)
        fk = np.minimum(np.maximum(fk, F32(0.0)), F32(54.0))
        fl = np.floor(fk)
        k0 = fl.astype(np.int64)
        f = fk - fl
        k1 = np.where(k0 == 54, 0, k0 + 1)
        c0, c1 = wheel[k0], wheel[k1]
        f3, rad3 = f[..., None], rad[..., None]
        col = (F32(1.0) - f3) * c0 + f3 * c1
        col = np.where(rad3 <= F32(1.0), F32(1.0) - rad3 * (F32(1.0) - col), col * F32(0.75))
        q = np.minimum(np.maximum(np.floor(F32(255.0) * col), F32(0.0)), F32(255.0))
    assert un.dtype == rad.dtype == fk.dtype == col.dtype == q.dtype == F32
    return q.astype(np.uint8)


def flow_colour(flows, norm="flow", max_rad=None, mask=None, order="rgb", layout="hwc", unknown=(0, 0, 0), frame=None,
                frame_layout="hwc", alpha256=128):
    """(images, max2): images (n, H, W, 3) or, with layout="chw", (n, 3, H, W) uint8; max2 the n + 1 float32 words.
    frame: (n, H, W) gray, or 3 channels in the output's channel order as (n, H, W, 3) / (n, 3, H, W) by frame_layout."""
    flows = np.asarray(flows, F32)
    n, _, H, W = flows.shape
    mode = NORMS[norm]
    m2 = max2(flows, mask)
    k = known(flows, mask)
    if mode == 0:
        R = np.full((n, 1, 1), F32(max_rad), F32)
    elif mode == 1:
        R = np.sqrt(m2[:n]).astype(F32).reshape(n, 1, 1)
    else:
        R = np.full((n, 1, 1), np.sqrt(m2[n]), F32)
    u, v = np.where(k, flows[:, 0], F32(0)), np.where(k, flows[:, 1], F32(0))
    rgb = colour_bytes(u, v, R, mode != 0) if n else np.empty((0, H, W, 3), np.uint8)
    img = rgb if order == "rgb" else rgb[..., ::-1]
    img = np.where(k[..., None], img, np.asarray(unknown, np.uint8).reshape(1, 1, 1, 3)).astype(np.uint8)
    if frame is not None:
        fr = np.asarray(frame, np.uint8)
        if fr.ndim == 3:
            fr = np.repeat(fr[..., None], 3, -1)
        elif frame_layout == "chw":
            fr = fr.transpose(0, 2, 3, 1)
        a = int(alpha256)
        img = ((a * img.astype(np.int64) + (256 - a) * fr.astype(np.int64) + 128) >> 8).astype(np.uint8)
    if layout == "chw":
        img = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
    return img, m2


def key_flow(size):
    """The radial flow and mask of the legend disc: u = x - c, v = y - c with c = (size - 1) / 2 in float32; the mask is 1
    outside the disc u*u + v*v <= c*c."""
    c = F32(size - 1) / F32(2)
    d = np.arange(size, dtype=F32) - c
    u, v = np.broadcast_to(d[None, :], (size, size)), np.broadcast_to(d[:, None], (size, size))
    flow = np.stack([u, v]).astype(F32)[None]
    mask = ((u * u + v * v) > c * c).astype(np.uint8)[None]
    return flow, mask


SPECIALS = ["nan_u", "nan_v", "+inf", "-inf", "1e30", "-1e30", "1e9", "above_1e9", "-0.0", "u1_v+0", "u1_v-0"]


def plant_specials(flow, skip=()):
    """Plants the special values (but those named in skip) at fixed pixels of flow (2, H, W) in place: special k goes to the
    pixel with row-major index 7 * k + 3 (modulo W * H: tiny sizes hold only the last few).  Returns {name: (x, y)}.
      nan_u / nan_v / +-inf / +-1e30 / above_1e9 (nextafter(1e9, inf)): unknown
      1e9: known, and then the flow's maximum;  -0.0: a flow of (-0.0, -0.0);  u1_v+0 / u1_v-0: the seam of the wheel"""
    _, H, W = flow.shape
    where = {}
    for k, name in enumerate(SPECIALS):
        if name in skip:
            continue
        y, x = divmod((7 * k + 3) % (W * H), W)
        where[name] = (x, y)
        flow[0, y, x], flow[1, y, x] = {
            "nan_u": (np.nan, 0.25), "nan_v": (0.25, np.nan), "+inf": (np.inf, 0.0), "-inf": (0.0, -np.inf),
            "1e30": (1e30, 0.0), "-1e30": (0.0, -1e30), "1e9": (1e9, 0.0), "above_1e9": (0.0, np.nextafter(F32(1e9), F32(np.inf))),
            "-0.0": (-0.0, -0.0), "u1_v+0": (1.0, 0.0), "u1_v-0": (1.0, -0.0)}[name]
    return where
