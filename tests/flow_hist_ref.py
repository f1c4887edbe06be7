"""NumPy reference of the motion descriptors of flows (include/dfx.h section (0.5.2), dfx_flow_hist_device; the kernel is
denseflow_amd/csrc/flow_hist_kernels.hip): per cell the orientation histograms of the flow (HOF) and of the spatial derivatives
of u and v (MBHx, MBHy).  Float32 throughout, one rounding per operation, no fused multiply-add, IEEE / and sqrtf, subnormals
kept; integer sums; the normalisation in float64:

    known = (mask == NULL || mask[y][x] == 0) && |u| <= 1e9f && |v| <= 1e9f          (false for NaN and both infinities)
    HOF : (gx, gy) = (u, v); takes part where known
    MBHX: gx = u(min(x+1, W-1), y) - u(max(x-1, 0), y);  gy = u(x, min(y+1, H-1)) - u(x, max(y-1, 0)); takes part where the
          pixel and its four clamped neighbours are all known
    MBHY: the same on v
    m = sqrtf(gx*gx + gy*gy)
    a = atan2_turns(gy, gx)
    Q = llrintf(m * 256.0f)
    hb = 0.5f * (float)bins
    fk = a * hb
    if (fk < 0) fk = fk + (float)bins
    k0 = (int)floorf(fk)
    f  = fk - (float)k0
    if (k0 == bins) { k0 = 0; f = 0; }
    k1 = (k0 + 1 == bins) ? 0 : k0 + 1
    F  = (int)rintf(f * 256.0f)
    w1 = (Q * F + 128) >> 8
    w0 = Q - w1
    the pixel adds w0 to slot k0 and w1 to slot k1 of cell (x / cell, y / cell); HOF only: if m <= still_thr it adds 256 to
    slot `bins` instead
    d_out: NONE S_b / 256;  L1 T ? S_b / T : 0;  L1_SQRT T ? sqrt(S_b / T) : 0;  L2 E > 0 ? S_b / sqrt(E) : 0 with
    E = sum of S_b * S_b in slot order; in float64, rounded once to float32

Flows are (n, 2, H, W) float32, plane 0 = u, plane 1 = v; masks (n, H, W) uint8, nonzero = not here."""
import numpy as np

from tests.flow_colour_ref import atan2_turns, known

F32 = np.float32
KINDS = {"hof": 1, "mbhx": 2, "mbhy": 4}
NORMS = {"none": 0, "l1": 1, "l1_sqrt": 2, "l2": 3}
CELLS = (4, 8, 16, 32)


def kinds_code(kinds):
    return kinds if isinstance(kinds, int) else sum(KINDS[k] for k in ((kinds,) if isinstance(kinds, str) else kinds))


def channels(kinds, bins):
    """[(name, first slot, slots)] of the channels in their order."""
    code, out, at = kinds_code(kinds), [], 0
    for name, bit in KINDS.items():
        if code & bit:
            length = bins + 1 if bit == 1 else bins
            out.append((name, at, length))
            at += length
    return out


def slots(kinds, bins):
    return sum(length for _, _, length in channels(kinds, bins))


def vectors(flows, mask=None):
    """{"hof" | "mbhx" | "mbhy": (gx, gy, part)}: (n, H, W) float32 vectors (0 where the pixel does not take part) and bool."""
    flows = np.asarray(flows, F32)
    n, _, H, W = flows.shape
    k = known(flows, mask)
    u, v = np.where(k, flows[:, 0], F32(0)), np.where(k, flows[:, 1], F32(0))
    xm, xp = np.maximum(np.arange(W) - 1, 0), np.minimum(np.arange(W) + 1, W - 1)
    ym, yp = np.maximum(np.arange(H) - 1, 0), np.minimum(np.arange(H) + 1, H - 1)
    part = k & k[:, :, xm] & k[:, :, xp] & k[:, ym] & k[:, yp]
    out = {"hof": (u, v, k)}
    for name, p in (("mbhx", u), ("mbhy", v)):
        gx, gy = p[:, :, xp] - p[:, :, xm], p[:, yp] - p[:, ym]
        assert gx.dtype == gy.dtype == F32
        out[name] = (np.where(part, gx, F32(0)), np.where(part, gy, F32(0)), part)
    return out


def bin_weights(gx, gy, bins):
    """(m, Q, k0, k1, w0, w1) of finite float32 vectors: the text's magnitude and binning."""
    gx, gy = np.asarray(gx, F32), np.asarray(gy, F32)
    fb = F32(bins)
    with np.errstate(all="ignore"):
        m = np.sqrt(gx * gx + gy * gy)
        a = atan2_turns(gy, gx)
        Q = np.rint(m * F32(256.0)).astype(np.int64)
        hb = F32(0.5) * fb
        fk = a * hb
        fk = np.where(fk < F32(0), fk + fb, fk)
        fl = np.floor(fk)
        k0 = fl.astype(np.int64)
        f = fk - fl
        wrap = k0 == bins
        k0 = np.where(wrap, 0, k0)
        f = np.where(wrap, F32(0), f)
        k1 = np.where(k0 + 1 == bins, 0, k0 + 1)
        F = np.rint(f * F32(256.0)).astype(np.int64)
    assert m.dtype == a.dtype == fk.dtype == f.dtype == F32
    assert k0.min(initial=0) >= 0 and k0.max(initial=0) < bins and F.min(initial=0) >= 0 and F.max(initial=0) <= 256
    w1 = (Q * F + 128) >> 8
    w0 = Q - w1
    return m, Q, k0, k1, w0, w1


def flow_hist_sums(flows, kinds=("hof", "mbhx", "mbhy"), cell=8, bins=8, still_thr=0.4, mask=None):
    """The integer sums (n, CH, CW, D) int64."""
    flows = np.asarray(flows, F32)
    n, _, H, W = flows.shape
    CH, CW = -(-H // cell), -(-W // cell)
    D = slots(kinds, bins)
    sums = np.zeros((n, CH, CW, D), np.int64)
    vec = vectors(flows, mask)
    ii, yy, xx = np.meshgrid(np.arange(n), np.arange(H) // cell, np.arange(W) // cell, indexing="ij")
    thr = F32(still_thr)
    for name, base, _ in channels(kinds, bins):
        gx, gy, part = vec[name]
        m, Q, k0, k1, w0, w1 = bin_weights(gx, gy, bins)
        if name == "hof":
            still = part & (m <= thr)
            np.add.at(sums, (ii[still], yy[still], xx[still], base + bins), 256)
            part = part & ~still
        np.add.at(sums, (ii[part], yy[part], xx[part], base + k0[part]), w0[part])
        np.add.at(sums, (ii[part], yy[part], xx[part], base + k1[part]), w1[part])
    return sums


def normalise(sums, kinds, bins, norm="none"):
    """The float32 values (n, CH, CW, D) of integer sums (n, CH, CW, D)."""
    sums = np.asarray(sums, np.int64)
    mode = NORMS[norm]
    S = sums.astype(np.float64)
    out = np.zeros(sums.shape, F32)
    if mode == 0:
        return (S / 256.0).astype(F32)
    for _, base, length in channels(kinds, bins):
        s = S[..., base:base + length]
        if mode == 3:
            E = np.zeros(s.shape[:-1], np.float64)
            for b in range(length):  # slot order, each step rounded
                sq = s[..., b] * s[..., b]
                E = E + sq
            d = np.sqrt(E)
        else:
            d = sums[..., base:base + length].sum(-1).astype(np.float64)
        ok = d > 0
        with np.errstate(all="ignore"):
            val = s / np.where(ok, d, 1.0)[..., None]
            if mode == 2:
                val = np.sqrt(val)
        out[..., base:base + length] = np.where(ok[..., None], val, 0.0).astype(F32)
    return out


def flow_hist(flows, kinds=("hof", "mbhx", "mbhy"), cell=8, bins=8, still_thr=0.4, norm="none", mask=None):
    """(values (n, D, CH, CW) float32, sums (n, CH, CW, D) int64)."""
    sums = flow_hist_sums(flows, kinds, cell, bins, still_thr, mask)
    return np.ascontiguousarray(normalise(sums, kinds, bins, norm).transpose(0, 3, 1, 2)), sums


def flow_hist_f64(flows, kinds=("hof", "mbhx", "mbhy"), cell=8, bins=8, still_thr=0.4, mask=None):
    """The same rule in float64 with the true arctan2 and unquantised weights, as (n, CH, CW, D) float64 in units of pixels
    times magnitude: what the float32 / integer definition is measured against (not part of it)."""
    flows = np.asarray(flows, F32)
    n, _, H, W = flows.shape
    CH, CW = -(-H // cell), -(-W // cell)
    out = np.zeros((n, CH, CW, slots(kinds, bins)), np.float64)
    vec = vectors(flows, mask)
    ii, yy, xx = np.meshgrid(np.arange(n), np.arange(H) // cell, np.arange(W) // cell, indexing="ij")
    for name, base, _ in channels(kinds, bins):
        gx, gy, part = vec[name]
        gx, gy = gx.astype(np.float64), gy.astype(np.float64)
        m = np.hypot(gx, gy)
        fk = np.mod(np.arctan2(gy, gx) / np.pi * (0.5 * bins), bins)
        k0 = np.floor(fk).astype(np.int64) % bins
        f = fk - np.floor(fk)
        k1 = (k0 + 1) % bins
        if name == "hof":
            still = part & (m <= float(F32(still_thr)))
            np.add.at(out, (ii[still], yy[still], xx[still], base + bins), 1.0)
            part = part & ~still
        np.add.at(out, (ii[part], yy[part], xx[part], base + k0[part]), (m * (1 - f))[part])
        np.add.at(out, (ii[part], yy[part], xx[part], base + k1[part]), (m * f)[part])
    return out
