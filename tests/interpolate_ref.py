"""NumPy reference of the frame interpolation at time t from two frames and their flows (include/dfx.h,
dfx_interpolate_device; the kernels are denseflow_amd/csrc/interpolate_kernels.hip).  All float operations are float32, each
rounded on its own, with no fused multiply-add.  t1 = 1.0f - t.

  1. Project.  (G0, H0) = the projection of F01 with t, scale = -t, min_weight, d_occ_fwd: exactly
     dfx_flow_project_device's out and hole planes.  With d_bwd: (G1, H1) = the projection of F10 with t = t1, scale = -t1,
     d_occ_bwd.  Without d_bwd: (G1, H1) = the projection of F01 with t, scale = t1; the sums are the same, so H1 = H0.
  2. Fill.  (Gf_k, Hf_k) = (G_k, H_k) after fill_passes applications of dfx_flow_median_device in DFX_MEDIAN_FILL with
     ksize, mask_out fed back as the mask, each side filled as its own flow.  With fill_passes = 0, Gf = G and Hf = H.
  3. Synthesise.  Per output pixel (x, y) and side k, with (gu, gv) = Gf_k(x, y):
         px = (float)x + gu;  py = (float)y + gv
         inside_k = px >= 0 && py >= 0 && px <= W-1 && py <= H-1      (dfx_warp_device's test, word for word)
         s_k = dfx_warp_device's bilinear sample of I_k at (px, py), per channel (taken where inside_k)
         prim_k = (H_k == 0) && inside_k;   cand_k = (Hf_k == 0) && inside_k
         (w0, w1) = (prim_0 || prim_1) ? (prim_0, prim_1) : (cand_0, cand_1)
         o = s0 + t*(s1 - s0)       both w0 and w1
             s_k                    only w_k
             P0 + t*(P1 - P0)       neither; P0, P1 the pixel's own bytes in I0, I1 as float
         o = fminf(fmaxf(o, 0), 255)
         stored: (uint8)rintf(o) for DFX_WARP_U8 (ties to even), o for DFX_PLANAR_F32
         source plane (uint8, optional): 0 both, 1 frame 0 only, 2 frame 1 only, 3 neither; plus 4 when the second tier
         (the filled flows) decided; 3 never carries 4.

Steps 1 and 2 and the sample are the committed references: tests/flow_project_ref.py, tests/flow_median_ref.py and
tests/warp_ref.py.  interpolate is the vectorised form, interpolate_loop a plain scalar loop over the pixels of step 3 on the
scalar forms of the projection and the sample (tests/test_interpolate_ref.py holds them against each other).  Images are
(H, W) or (H, W, C) uint8 arrays (channels last), flows (2, H, W) float32, masks (H, W) uint8."""
import numpy as np

from tests import flow_project_ref as P
from tests import warp_ref as WR
from tests.flow_median_ref import flow_median_batch

F32 = np.float32


def flows_at_t(fwd, bwd=None, t=0.5, occ_fwd=None, occ_bwd=None, fill_passes=3, ksize=3, min_weight=0.25, loop=False):
    """Steps 1 and 2 of one pair: ((G0, G1), (H0, H1), (Gf0, Gf1), (Hf0, Hf1))."""
    t = F32(t)
    t1 = F32(1.0) - t
    assert 0 <= fill_passes <= 16 and ksize in (3, 5)
    assert occ_bwd is None or bwd is not None
    proj = P.project_loop if loop else P.project
    one = lambda m: None if m is None else np.asarray(m, np.uint8)[None]  # noqa: E731
    fwd = np.asarray(fwd, F32)
    g0, h0, _ = proj(fwd[None], t=t, scale=-t, occ=one(occ_fwd), min_weight=min_weight)
    if bwd is not None:
        g1, h1, _ = proj(np.asarray(bwd, F32)[None], t=t1, scale=-t1, occ=one(occ_bwd), min_weight=min_weight)
    else:
        g1, h1, _ = proj(fwd[None], t=t, scale=t1, occ=one(occ_fwd), min_weight=min_weight)
    G, Hh = (g0[0], g1[0]), (h0[0], h1[0])
    if fill_passes == 0:
        return G, Hh, G, Hh
    filled = [flow_median_batch(g[None], ksize, h[None], "fill", fill_passes) for g, h in zip(G, Hh)]
    return G, Hh, tuple(f[0][0] for f in filled), tuple(f[1][0] for f in filled)


def synthesise(img0, img1, Gf, Hh, Hf, t):
    """Step 3, vectorised: (o float32 in the images' shape, source (H, W) uint8)."""
    t = F32(t)
    img0, img1 = np.asarray(img0, np.uint8), np.asarray(img1, np.uint8)
    H, W = Hh[0].shape
    s, ins = [], []
    for img, g in ((img0, Gf[0]), (img1, Gf[1])):
        sk, valid = WR.warp(img, g, "zero")
        s.append(sk.reshape(H, W, -1))
        ins.append(valid != 0)
    prim = [(Hh[k] == 0) & ins[k] for k in (0, 1)]
    cand = [(Hf[k] == 0) & ins[k] for k in (0, 1)]
    first = prim[0] | prim[1]
    w0, w1 = np.where(first, prim[0], cand[0]), np.where(first, prim[1], cand[1])
    p0, p1 = img0.reshape(H, W, -1).astype(F32), img1.reshape(H, W, -1).astype(F32)
    both = s[0] + t * (s[1] - s[0])
    own = p0 + t * (p1 - p0)
    assert both.dtype == F32 and own.dtype == F32
    b, a0, a1 = (w0 & w1)[..., None], (w0 & ~w1)[..., None], (w1 & ~w0)[..., None]
    o = np.where(b, both, np.where(a0, s[0], np.where(a1, s[1], own)))
    o = np.minimum(np.maximum(o, F32(0)), F32(255)).astype(F32)
    source = np.where(w0 & w1, 0, np.where(w0, 1, np.where(w1, 2, 3))).astype(np.uint8)
    source = np.where(~first & (w0 | w1), source + 4, source).astype(np.uint8)
    return o.reshape(img0.shape), source


def synthesise_loop(img0, img1, Gf, Hh, Hf, t):
    """Step 3, pixel by pixel in NumPy float32 scalars, on warp_ref.warp_loop's samples."""
    t = F32(t)
    img0, img1 = np.asarray(img0, np.uint8), np.asarray(img1, np.uint8)
    H, W = Hh[0].shape
    P0, P1 = img0.reshape(H, W, -1), img1.reshape(H, W, -1)
    C = P0.shape[2]
    s0, in0 = WR.warp_loop(img0, Gf[0], "zero")
    s1, in1 = WR.warp_loop(img1, Gf[1], "zero")
    s0, s1 = s0.reshape(H, W, C), s1.reshape(H, W, C)
    o = np.zeros((H, W, C), F32)
    source = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            prim0, prim1 = bool(Hh[0][y, x] == 0 and in0[y, x]), bool(Hh[1][y, x] == 0 and in1[y, x])
            cand0, cand1 = bool(Hf[0][y, x] == 0 and in0[y, x]), bool(Hf[1][y, x] == 0 and in1[y, x])
            first = prim0 or prim1
            w0, w1 = (prim0, prim1) if first else (cand0, cand1)
            for c in range(C):
                if w0 and w1:
                    v = s0[y, x, c] + t * (s1[y, x, c] - s0[y, x, c])
                elif w0:
                    v = s0[y, x, c]
                elif w1:
                    v = s1[y, x, c]
                else:
                    p0, p1 = F32(P0[y, x, c]), F32(P1[y, x, c])
                    v = p0 + t * (p1 - p0)
                o[y, x, c] = min(max(F32(v), F32(0)), F32(255))
            code = 0 if (w0 and w1) else 1 if w0 else 2 if w1 else 3
            source[y, x] = code + (4 if (not first and code != 3) else 0)
    return o.reshape(img0.shape), source


def interpolate(img0, img1, fwd, bwd=None, t=0.5, occ_fwd=None, occ_bwd=None, fill_passes=3, ksize=3, min_weight=0.25,
                loop=False):
    """One pair: (o float32 in the images' shape, source (H, W) uint8)."""
    _, Hh, Gf, Hf = flows_at_t(fwd, bwd, t, occ_fwd, occ_bwd, fill_passes, ksize, min_weight, loop)
    return (synthesise_loop if loop else synthesise)(img0, img1, Gf, Hh, Hf, t)


def interpolate_loop(img0, img1, fwd, bwd=None, **kw):
    return interpolate(img0, img1, fwd, bwd, loop=True, **kw)


def stored(o, dtype):
    """What the device stores for o: uint8 ("uint8": rint, ties to even) or float32 ("float32")."""
    assert dtype in ("uint8", "float32")
    return WR.quantise(o) if dtype == "uint8" else np.asarray(o, F32)


def interpolate_batch(img0, img1, fwd, bwd=None, occ_fwd=None, occ_bwd=None, **kw):
    """n pairs: (o (n, ...) float32, source (n, H, W) uint8)."""
    pick = lambda a, i: None if a is None else a[i]  # noqa: E731
    res = [interpolate(img0[i], img1[i], fwd[i], pick(bwd, i), occ_fwd=pick(occ_fwd, i), occ_bwd=pick(occ_bwd, i), **kw)
           for i in range(len(fwd))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def plain_blend(img0, img1, t):
    """rint(P0 + t (P1 - P0)) as uint8: what the call gives where neither frame is usable, and the baseline of the quality
    figures."""
    t = F32(t)
    p0, p1 = np.asarray(img0, np.uint8).astype(F32), np.asarray(img1, np.uint8).astype(F32)
    return WR.quantise(np.minimum(np.maximum(p0 + t * (p1 - p0), F32(0)), F32(255)))


def mean_abs_error(a, b):
    return float(np.abs(np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)).mean())


same_bits = P.same_bits
