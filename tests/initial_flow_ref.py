"""The references of caller-supplied initial flows (dfx_calc_batch_init*): OpticalFlowDual_TVL1's useInitialFlow and
Farneback's OPTFLOW_USE_INITIAL_FLOW, assembled from the oracle's stage functions (imported, oracle/ stays as it is) and
the existing references tests/tvl1_gamma_ref.py and tests/farneback_window_ref.py.  Test infrastructure only.

Semantics (SURVEY.md Appendix A / B "initial flow"; restated from memory of opencv_contrib 4.5.x cudaoptflow, rated MED,
parity unpinned):

  TVL1       u1[0], u2[0] = the seed's u and v; for s = 1 .. n-1 (n = the levels actually used, after the < 16 cut)
             u[s] = resize_linear(u[s-1], w_s, h_s, ifx, ify) * (float)scaleStep with ifx = (float)(1.0 / ((double)w_s /
             w_{s-1})), every level rounded to float before the next reads it; u[n-1] replaces the zeros at the coarsest
             level and everything after that is the unseeded algorithm.  n = 1: the seed as it is.  u3 (gamma) starts at 0.
  Farneback  at the coarsest level k only, flow = resize_linear(seed, w_k, h_k, ifx, ify) * (float)scale_k, scale_k the
             double that the level loop accumulates (pyrScale multiplied k times), ifx = (float)(1.0 / ((double)w_k / W)).

init = None is the unseeded algorithm through the same code; tests/test_initial_flow_ref.py holds that, and an all-zero
seed, to the oracle bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import farneback_window_ref as WR
from tests import tvl1_gamma_ref as GR

F = np.float32


def _inv(dst, src):
    return float(F(1.0 / (float(dst) / float(src))))  # orc_inv_scale_from_sizes


def tvl1_levels(w, h, nscales, scale_step):
    """(w, h) of the levels OpticalFlowDual_TVL1 uses: cvRound per level, the level below 16 px and all after it cut."""
    sizes = [(w, h)]
    for _ in range(1, nscales):
        pw, ph = sizes[-1]
        nw, nh = int(np.rint(pw * scale_step)), int(np.rint(ph * scale_step))
        if nw < 16 or nh < 16:
            break
        sizes.append((nw, nh))
    return sizes


def tvl1_seed_chain(oracle, init, sizes, scale_step):
    """The seed carried to the coarsest of `sizes`: (u1, u2) float32 planes there."""
    u = [np.ascontiguousarray(init[..., ch], dtype=F) for ch in range(2)]
    for s in range(1, len(sizes)):
        (dw, dh), (sw, sh) = sizes[s], sizes[s - 1]
        u = [(oracle.resize_linear(p, dw, dh, _inv(dw, sw), _inv(dh, sh)) * F(scale_step)).astype(F) for p in u]
    return u


def tvl1_init_calc(oracle, frame0, frame1, init=None, gamma=0.0, nscales=5, warps=5, iterations=300, epsilon=0.01,
                   scale_step=0.8, tau=0.25, lam=0.15, theta=0.3):
    """Returns (flow (H, W, 2), iteration table [level][warp], convergence sums evaluated).  gamma = 0: the levels run
    orc_tvl1_proc_one_scale; otherwise tests/tvl1_gamma_ref._proc_one_scale with u3 = 0 at the coarsest level."""
    f0 = np.ascontiguousarray(frame0, dtype=np.uint8)
    f1 = np.ascontiguousarray(frame1, dtype=np.uint8)
    H, W = f0.shape
    if init is not None:
        assert init.shape == (H, W, 2)
    sizes = tvl1_levels(W, H, nscales, scale_step)
    n = len(sizes)
    ifs = float(F(1.0 / scale_step))
    I0s, I1s = [f0.astype(F)], [f1.astype(F)]
    for s in range(1, n):
        I0s.append(oracle.resize_linear(I0s[-1], sizes[s][0], sizes[s][1], ifs, ifs))
        I1s.append(oracle.resize_linear(I1s[-1], sizes[s][0], sizes[s][1], ifs, ifs))
    cw, ch = sizes[-1]
    if init is None:
        u = [np.zeros((ch, cw), F), np.zeros((ch, cw), F)]
    else:
        u = tvl1_seed_chain(oracle, init, sizes, scale_step)
    prm = oracle.tvl1_default_params()
    prm.tau, prm.lambda_, prm.theta, prm.nscales, prm.warps = tau, lam, theta, nscales, warps
    prm.epsilon, prm.iterations, prm.scale_step = epsilon, iterations, scale_step
    trace = oracle.Tvl1Trace()
    table, checks = [None] * n, 0
    u3 = np.zeros((ch, cw), F)
    oracle._pick_threads(H, W, None)
    for s in range(n - 1, -1, -1):
        w, h = sizes[s]
        if gamma == 0.0:
            u = [np.ascontiguousarray(p, dtype=F) for p in u]
            oracle.lib().orc_tvl1_proc_one_scale(np.ascontiguousarray(I0s[s]), np.ascontiguousarray(I1s[s]), u[0], u[1], w, h,
                                                 C.byref(prm), s, C.byref(trace))
            table[s] = [trace.iters[s][k] for k in range(warps)]
            checks = trace.n_checks
        else:
            (u0, u1, u3), table[s], ck = GR._proc_one_scale(I0s[s], I1s[s], [u[0], u[1], u3], F(gamma), warps, iterations,
                                                            epsilon, lam, theta, tau)
            u = [u0, u1]
            checks += ck
        if s > 0:
            dw, dh = sizes[s - 1]
            up = F(1.0 / scale_step)
            u = [(oracle.resize_linear(p, dw, dh, _inv(dw, w), _inv(dh, h)) * up).astype(F) for p in u]
            u3 = oracle.resize_linear(u3, dw, dh, _inv(dw, w), _inv(dh, h))
    return np.ascontiguousarray(np.stack([u[0], u[1]], axis=-1)), table, int(checks)


def farneback_init_calc(oracle, frame0, frame1, init=None, params=None, window="box"):
    """tests/farneback_window_ref.farneback_flow's loop (orc_farneback_calc's) with the coarsest level's flow taken from
    the seed.  Returns (flow (H, W, 2), levels used)."""
    assert window in ("box", "gaussian")
    L = oracle.lib()
    p = params if params is not None else oracle.farneback_default_params()
    f0 = np.ascontiguousarray(frame0, dtype=np.uint8)
    f1 = np.ascontiguousarray(frame1, dtype=np.uint8)
    H, W = f0.shape
    assert p.poly_n in (5, 7) and not p.fast_pyramids and p.flags == 0 and p.win_size >= 1 and p.win_size & 1
    if init is not None:
        assert init.shape == (H, W, 2)
    oracle._pick_threads(H, W, None)
    frames = [f0.astype(F), f1.astype(F)]
    scale, cropped = 1.0, 0
    while cropped < p.num_levels:
        scale *= p.pyr_scale
        if W * scale < WR.MIN_SIZE or H * scale < WR.MIN_SIZE:
            break
        cropped += 1
    pc = WR.PolyConsts()
    L.orc_farneback_prepare_poly(C.c_int(p.poly_n), C.c_double(p.poly_sigma), C.byref(pc))
    half_win = p.win_size // 2
    taps = WR.window_taps(oracle, p.win_size) if window == "gaussian" else None
    prev = None
    for k in range(cropped, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= p.pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        smooth = max(int(np.rint(sigma * 5)) | 1, 3)
        w, h = int(np.rint(W * scale)), int(np.rint(H * scale))
        if prev is None and init is None:
            curx, cury = np.zeros((h, w), F), np.zeros((h, w), F)
        elif prev is None:  # OPTFLOW_USE_INITIAL_FLOW: the coarsest level only
            curx = oracle.resize_linear(np.ascontiguousarray(init[..., 0], dtype=F), w, h, _inv(w, W), _inv(h, H)) * F(scale)
            cury = oracle.resize_linear(np.ascontiguousarray(init[..., 1], dtype=F), w, h, _inv(w, W), _inv(h, H)) * F(scale)
        else:
            px, py, pw, ph = prev
            up = F(1.0 / p.pyr_scale)
            curx = oracle.resize_linear(px, w, h, _inv(w, pw), _inv(h, ph)) * up
            cury = oracle.resize_linear(py, w, h, _inv(w, pw), _inv(h, ph)) * up
        gk = WR.gaussian_kernel(oracle, smooth, sigma)
        ker_half = np.ascontiguousarray(gk[smooth // 2:])
        R = []
        for f in frames:
            blurred = np.empty((H, W), F)
            L.orc_farneback_gaussian_blur(WR._p(f), C.c_int(W), C.c_int(H), WR._p(ker_half), C.c_int(smooth // 2), WR._p(blurred))
            pyr = oracle.resize_linear(blurred, w, h, _inv(w, W), _inv(h, H))
            Rf = np.empty((5, h, w), F)
            L.orc_farneback_poly_exp(WR._p(pyr), C.c_int(w), C.c_int(h), C.c_int(p.poly_n), C.byref(pc), WR._p(Rf))
            R.append(Rf)
        curx, cury = np.ascontiguousarray(curx, dtype=F), np.ascontiguousarray(cury, dtype=F)

        def update_matrices():
            M = np.empty((5, h, w), F)
            L.orc_farneback_update_matrices(WR._p(curx), WR._p(cury), WR._p(R[0]), WR._p(R[1]), C.c_int(w), C.c_int(h), WR._p(M))
            return M

        M = update_matrices()
        for it in range(p.num_iters):
            M = np.ascontiguousarray(WR.gauss5(M, w, h, taps)) if window == "gaussian" else WR._box5(oracle, M, w, h, half_win)
            L.orc_farneback_update_flow(WR._p(M), C.c_int(w), C.c_int(h), WR._p(curx), WR._p(cury))
            if it < p.num_iters - 1:
                M = update_matrices()
        prev = (curx, cury, w, h)
    return np.ascontiguousarray(np.stack([prev[0], prev[1]], axis=-1)), cropped + 1


def seeded_inputs(w, h, clip_seed):
    """The inputs of the GPU cases: frames 0, 6, 12, 18 of SynthClip(w, h, clip_seed) — three pairs of about 10 px of
    motion each — and one seed per pair, distinct so that a pair <-> seed mix-up fails: zeros, the pair's true flow, half
    of the pair's true flow.  Returns (frames, seeds), the seeds (H, W, 2) float32 and read-only."""
    from denseflow_amd.synth import SynthClip

    clip = SynthClip(w, h, clip_seed)
    frames = clip.frames(19)[::6]
    seeds = [np.zeros((h, w, 2), F), clip.true_flow(6, 12).astype(F), (F(0.5) * clip.true_flow(12, 18).astype(F)).astype(F)]
    for s in seeds:
        s.setflags(write=False)
    return frames, seeds
