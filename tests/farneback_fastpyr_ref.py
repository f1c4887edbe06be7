"""The reference of -a=farn with fast pyramids (dfx_params.farn_fast_pyramids): oracle/'s own
driver restated over its exported stage functions, as tests/farneback_window_ref.py and tests/initial_flow_ref.py do, with
the pyramid construction exchangeable.  oracle.farneback_calc refuses fast_pyramids, and oracle/ is not touched.

  * fast=False: the blur + resize pyramid and the bilinear flow up-sampling of orc_farneback_calc.  With window="box" and no
    seed the composition equals oracle.farneback_calc bit for bit (tests/test_farneback_fastpyr_ref.py holds it to that).
  * fast=True:  upstream's fastPyramids path (opencv_contrib 4.5.x, cudaoptflow/src/farneback.cpp with cudawarping's
    pyr_down.cu / pyr_up.cu) restated from memory of those files, rated MED (the pyrUp border rule LOW): level 0 is the
    frame as float, level k = pyr_down(level k - 1), the level sizes are the pyramid's, and a flow climbs a level as
    pyr_up(flow) * (float)(1 / pyrScale).  The level crop, the polynomial expansion, the update window, updateMatrices,
    updateFlow and the seed of the coarsest level are the default path's.

pyr_down and pyr_up are float32 throughout: every product and every sum is one float32 array operation, left to right,
nothing contracts.  Test infrastructure only."""
import ctypes as C

import numpy as np

from tests import farneback_window_ref as WR

F = np.float32
TAPS = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))


def _reflect101(i, n):
    """BORDER_REFLECT_101 of an index array into [0, n)."""
    if n == 1:
        return np.zeros_like(i)
    i = np.abs(i) % (2 * (n - 1))
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def pyr_down(src):
    """(h, w) float32 -> ((h + 1) / 2, (w + 1) / 2): the 5-tap filter at every second row of every source column
    (reflect-101), then at every second column of that."""
    src = np.asarray(src)
    assert src.dtype == F and src.ndim == 2
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    ys, xs = 2 * np.arange(dh), 2 * np.arange(dw)
    v = TAPS[0] * src[_reflect101(ys - 2, h), :]
    for j in range(1, 5):
        v = v + TAPS[j] * src[_reflect101(ys - 2 + j, h), :]
    d = TAPS[0] * v[:, _reflect101(xs - 2, w)]
    for j in range(1, 5):
        d = d + TAPS[j] * v[:, _reflect101(xs - 2 + j, w)]
    assert d.dtype == F and d.shape == (dh, dw)
    return np.ascontiguousarray(d)


def _up_axis0(s):
    """One pass of pyr_up along axis 0: n rows -> 2n, border index min(|i|, n - 1)."""
    n = s.shape[0]
    a = np.arange(n)
    lo, hi = np.minimum(np.abs(a - 1), n - 1), np.minimum(a + 1, n - 1)
    even = TAPS[0] * s[lo] + TAPS[2] * s
    even = even + TAPS[4] * s[hi]
    odd = TAPS[1] * s + TAPS[3] * s[hi]
    out = np.empty((2 * n,) + s.shape[1:], F)
    out[0::2], out[1::2] = even, odd
    return out


def pyr_up(src):
    """(h, w) float32 -> (2h, 2w): the even / odd phase forms along the rows' direction first (horizontal pass), then down
    the rows, times 4.  The stuffed zeros' products are left out: they change nothing for finite inputs."""
    src = np.asarray(src)
    assert src.dtype == F and src.ndim == 2
    t = np.ascontiguousarray(_up_axis0(np.ascontiguousarray(src.T)).T)  # horizontal
    out = _up_axis0(t) * F(4.0)
    assert out.dtype == F and out.shape == (2 * src.shape[0], 2 * src.shape[1])
    return np.ascontiguousarray(out)


def crop_levels(W, H, num_levels, pyr_scale):
    """numLevelsCropped of B.2."""
    scale, cropped = 1.0, 0
    while cropped < num_levels:
        scale *= pyr_scale
        if W * scale < WR.MIN_SIZE or H * scale < WR.MIN_SIZE:
            break
        cropped += 1
    return cropped


def fast_level_sizes(W, H, cropped):
    """[(w, h)] of levels 0 .. cropped on the (n + 1) / 2 chain; None where a level below the coarsest is odd."""
    sizes, w, h = [], W, H
    for k in range(cropped + 1):
        if k < cropped and (w & 1 or h & 1):
            return None
        sizes.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return sizes


def farneback_flow(oracle, frame0, frame1, params=None, fast=False, window="box", seed=None):
    """orc_farneback_calc's loop over the oracle's stage functions.  params: oracle.FarnebackParams (flags and fast_pyramids
    stay 0: the window, the pyramids and the seed are this function's arguments).  seed: an (H, W, 2) initial flow for the
    coarsest level, or None.  Returns the (H, W, 2) float32 flow."""
    assert window in ("box", "gaussian")
    L = oracle.lib()
    p = params if params is not None else oracle.farneback_default_params()
    f0 = np.ascontiguousarray(frame0, dtype=np.uint8)
    f1 = np.ascontiguousarray(frame1, dtype=np.uint8)
    assert f0.shape == f1.shape and f0.ndim == 2
    H, W = f0.shape
    assert p.poly_n in (5, 7) and not p.fast_pyramids and p.flags == 0 and p.win_size >= 1 and p.win_size & 1
    if seed is not None:
        assert seed.shape == (H, W, 2)
    oracle._pick_threads(H, W, None)
    frames = [f0.astype(F), f1.astype(F)]  # convertTo(CV_32F), alpha = 1: exact
    cropped = crop_levels(W, H, p.num_levels, p.pyr_scale)
    pyramids = None
    if fast:
        assert p.pyr_scale == 0.5, "upstream asserts pyrScale == 0.5 with fastPyramids"
        sizes = fast_level_sizes(W, H, cropped)
        assert sizes is not None, "a level below the coarsest is odd: upstream defines no result"
        pyramids = [[frames[0]], [frames[1]]]
        for pyr in pyramids:
            for k in range(1, cropped + 1):
                pyr.append(pyr_down(pyr[-1]))
            assert [(a.shape[1], a.shape[0]) for a in pyr] == sizes

    pc = WR.PolyConsts()
    L.orc_farneback_prepare_poly(C.c_int(p.poly_n), C.c_double(p.poly_sigma), C.byref(pc))
    half_win = p.win_size // 2
    taps = WR.window_taps(oracle, p.win_size) if window == "gaussian" else None
    inv = lambda dst, src: float(F(1.0 / (float(dst) / float(src))))  # orc_inv_scale_from_sizes
    up = F(1.0 / p.pyr_scale)

    prev = None  # (flow x, flow y, width, height) of the coarser level
    for k in range(cropped, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= p.pyr_scale
        if fast:
            w, h = sizes[k]
        else:
            sigma = (1.0 / scale - 1) * 0.5
            smooth = max(int(np.rint(sigma * 5)) | 1, 3)
            w, h = int(np.rint(W * scale)), int(np.rint(H * scale))
        if prev is None and seed is None:
            curx, cury = np.zeros((h, w), F), np.zeros((h, w), F)
        elif prev is None:  # OPTFLOW_USE_INITIAL_FLOW (B.12): the coarsest level only, the same on both paths
            curx = oracle.resize_linear(np.ascontiguousarray(seed[..., 0], dtype=F), w, h, inv(w, W), inv(h, H)) * F(scale)
            cury = oracle.resize_linear(np.ascontiguousarray(seed[..., 1], dtype=F), w, h, inv(w, W), inv(h, H)) * F(scale)
        elif fast:
            curx, cury = pyr_up(prev[0]) * up, pyr_up(prev[1]) * up
            assert curx.shape == (h, w)
        else:
            px, py, pw, ph = prev
            curx = oracle.resize_linear(px, w, h, inv(w, pw), inv(h, ph)) * up
            cury = oracle.resize_linear(py, w, h, inv(w, pw), inv(h, ph)) * up
        R = []
        for i, f in enumerate(frames):
            if fast:
                pyr = pyramids[i][k]
            else:
                gk = WR.gaussian_kernel(oracle, smooth, sigma)
                ker_half = np.ascontiguousarray(gk[smooth // 2:])
                blurred = np.empty((H, W), F)
                L.orc_farneback_gaussian_blur(WR._p(f), C.c_int(W), C.c_int(H), WR._p(ker_half), C.c_int(smooth // 2),
                                              WR._p(blurred))
                pyr = oracle.resize_linear(blurred, w, h, inv(w, W), inv(h, H))
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
    return np.ascontiguousarray(np.stack([prev[0], prev[1]], axis=-1))
