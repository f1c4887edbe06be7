"""The reference of the Farneback update window (dfx_params.farn_window): oracle/'s own driver, restated over its exported
stage functions, with the window step exchangeable.

oracle.farneback_calc refuses non-zero flags, and oracle/ is not touched.  Its driver (orc_farneback_calc) is only a
composition of stage functions the library exports, so `farneback_flow` restates that loop in Python — the level crop,
smoothSize, cvRound as rint, the 1 / (dst / src) inverse scales and the 1 / pyrScale up-scaling follow the C text — and
takes the step between updateMatrices and updateFlow as an argument:

  * window="box":      orc_farneback_box_filter5.  The composition then equals oracle.farneback_calc bit for bit
                       (tests/test_farneback_window_ref.py holds it to that), so it cannot drift from the oracle unnoticed.
  * window="gaussian": gauss5 below, upstream's updateFlow_gaussianBlur path (opencv_contrib 4.5.2,
                       cudaoptflow/src/farneback.cpp and cuda/farneback.cu: gaussianBlur5) restated from memory of those
                       files, rated MED like SURVEY.md's Appendix B items: a separable weighted sum of the five planes of
                       M, vertical pass first, replicate borders, in orc_farneback_gaussian_blur's operation order and
                       with no 1 / area factor.  Products and sums are separate float32 array operations: nothing contracts.
"""
import ctypes as C

import numpy as np

MIN_SIZE = 32  # upstream MIN_SIZE (oracle/farneback_oracle.c)


class PolyConsts(C.Structure):  # orc_farneback_poly_consts
    _fields_ = [("g", C.c_float * 8), ("xg", C.c_float * 8), ("xxg", C.c_float * 8),
                ("ig11", C.c_float), ("ig03", C.c_float), ("ig33", C.c_float), ("ig55", C.c_float)]


def _p(a):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(C.c_void_p)


def gaussian_kernel(oracle, ksize, sigma):
    """orc_farneback_gaussian_kernel: the ksize taps of cv::getGaussianKernel(ksize, sigma, CV_32F)."""
    k = np.empty(ksize, np.float32)
    rc = oracle.lib().orc_farneback_gaussian_kernel(C.c_int(ksize), C.c_double(sigma), _p(k))
    assert rc == 0, (ksize, sigma)
    return k


def window_taps(oracle, win_size):
    """The non-negative half of the Gaussian window's taps, centre first: sigma = (winSize / 2) * 0.3f — an integer
    division and a float product."""
    sigma = float(np.float32(win_size // 2) * np.float32(0.3))
    return gaussian_kernel(oracle, win_size, sigma)[win_size // 2:].copy()


def gauss5(M, w, h, taps):
    """M: (5, h, w) float32.  r = M[y][x] * g[0]; r = r + (M[clamp(y-j)][x] + M[clamp(y+j)][x]) * g[j], then the same along
    x on r.  Clamping by index arrays; every product and every sum is one float32 array operation."""
    assert M.shape == (5, h, w) and M.dtype == np.float32
    g = np.asarray(taps, np.float32)
    half = len(g) - 1
    ys, xs = np.arange(h), np.arange(w)
    r = M * g[0]
    for j in range(1, half + 1):
        pair = M[:, np.clip(ys - j, 0, h - 1), :] + M[:, np.clip(ys + j, 0, h - 1), :]
        r = r + pair * g[j]
    out = r * g[0]
    for i in range(1, half + 1):
        pair = r[:, :, np.clip(xs - i, 0, w - 1)] + r[:, :, np.clip(xs + i, 0, w - 1)]
        out = out + pair * g[i]
    assert out.dtype == np.float32
    return out


def _box5(oracle, M, w, h, half):
    out = np.empty_like(M)
    oracle.lib().orc_farneback_box_filter5(_p(M), C.c_int(w), C.c_int(h), C.c_int(half), _p(out))
    return out


def farneback_flow(oracle, frame0, frame1, params=None, window="box"):
    """orc_farneback_calc's loop over the oracle's stage functions.  params: oracle.FarnebackParams (flags stay 0: the
    window is this function's argument).  Returns the (H, W, 2) float32 flow."""
    assert window in ("box", "gaussian")
    L = oracle.lib()
    p = params if params is not None else oracle.farneback_default_params()
    f0 = np.ascontiguousarray(frame0, dtype=np.uint8)
    f1 = np.ascontiguousarray(frame1, dtype=np.uint8)
    assert f0.shape == f1.shape and f0.ndim == 2
    H, W = f0.shape
    assert p.poly_n in (5, 7) and not p.fast_pyramids and p.flags == 0 and p.win_size >= 1 and p.win_size & 1
    oracle._pick_threads(H, W, None)
    frames = [f0.astype(np.float32), f1.astype(np.float32)]  # convertTo(CV_32F), alpha = 1: exact

    scale, cropped = 1.0, 0
    while cropped < p.num_levels:
        scale *= p.pyr_scale
        if W * scale < MIN_SIZE or H * scale < MIN_SIZE:
            break
        cropped += 1

    pc = PolyConsts()
    L.orc_farneback_prepare_poly(C.c_int(p.poly_n), C.c_double(p.poly_sigma), C.byref(pc))
    half_win = p.win_size // 2
    taps = window_taps(oracle, p.win_size) if window == "gaussian" else None
    inv = lambda dst, src: float(np.float32(1.0 / (float(dst) / float(src))))  # orc_inv_scale_from_sizes

    prev = None  # (flow x, flow y, width, height) of the coarser level
    for k in range(cropped, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= p.pyr_scale
        sigma = (1.0 / scale - 1) * 0.5
        smooth = max(int(np.rint(sigma * 5)) | 1, 3)
        w, h = int(np.rint(W * scale)), int(np.rint(H * scale))
        if prev is None:
            curx, cury = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        else:
            px, py, pw, ph = prev
            up = np.float32(1.0 / p.pyr_scale)
            curx = oracle.resize_linear(px, w, h, inv(w, pw), inv(h, ph)) * up
            cury = oracle.resize_linear(py, w, h, inv(w, pw), inv(h, ph)) * up
        gk = gaussian_kernel(oracle, smooth, sigma)
        ker_half = np.ascontiguousarray(gk[smooth // 2:])
        R = []
        for f in frames:
            blurred = np.empty((H, W), np.float32)
            L.orc_farneback_gaussian_blur(_p(f), C.c_int(W), C.c_int(H), _p(ker_half), C.c_int(smooth // 2), _p(blurred))
            pyr = oracle.resize_linear(blurred, w, h, inv(w, W), inv(h, H))
            Rf = np.empty((5, h, w), np.float32)
            L.orc_farneback_poly_exp(_p(pyr), C.c_int(w), C.c_int(h), C.c_int(p.poly_n), C.byref(pc), _p(Rf))
            R.append(Rf)

        def update_matrices():
            M = np.empty((5, h, w), np.float32)
            L.orc_farneback_update_matrices(_p(curx), _p(cury), _p(R[0]), _p(R[1]), C.c_int(w), C.c_int(h), _p(M))
            return M

        curx, cury = np.ascontiguousarray(curx), np.ascontiguousarray(cury)
        M = update_matrices()
        for it in range(p.num_iters):
            M = np.ascontiguousarray(gauss5(M, w, h, taps)) if window == "gaussian" else _box5(oracle, M, w, h, half_win)
            L.orc_farneback_update_flow(_p(M), C.c_int(w), C.c_int(h), _p(curx), _p(cury))
            if it < p.num_iters - 1:
                M = update_matrices()
        prev = (curx, cury, w, h)
    return np.ascontiguousarray(np.stack([prev[0], prev[1]], axis=-1))
