"""The reference of the Farneback update window (tests/farneback_window_ref.py) and the ABI of dfx_params.farn_window, without
a GPU: the composed driver with the box step is oracle.farneback_calc bit for bit, so the Gaussian reference the GPU tests
compare against differs from the oracle in the window step alone; gauss5 is held to a float64 convolution within the float32
rounding of its sums; the taps are a normalised symmetric kernel."""
import os
import re

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import farneback_window_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (w, h, winSize, numIters, numLevels, seed)
BOX_CASES = [(129, 49, 13, 3, 5, 14), (70, 200, 7, 2, 2, 12), (65, 43, 21, 2, 2, 15), (33, 40, 31, 1, 5, 2),
             (65, 43, 1, 2, 2, 15)]


def _params(oracle, win, iters, levels):
    p = oracle.farneback_default_params()
    p.win_size, p.num_iters, p.num_levels = win, iters, levels
    return p


@pytest.mark.parametrize("w,h,win,iters,levels,seed", BOX_CASES)
def test_composed_driver_with_the_box_step_is_the_oracle(oracle, w, h, win, iters, levels, seed):
    f0, f1 = SynthClip(w, h, seed).frames(2)
    p = _params(oracle, win, iters, levels)
    assert np.array_equal(WR.farneback_flow(oracle, f0, f1, p, "box"), oracle.farneback_calc(f0, f1, p))


def test_gaussian_window_1_is_the_box_window_1(oracle):
    f0, f1 = SynthClip(65, 43, 15).frames(2)
    p = _params(oracle, 1, 2, 2)
    assert np.array_equal(WR.window_taps(oracle, 1), np.ones(1, np.float32))
    assert np.array_equal(WR.farneback_flow(oracle, f0, f1, p, "gaussian"), WR.farneback_flow(oracle, f0, f1, p, "box"))


def test_gaussian_window_13_is_not_the_box_window(oracle):
    f0, f1 = SynthClip(129, 49, 14).frames(2)
    p = _params(oracle, 13, 3, 5)
    g, b = WR.farneback_flow(oracle, f0, f1, p, "gaussian"), WR.farneback_flow(oracle, f0, f1, p, "box")
    assert np.isfinite(g).all()
    assert float(np.max(np.abs(g - b))) > 0.1


@pytest.mark.parametrize("half", [1, 6, 15])
def test_gauss5_against_a_float64_convolution(oracle, half):
    """Bound: the float32 rounding of the sums, (2 * half + 2) * 2^-24 * sum|taps| * max|M| per pass, two passes.  Derived, not
    tuned: a pass is a centre product, then per symmetric pair one sum, one product and one accumulation — each rounding at
    most 2^-24 of a magnitude that sum|taps| * max|M| bounds (the pair sums carry twice the input, weighted by taps that sum
    to half of sum|taps|) — which comes to about (half + 3) such roundings, fewer than the 2 * half + 2 the bound counts."""
    rng = np.random.default_rng(half)
    h, w = 37, 29
    M = rng.standard_normal((5, h, w)).astype(np.float32)
    taps = WR.window_taps(oracle, 2 * half + 1)
    assert len(taps) == half + 1
    got = WR.gauss5(M, w, h, taps)
    full = np.concatenate([taps[:0:-1], taps]).astype(np.float64)
    P = np.pad(M.astype(np.float64), ((0, 0), (half, half), (0, 0)), mode="edge")
    r = sum(full[k] * P[:, k:k + h, :] for k in range(2 * half + 1))
    P = np.pad(r, ((0, 0), (0, 0), (half, half)), mode="edge")
    want = sum(full[k] * P[:, :, k:k + w] for k in range(2 * half + 1))
    s = float(np.abs(full).sum())
    per_pass = (2 * half + 2) * 2.0 ** -24 * s * float(np.abs(M).max())
    bound = 2 * per_pass
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"half {half}: max-abs {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_taps_are_symmetric_positive_and_sum_to_one(oracle):
    for win in range(1, 32, 2):
        sigma = float(np.float32(win // 2) * np.float32(0.3))
        k = WR.gaussian_kernel(oracle, win, sigma)
        assert k.dtype == np.float32 and len(k) == win
        assert np.array_equal(k, k[::-1]), win
        assert (k > 0).all(), win
        assert abs(float(k.astype(np.float64).sum()) - 1.0) <= win * 2.0 ** -24, win
        assert np.array_equal(WR.window_taps(oracle, win), k[win // 2:])


# ------------------------------------------------------------------------------------------------ ABI

def _header():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_defines_the_window_constants_and_the_version():
    _, code = _header()
    assert re.search(r"#define\s+DFX_FARN_WINDOW_BOX\s+0\b", code)
    assert re.search(r"#define\s+DFX_FARN_WINDOW_GAUSSIAN\s+1\b", code)
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", code).group(1)) >= 390


def test_header_comment_names_the_upstream_flag_and_the_refusal():
    src = re.sub(r"\s*\n\s*\*\s*", " ", _header()[0])  # comment lines joined
    assert "farn_window is how upstream's OPTFLOW_FARNEBACK_GAUSSIAN is requested" in src
    assert "farn_flags = 256 is still refused" in src


def test_binding_has_farn_window_where_the_header_has_it():
    from denseflow_amd import engine as E

    _, code = _header()
    body = re.search(r"typedef struct \{(.*?)\}\s*dfx_params;", code, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names = re.sub(r"^(double|float|int)\s+", "", decl)
            fields += [n.strip() for n in names.split(",")]
    assert fields == [f[0] for f in E.DfxParams._fields_]
    i = fields.index("farn_window")
    assert fields[i - 1] == "farn_flags" and fields[i + 1] == "brox_alpha"
    assert (E.FARN_WINDOW_BOX, E.FARN_WINDOW_GAUSSIAN) == (0, 1)


def test_default_params_choose_the_box(dfx):
    assert dfx.engine.default_params().farn_window == 0


def test_engine_taps_are_the_oracles(oracle):
    """farn_window_taps, the host function the engine hands to its kernels, compiled as it stands: the oracle's taps for every
    accepted window, zeros behind them, and a refusal past the 16 entries the kernels take."""
    import ctypes as C
    import subprocess

    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libfarn_window_taps.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so,
                    os.path.join(ROOT, "tests", "farn_window_taps_harness.cpp")], check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    for win in range(1, 32, 2):
        got = np.full(16, -1, np.float32)
        assert L.fwt_window_taps(win, got.ctypes.data_as(C.c_void_p)) == 0
        want = WR.window_taps(oracle, win)
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), win
    assert L.fwt_window_taps(33, np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)) != 0
    assert L.fwt_window_taps(14, np.zeros(16, np.float32).ctypes.data_as(C.c_void_p)) != 0
