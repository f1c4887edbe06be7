"""The reference of -a=farn with fast pyramids (tests/farneback_fastpyr_ref.py), the engine's level rule and the ABI of
dfx_params.farn_fast_pyramids, without a GPU: the composed driver with fast=False is oracle.farneback_calc bit for bit, so
the fast reference the GPU tests compare against differs from the oracle in the pyramids alone; pyr_down and pyr_up are held
to a float64 evaluation of their definitions within the float32 rounding of their sums; the fast flows are a different
result of comparable accuracy; farn_plan accepts and refuses the sizes SURVEY.md B.13 lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import farneback_fastpyr_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# (w, h, winSize, numIters, numLevels, seed): the shapes of tests/test_farneback_window_ref.py
BOX_CASES = [(129, 49, 13, 3, 5, 14), (70, 200, 7, 2, 2, 12), (65, 43, 21, 2, 2, 15), (33, 40, 31, 1, 5, 2),
             (65, 43, 1, 2, 2, 15)]
SHAPES = [(33, 47), (64, 40)]  # (h, w): odd and even


def _params(oracle, win, iters, levels):
    p = oracle.farneback_default_params()
    p.win_size, p.num_iters, p.num_levels = win, iters, levels
    return p


@pytest.mark.parametrize("w,h,win,iters,levels,seed", BOX_CASES)
def test_composed_driver_with_default_pyramids_is_the_oracle(oracle, w, h, win, iters, levels, seed):
    f0, f1 = SynthClip(w, h, seed).frames(2)
    p = _params(oracle, win, iters, levels)
    assert np.array_equal(FR.farneback_flow(oracle, f0, f1, p, fast=False), oracle.farneback_calc(f0, f1, p))


# ------------------------------------------------------------------------------------------------ the two filters

def _reflect(i, n):
    i = np.abs(i) % (2 * (n - 1))
    return np.where(i > n - 1, 2 * (n - 1) - i, i)


def _down64(s):
    c = np.array(FR.TAPS, np.float64)
    h, w = s.shape
    ys, xs = 2 * np.arange((h + 1) // 2), 2 * np.arange((w + 1) // 2)
    v = sum(c[j] * s[_reflect(ys - 2 + j, h), :] for j in range(5))
    return sum(c[j] * v[:, _reflect(xs - 2 + j, w)] for j in range(5))


def _up64_axis0(s):
    c = np.array(FR.TAPS, np.float64)
    n = s.shape[0]
    a = np.arange(n)
    lo, hi = np.minimum(np.abs(a - 1), n - 1), np.minimum(a + 1, n - 1)
    out = np.empty((2 * n,) + s.shape[1:])
    out[0::2] = c[0] * s[lo] + c[2] * s + c[4] * s[hi]
    out[1::2] = c[1] * s + c[3] * s[hi]
    return out


@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_down_against_a_float64_evaluation(h, w):
    """Bound: 2 passes * 9 roundings * 2^-24 * max|input|.  Derived, not tuned: a pass is five products and four sums, nine
    float32 roundings; the taps are positive and sum to 1, so every product and every partial sum is at most max|input| in
    magnitude and each rounding at most 2^-24 of that; the second pass carries the first one's error with weights that sum
    to 1 and adds nine roundings of its own.  (The products by dyadic taps are in fact exact: the bound counts them anyway.)"""
    src = (np.random.default_rng(h * 100 + w).standard_normal((h, w)) * 100).astype(F)
    got = FR.pyr_down(src)
    assert got.shape == ((h + 1) // 2, (w + 1) // 2) and got.dtype == F
    bound = 2 * 9 * 2.0 ** -24 * float(np.abs(src).max())
    err = float(np.max(np.abs(got.astype(np.float64) - _down64(src.astype(np.float64)))))
    print(f"pyr_down {h}x{w}: max-abs {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("h,w", SHAPES)
def test_pyr_up_against_a_float64_evaluation(h, w):
    """Bound: 4 * 2 passes * 5 roundings * 2^-24 * max|input|.  Derived, not tuned: the even phase of a pass is three
    products and two sums, five float32 roundings (the odd phase three), each of a magnitude at most max|input| (a phase's
    taps sum to 1/2); the second pass carries the first one's error with weights that sum to 1/2 and adds five roundings of
    its own; the final product by 4 is exact and scales the error by 4."""
    src = (np.random.default_rng(h * 100 + w + 1).standard_normal((h, w)) * 100).astype(F)
    got = FR.pyr_up(src)
    assert got.shape == (2 * h, 2 * w) and got.dtype == F
    want = 4.0 * _up64_axis0(_up64_axis0(src.astype(np.float64).T).T)
    bound = 4 * 2 * 5 * 2.0 ** -24 * float(np.abs(src).max())
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"pyr_up {h}x{w}: max-abs {err:.3g}, bound {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("h,w", SHAPES)
def test_a_constant_plane_comes_back_exactly(h, w):
    """The taps are dyadic and sum to 1 (pyr_down), and to 1/2 per phase and pass, times 4 (pyr_up): no rounding at all."""
    src = np.full((h, w), 93.0, F)
    assert np.array_equal(FR.pyr_down(src), np.full(((h + 1) // 2, (w + 1) // 2), 93.0, F))
    assert np.array_equal(FR.pyr_up(src), np.full((2 * h, 2 * w), 93.0, F))


# ------------------------------------------------------------------------------------------------ the flows

def _epe(flow, truth, margin=8):
    d = (flow.astype(np.float64) - truth)[margin:-margin, margin:-margin]
    return float(np.mean(np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)))


@pytest.mark.parametrize("t1", [1, 6])
@pytest.mark.parametrize("w,h", [(224, 224), (640, 384)])
def test_fast_flows_are_another_result_of_comparable_accuracy(oracle, w, h, t1):
    """On a prototype of this reference the fast path's end-point error was at most the default path's in every case
    measured (ratios 0.69 .. 1.00); the quarter is room for other seeds, not a tuned number."""
    clip = SynthClip(w, h, 9)
    f0, f1 = clip.frame(0), clip.frame(t1)
    truth = clip.true_flow(0, t1)
    fast = FR.farneback_flow(oracle, f0, f1, None, fast=True)
    default = FR.farneback_flow(oracle, f0, f1, None, fast=False)
    assert np.isfinite(fast).all()
    diff = float(np.max(np.abs(fast - default)))
    e_fast, e_def = _epe(fast, truth), _epe(default, truth)
    print(f"{w}x{h} 0->{t1}: fast against default max-abs {diff:.3f}, EPE fast {e_fast:.4f}, default {e_def:.4f}")
    assert diff > 0.05
    assert e_fast <= 1.25 * e_def


def test_a_seed_enters_the_fast_path_at_the_coarsest_level_only(oracle):
    clip = SynthClip(132, 140, 3)
    f0, f1 = clip.frame(0), clip.frame(6)
    p = _params(oracle, 13, 2, 2)
    seed = clip.true_flow(0, 6).astype(F)
    plain, seeded = FR.farneback_flow(oracle, f0, f1, p, fast=True), FR.farneback_flow(oracle, f0, f1, p, fast=True, seed=seed)
    assert np.isfinite(seeded).all() and not np.array_equal(plain, seeded)
    zero = FR.farneback_flow(oracle, f0, f1, p, fast=True, seed=np.zeros_like(seed))
    assert np.array_equal(zero, plain)


# ------------------------------------------------------------------------------------------------ the level rule

@pytest.fixture(scope="module")
def plan():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libfarn_fastpyr_plan.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so,
                    os.path.join(ROOT, "tests", "farn_fastpyr_plan_harness.cpp")], check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)

    def run(w, h, levels, fast=1):
        nlev, mx, nt = C.c_int(), C.c_int(), C.c_int()
        ws, hs = (C.c_int * 16)(), (C.c_int * 16)()
        odd = L.ffp_plan(w, h, levels, fast, C.byref(nlev), ws, hs, C.byref(mx), C.byref(nt))
        return dict(odd=bool(odd), sizes=[(ws[k], hs[k]) for k in range(nlev.value)], max_levels=mx.value, taps=nt.value)

    return run


ACCEPTED = [(224, 224, 5), (1280, 720, 5), (1920, 1080, 3), (1920, 1080, 2), (3840, 2160, 4), (97, 61, 0), (1921, 1081, 0),
            (66, 64, 1), (132, 140, 2), (520, 72, 1), (72, 520, 1), (256, 256, 3), (1088, 72, 1), (224, 160, 5), (256, 128, 2)]
REFUSED = [(1920, 1080, 5, 3), (340, 256, 5, 2), (130, 132, 2, 1), (3840, 2160, 5, 4)]  # ..., the level count it accepts


@pytest.mark.parametrize("w,h,levels", ACCEPTED)
def test_level_rule_accepts(plan, w, h, levels):
    r = plan(w, h, levels)
    assert not r["odd"], r
    cropped = FR.crop_levels(w, h, levels, 0.5)
    assert r["sizes"] == FR.fast_level_sizes(w, h, cropped)
    assert r["taps"] == 0  # no Gaussian pre-blur


@pytest.mark.parametrize("w,h,levels,accepts", REFUSED)
def test_level_rule_refuses_and_names_the_level_count_it_accepts(plan, w, h, levels, accepts):
    r = plan(w, h, levels)
    assert r["odd"] and r["max_levels"] == accepts, r
    assert FR.fast_level_sizes(w, h, FR.crop_levels(w, h, levels, 0.5)) is None
    assert not plan(w, h, accepts)["odd"]


def test_level_sizes_follow_the_pyramid_not_the_rounded_scale(plan):
    assert plan(132, 140, 2)["sizes"] == [(132, 140), (66, 70), (33, 35)]
    assert plan(66, 64, 1)["sizes"] == [(66, 64), (33, 32)]
    assert plan(1920, 1080, 5)["sizes"][3] == (240, 135)  # the odd level 3 of 5
    # the coarsest level may be odd; below an odd level the chain is not cvRound(W * scale): 66 -> 33 -> 17, against rint(16.5) = 16
    assert plan(130, 134, 1)["sizes"] == [(130, 134), (65, 67)]
    assert plan(66, 64, 1, fast=0)["sizes"] == [(66, 64), (33, 32)]


def test_the_flag_at_zero_leaves_the_plan_alone(plan):
    r = plan(1920, 1080, 5, fast=0)
    assert not r["odd"] and r["taps"] > 0 and r["sizes"] == [(1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68),
                                                              (60, 34)]


# ------------------------------------------------------------------------------------------------ ABI

def _header():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_fields():
    body = re.search(r"typedef struct \{(.*?)\}\s*dfx_params;", _header()[1], flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip() for n in re.sub(r"^(double|float|int)\s+", "", decl).split(",")]
    return fields


def test_header_has_the_field_last_and_the_version():
    fields = _header_fields()
    assert fields[-1] == "farn_fast_pyramids" and fields[-2] == "tvl1_gamma"
    assert re.search(r"int\s+farn_fast_pyramids\s*;", _header()[1])
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", _header()[1]).group(1)) >= 420


def test_header_comment_documents_the_option_and_its_refusals():
    src = re.sub(r"\s*\n\s*\*\s*", " ", _header()[0])  # comment lines joined
    assert "farn_fast_pyramids" in src and "upstream's fastPyramids" in src
    assert "farn_pyr_scale != 0.5 is DFX_ERR_INVALID" in src
    assert "odd width or height is DFX_ERR_UNSUPPORTED" in src
    assert "restated from memory, MED, unpinned" in src
    assert "no fastPyramids" not in src


def test_binding_has_the_fields_in_the_headers_order():
    from denseflow_amd import engine as E

    assert [f[0] for f in E.DfxParams._fields_] == _header_fields()
    assert dict(E.DfxParams._fields_)["farn_fast_pyramids"] is C.c_int


def test_default_params_leave_fast_pyramids_off(dfx):
    assert dfx.engine.default_params().farn_fast_pyramids == 0
