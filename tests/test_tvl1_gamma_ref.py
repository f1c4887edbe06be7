"""The reference of dfx_params.tvl1_gamma (tests/tvl1_gamma_ref.py) and the plan of a gamma handle, without a GPU.

1. With gamma = 0 the three-channel restatement IS oracle.tvl1_calc, bit for bit (flow and iteration table), and u3 stays 0:
   the definition degenerates correctly, so the reference cannot drift from the oracle unnoticed.
2. Discrimination, on reference output only: gamma 0.4 and 2.0 each move the flow by more than 1e-3 px (max-abs) away from
   the gamma = 0 flow at every size the GPU tests use, so a kernel that ignored gamma could not pass them by accident.
3. What the channel is for: on a pair whose second frame is 20 grey levels brighter, gamma = 2.0 brings the mean flow error
   against the clean pair's flow below a quarter of the gamma = 0 error, and gamma * u3 settles at the brightness step.
4. The plan boundary (engine_plan.h's tvl1_plan, compiled into a small harness): 22 planes and the 88-byte rule with gamma,
   16 planes and the 64-byte rule without."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import tvl1_gamma_ref as GR

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = {(97, 61): 9, (130, 97): 5, (65, 17): 4}  # (w, h) -> SynthClip seed
DISCRIMINATION = 1e-3  # px

_cache = {}


def _pair(w, h):
    return SynthClip(w, h, SIZES[(w, h)]).frames(2)


def _ref(w, h, gamma):
    if (w, h, gamma) not in _cache:
        f0, f1 = _pair(w, h)
        _cache[(w, h, gamma)] = GR.tvl1_gamma_calc(f0, f1, gamma)
    return _cache[(w, h, gamma)]


@pytest.mark.parametrize("w,h", list(SIZES))
def test_gamma_zero_is_the_oracle(oracle, w, h):
    f0, f1 = _pair(w, h)
    want, tr = oracle.tvl1_calc(f0, f1, want_trace=True)
    flow, u3, table, checks = _ref(w, h, 0.0)
    assert np.array_equal(flow, want), np.max(np.abs(flow - want))
    assert not u3.any() and not np.signbit(u3).any()
    assert table == [r[:5] for r in tr.iters_table()]
    assert checks == tr.n_checks


@pytest.mark.parametrize("gamma", [0.4, 2.0])
@pytest.mark.parametrize("w,h", list(SIZES))
def test_gamma_moves_the_reference_flow(w, h, gamma):
    base, moved = _ref(w, h, 0.0)[0], _ref(w, h, gamma)
    d = float(np.max(np.abs(moved[0] - base)))
    print(f"gamma {gamma} {w}x{h}: max-abs against gamma 0 {d:.4g} px, max |gamma*u3| {float(np.max(np.abs(gamma * moved[1]))):.4g}")
    assert np.isfinite(moved[0]).all() and np.isfinite(moved[1]).all()
    assert d > DISCRIMINATION


def test_gamma_absorbs_a_brightness_step():
    w, h = 97, 61
    f0, f1 = _pair(w, h)
    bright = np.clip(f1.astype(np.int32) + 20, 0, 255).astype(np.uint8)
    clean = _ref(w, h, 0.0)[0]
    err = {}
    for gamma in (0.0, 2.0):
        flow, u3, table, _ = GR.tvl1_gamma_calc(f0, bright, gamma)
        err[gamma] = float(np.mean(np.abs(flow - clean)))
        print(f"+20 grey levels, gamma {gamma}: mean flow error {err[gamma]:.4g} px, {sum(map(sum, table))} inner iterations, "
              f"mean gamma*u3 {float(np.mean(gamma * u3)):.4g}")
    assert err[2.0] < 0.25 * err[0.0], err
    assert abs(float(np.mean(np.float32(2.0) * u3)) + 20.0) < 1.0


@pytest.fixture(scope="module")
def gp():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libtvl1_gamma_plan_harness.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "tvl1_gamma_plan_harness.cpp")],
                   check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    L.gp_tvl1.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_longlong)]
    L.gp_tvl1.restype = None

    def plan(w, h, gamma):
        out = (C.c_longlong * 5)()
        L.gp_tvl1(w, h, gamma, out)
        return dict(n_planes=out[0], plane_stride=out[1], slot_stride=out[2], too_large=bool(out[3]), per_pair=out[4])

    return plan


def test_plan_boundary_follows_the_plane_count(gp):
    for gamma in (0.4, -2.0):
        fits, over = gp(8192, 5957, gamma), gp(8192, 5958, gamma)
        assert fits["n_planes"] == over["n_planes"] == 22
        assert not fits["too_large"] and over["too_large"]
        assert fits["slot_stride"] * 4 == 8192 * 5957 * 88 < 2 ** 32 <= over["slot_stride"] * 4
    for gamma in (0.0, -0.0):  # either sign of zero is the 16-plane path
        assert gp(8192, 5958, gamma) == gp(8192, 5958, 0.0) and gp(8192, 5958, gamma)["n_planes"] == 16
        assert not gp(8192, 8191, gamma)["too_large"] and gp(8192, 8192, gamma)["too_large"]
    small, small_g = gp(130, 97, 0.0), gp(130, 97, 0.4)
    assert small_g["plane_stride"] == small["plane_stride"] and small_g["slot_stride"] * 16 == small["slot_stride"] * 22
    assert small_g["per_pair"] - small["per_pair"] == 6 * 4 * small["plane_stride"]
