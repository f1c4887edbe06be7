"""tests/initial_flow_ref.py against the oracle (no GPU): an all-zero seed is the unseeded algorithm bit for bit, a
one-level pyramid uses the seed as it is, and a good seed buys what it is for — the figures of the README's TVL1 and
Farneback rows are printed here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import farneback_window_ref as WR
from tests import initial_flow_ref as IR

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {(97, 61): 9, (130, 97): 5}  # (w, h) -> SynthClip seed


def _pair(w, h, dt):
    c = SynthClip(w, h, SIZES[(w, h)])
    return c.frame(0), c.frame(dt), c.true_flow(0, dt).astype(F)


def _epe(flow, true):
    return float(np.mean(np.hypot(flow[..., 0] - true[..., 0], flow[..., 1] - true[..., 1])))


def _table(trace, warps=5):
    return [r[:warps] for r in trace.iters_table()]


@pytest.mark.parametrize("w,h", list(SIZES))
def test_tvl1_zero_seed_is_the_unseeded_oracle(oracle, w, h):
    f0, f1, _ = _pair(w, h, 6)
    want, tr = oracle.tvl1_calc(f0, f1, want_trace=True)
    for init in (None, np.zeros((h, w, 2), F)):
        flow, table, checks = IR.tvl1_init_calc(oracle, f0, f1, init)
        assert np.array_equal(flow, want)
        assert table == _table(tr) and checks == tr.n_checks


@pytest.mark.parametrize("w,h", list(SIZES))
@pytest.mark.parametrize("window", ["box", "gaussian"])
def test_farneback_zero_seed_is_the_unseeded_reference(oracle, w, h, window):
    f0, f1, _ = _pair(w, h, 6)
    want = oracle.farneback_calc(f0, f1) if window == "box" else WR.farneback_flow(oracle, f0, f1, window="gaussian")
    for init in (None, np.zeros((h, w, 2), F)):
        flow, _ = IR.farneback_init_calc(oracle, f0, f1, init, window=window)
        assert np.array_equal(flow, want)


def test_tvl1_one_level_uses_the_seed_as_it_is(oracle):
    w, h = 97, 61
    f0, f1, true = _pair(w, h, 6)
    flow, table, checks = IR.tvl1_init_calc(oracle, f0, f1, true, nscales=1)
    prm = oracle.tvl1_default_params()
    prm.nscales = 1
    u1, u2 = np.ascontiguousarray(true[..., 0]), np.ascontiguousarray(true[..., 1])
    trace = oracle.Tvl1Trace()
    oracle.lib().orc_tvl1_proc_one_scale(f0.astype(F), f1.astype(F), u1, u2, w, h, C.byref(prm), 0, C.byref(trace))
    assert np.array_equal(flow[..., 0], u1) and np.array_equal(flow[..., 1], u2)
    assert table == [[trace.iters[0][k] for k in range(5)]] and checks == trace.n_checks


def test_farneback_one_level_uses_the_seed_with_factor_one(oracle):
    """num_levels = 0: resize_linear to the seed's own size with ifx = ify = 1 and the factor (float)1.0 returns the seed, so
    the level starts from it — held by running the level's loop on the seed by hand."""
    w, h = 97, 61
    f0, f1, true = _pair(w, h, 6)
    p = oracle.farneback_default_params()
    p.num_levels = 0
    flow, levels = IR.farneback_init_calc(oracle, f0, f1, true, params=p)
    assert levels == 1
    L = oracle.lib()
    pc = WR.PolyConsts()
    L.orc_farneback_prepare_poly(C.c_int(p.poly_n), C.c_double(p.poly_sigma), C.byref(pc))
    R = []
    for f in (f0, f1):  # level 0 of a one-level pyramid: sigma = 0, smoothSize 3 — the driver's own preparation
        gk = WR.gaussian_kernel(oracle, 3, 0.0)
        blurred = np.empty((h, w), F)
        L.orc_farneback_gaussian_blur(WR._p(f.astype(F)), C.c_int(w), C.c_int(h), WR._p(np.ascontiguousarray(gk[1:])), C.c_int(1),
                                      WR._p(blurred))
        pyr = oracle.resize_linear(blurred, w, h, 1.0, 1.0)
        Rf = np.empty((5, h, w), F)
        L.orc_farneback_poly_exp(WR._p(pyr), C.c_int(w), C.c_int(h), C.c_int(p.poly_n), C.byref(pc), WR._p(Rf))
        R.append(Rf)
    curx, cury = np.ascontiguousarray(true[..., 0]), np.ascontiguousarray(true[..., 1])  # the seed, factor 1
    for it in range(p.num_iters):
        M = np.empty((5, h, w), F)
        L.orc_farneback_update_matrices(WR._p(curx), WR._p(cury), WR._p(R[0]), WR._p(R[1]), C.c_int(w), C.c_int(h), WR._p(M))
        M = WR._box5(oracle, M, w, h, p.win_size // 2)
        L.orc_farneback_update_flow(WR._p(M), C.c_int(w), C.c_int(h), WR._p(curx), WR._p(cury))
    assert np.array_equal(flow[..., 0], curx) and np.array_equal(flow[..., 1], cury)


def test_what_the_seed_is_for(oracle):
    """SynthClip(97, 61, 9), seed = true_flow.  Bounds 0.25 (measured ratios 0.11, 0.03 and 0.10)."""
    w, h = 97, 61
    f0, f6, true6 = _pair(w, h, 6)
    _, f1, true1 = _pair(w, h, 1)
    # TVL1, frames 0 -> 6 (about 10 px of motion), one level: the end-point error
    a, ta, _ = IR.tvl1_init_calc(oracle, f0, f6, None, nscales=1)
    b, tb, _ = IR.tvl1_init_calc(oracle, f0, f6, true6, nscales=1)
    print(f"TVL1 0->6 nscales=1: EPE unseeded {_epe(a, true6):.3f} px ({sum(map(sum, ta))} inner iterations), "
          f"seeded {_epe(b, true6):.3f} px ({sum(map(sum, tb))})")
    assert _epe(b, true6) < 0.25 * _epe(a, true6)
    # TVL1, adjacent frames, one level: the inner iterations, at the same accuracy
    a, ta, _ = IR.tvl1_init_calc(oracle, f0, f1, None, nscales=1)
    b, tb, _ = IR.tvl1_init_calc(oracle, f0, f1, true1, nscales=1)
    ia, ib = sum(map(sum, ta)), sum(map(sum, tb))
    print(f"TVL1 0->1 nscales=1: inner iterations unseeded {ia} (EPE {_epe(a, true1):.3f} px), seeded {ib} "
          f"(EPE {_epe(b, true1):.3f} px)")
    assert ib < 0.25 * ia
    a5, ta5, _ = IR.tvl1_init_calc(oracle, f0, f1, None)
    b5, tb5, _ = IR.tvl1_init_calc(oracle, f0, f1, true1)
    print(f"TVL1 0->1 nscales=5: inner iterations unseeded {sum(map(sum, ta5))}, seeded {sum(map(sum, tb5))}")
    # Farneback, frames 0 -> 6, one level
    p = oracle.farneback_default_params()
    p.num_levels = 0
    a, _ = IR.farneback_init_calc(oracle, f0, f6, None, params=p)
    b, _ = IR.farneback_init_calc(oracle, f0, f6, true6, params=p)
    print(f"Farneback 0->6 num_levels=0: EPE unseeded {_epe(a, true6):.3f} px, seeded {_epe(b, true6):.3f} px")
    assert _epe(b, true6) < 0.25 * _epe(a, true6)


def test_header_and_binding_declare_the_seeded_entry_points(dfx):
    """include/dfx.h declares the three entry points at DFX_VERSION >= 410, libdfx.so exports them and engine.py binds them
    with the header's arity."""
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 410
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = dfx.load_library()
    for name, arity in [("dfx_calc_batch_init", 9), ("dfx_calc_batch_init_device", 10),
                        ("dfx_calc_batch_planar_init_device", 12)]:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, f"include/dfx.h does not declare {name}"
        assert len(m.group(1).split(",")) == arity
        assert len(getattr(L, name).argtypes) == arity
    import inspect

    for fn in ("calc", "calc_optflows", "calc_optflows_device", "flow_tensor"):
        assert inspect.signature(getattr(dfx.FlowEngine, fn)).parameters["init"].default is None
