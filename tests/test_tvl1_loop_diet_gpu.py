"""The instruction reductions of the TVL1 tile function's inner loop (denseflow_amd/csrc/tvl1_math_pk.h, tvl1_tile.h), each
against the form it replaces, bit for bit:

  * pk_dual_denominator — 1 + taut * sqrt(s) without the square root's NaN guard and with its half reciprocal root
    unrefined — on EVERY float s of the domain [0, 2^63), for the taut of the default parameters and of the non-default
    tau / theta sets tests/ runs (test_tvl1_params_gpu.py: A, B), in both halves of a float2;
  * sub_right_minus_self (the dual's u_right - u as one DPP subtraction) and the assembly max / min that follows it,
    on one wave at a time;
  * the tile kernels themselves on a 200 x 104 pair whose content reaches each new path.

Every comparison is exact (uint32 views); where both sides are NaN any payload counts as equal, since a NaN's only
consumers are packed multiplications."""
import ctypes as C

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

# (tau, lambda, theta): the defaults and the sets A, B of tests/test_tvl1_params_gpu.py (F repeats A's three values)
PARAMS = {"default": (0.25, 0.15, 0.3), "A": (0.1, 0.05, 0.5), "B": (0.2, 0.4, 0.1)}


def _taut(name):  # tvl1_engine.cpp: kc.taut = (float)(tau / theta)
    tau, _, theta = PARAMS[name]
    return np.float32(tau / theta)


def _same(a, b):
    """Bit equality; two NaNs are equal whatever their payload."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def _first_bad(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    bad = np.flatnonzero(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


# ---- the denominator, exhaustive ---------------------------------------------------------------------------------------

# taut_s = taut * 2^-32 as the tile function forms it (exact).  The last two are not parameters but magnifiers: at
# taut_s = 2^70 the sum 1 + taut_s * g is taut_s * g exactly for every g below 2^57, at 2^-6 for every g from 2^31 up
# (g = sqrt(s) * 2^32 lies in [2^-42.5, 2^63.5)), so between them they compare the square root ITSELF on every s > 0 and
# the result holds for any taut.  They start at the first positive float: at s = 0 the new form's g is 2^-63 instead of 0,
# which 1 + taut_s * g hides only for taut below 2^70.
DENOMINATOR_CASES = [(n, float(_taut(n)) * 2.0 ** -32, 0) for n in PARAMS] + [("g_low", 2.0 ** 70, 1), ("g_high", 2.0 ** -6, 1)]


@pytest.mark.parametrize("name,taut_s,first", DENOMINATOR_CASES, ids=[c[0] for c in DENOMINATOR_CASES])
def test_dual_denominator_on_every_float_of_the_domain(dfx, name, taut_s, first):
    lib = dfx.load_library()
    fn = lib.dfxi_dual_denominator_exhaustive
    fn.argtypes = [C.c_int, C.c_uint, C.c_uint, C.c_float, C.POINTER(C.c_ulonglong)]
    fn.restype = C.c_int
    assert float(np.float32(taut_s)) == taut_s
    counts = (C.c_ulonglong * 3)()
    last = int(np.float32(2.0 ** 63).view(np.uint32)) - 1
    assert fn(0, first, last, taut_s, counts) == 0
    print(f"dual denominator {name}: mismatches packed / scalar positions {counts[0]} / {counts[1]}, first + 1 = {counts[2]:#x}")
    assert list(counts) == [0, 0, 0], (f"mismatches packed/scalar positions: {counts[0]}/{counts[1]}, "
                                       f"first at bits {counts[2] - 1:#x}")


# ---- the lane difference and the assembly max / min -----------------------------------------------------------------------

def _lane_probe(dfx, a, b):
    lib = dfx.load_library()
    fn = lib.dfxi_probe_lane_pieces
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    fn.restype = C.c_int
    inp = np.ascontiguousarray(np.stack([a, b]), np.float32)
    out = np.empty((10, a.size), np.float32)
    assert a.size % 64 == 0 and fn(0, inp.ctypes.data, out.ctypes.data, a.size) == 0
    return out


def test_lane_difference_and_max_min(dfx):
    """sub_right_minus_self against roll(u, -1) - u per wave of 64 lanes (lane 63: 0 - u), and pk_abs_max_min against
    fmaxf(fabsf) / fminf(fabsf) — the compiler's, from the same kernel, and numpy's: ordinary values, +-0, denormals, equal
    magnitudes of opposite sign, infinities, a quiet NaN in either place."""
    sub = np.float32(1e-45)
    vals = np.array([0.0, -0.0, 1.0, -1.0, 2.5, -2.5, sub, -sub, 3 * sub, 1.1754944e-38, -1e-39, 1e-20, 3e38, -3e38, np.inf,
                     -np.inf, np.nan, 0.1, 123456.0], np.float32)
    x, y = (g.ravel() for g in np.meshgrid(vals, vals))
    rng = np.random.default_rng(31)
    pad = (-x.size) % 64 + 64 * 8
    a = np.concatenate([x, (rng.standard_normal(pad) * rng.choice([1e-3, 1.0, 50.0], pad)).astype(np.float32)])
    b = np.concatenate([y, (rng.standard_normal(pad) * rng.choice([1e-3, 1.0, 50.0], pad)).astype(np.float32)])
    for a_, b_ in ((a, b), (a, np.roll(b, 7)), (np.roll(a, 1), b[::-1].copy())):  # other neighbours, other pairs
        out = _lane_probe(dfx, a_, b_)
        with np.errstate(all="ignore"):
            def right_minus_self(u):
                w = u.reshape(-1, 64)
                r = np.concatenate([w[:, 1:], np.zeros((w.shape[0], 1), np.float32)], axis=1)
                return (r - w).ravel()

            da, db = right_minus_self(a_), right_minus_self(b_)
            mx, mn = np.fmax(np.abs(a_), np.abs(b_)), np.fmin(np.abs(a_), np.abs(b_))
        for k, ref in ((0, da), (2, da), (1, db), (3, db)):
            assert _same(out[k], ref), ("difference", k, _first_bad(out[k], ref))
        for k in (4, 5):
            assert _same(out[k], out[8]) and _same(out[k], mx), ("max", k, _first_bad(out[k], out[8]))
        for k in (6, 7):
            assert _same(out[k], out[9]) and _same(out[k], mn), ("min", k, _first_bad(out[k], out[9]))


# ---- the tile kernels -----------------------------------------------------------------------------------------------------

W, H = 200, 104  # 4 x 5 step tiles, 4 x 4 head tiles: the smallest size with interior tiles in both kernels
_cache = {}


def _pair():
    """Moving texture; a 76 x 44 block that is constant and identical in both frames (grad = 0, s = 0, rgrad = 0); two blocks
    whose brightness jumps by +60 and by -60 grey levels between the frames (the saturated arms, both signs).  All three
    lie in the middle of the frame, across the interior tiles of both kernels."""
    if "pair" not in _cache:
        clip = SynthClip(W, H, 12)
        f0, f1 = clip.frame(0).copy(), clip.frame(1).copy()
        f0[22:66, 44:120] = 128
        f1[22:66, 44:120] = 128
        for ys, sign in ((slice(24, 60), 60), (slice(62, 96), -60)):
            base = np.clip(f0[ys, 126:172].astype(int), 70, 185)
            f0[ys, 126:172] = base
            f1[ys, 126:172] = base + sign
        f0.setflags(write=False)
        f1.setflags(write=False)
        _cache["pair"] = (f0, f1)
    return _cache["pair"]


def _iters(rows):
    return [r[:5] for r in rows]


def _bits(flow):
    return np.ascontiguousarray(flow, np.float32).view(np.uint32)


def _reference(dfx, oracle, math, nscales):
    """The oracle's flow and iteration table and the simple kernel's (impl = 1 keeps the guarded square root and
    plain subtractions), once per case."""
    key = (math, nscales)
    if key not in _cache:
        f0, f1 = _pair()
        flags = {0: 0, 2: oracle.VAR_TVL1_SQRT_HYPOT}[math]
        with oracle.variant(flags):
            p = oracle.tvl1_default_params()
            p.nscales = nscales
            ref, tr = oracle.tvl1_calc(f0, f1, p, want_trace=True)
        with dfx.FlowEngine(W, H, "tvl1", impl=1, tvl1_nscales=nscales, **({"tvl1_math": math} if math else {})) as eng:
            simple = eng.calc(f0, f1)
            simple_iters = _iters(eng.stats().iters_table())
        ref.setflags(write=False)
        simple.setflags(write=False)
        _cache[key] = (ref, _iters(tr.iters_table()), simple, simple_iters)
    return _cache[key]


def _variants():
    from denseflow_amd import engine as E

    return {"default": 0, "no_head": E.VAR_TVL1_NO_HEAD, "step_nbr_lds": E.VAR_TVL1_STEP_NBR_LDS}


def test_the_pair_reaches_the_new_paths(dfx, oracle):
    """On oracle output and the frames only: the constant block has no gradient, and the jump blocks keep their +-60."""
    f0, f1 = _pair()
    assert np.array_equal(f0[22:66, 44:120], f1[22:66, 44:120]) and np.ptp(f0[22:66, 44:120]) == 0
    assert f0[22:66, 44:120].shape[0] >= 40 and f0[22:66, 44:120].shape[1] >= 70
    assert np.all(f1[24:60, 126:172].astype(int) - f0[24:60, 126:172] == 60)
    assert np.all(f1[62:96, 126:172].astype(int) - f0[62:96, 126:172] == -60)
    ref = _reference(dfx, oracle, 0, 1)[0]
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) > 0.1


@pytest.mark.parametrize("variant", ["default", "no_head", "step_nbr_lds"])
@pytest.mark.parametrize("nscales", [1, 3])
@pytest.mark.parametrize("math", [0, 2])
def test_tile_kernels_equal_the_simple_kernel_and_the_oracle(dfx, oracle, math, nscales, variant):
    f0, f1 = _pair()
    ref, ref_iters, simple, simple_iters = _reference(dfx, oracle, math, nscales)
    with dfx.FlowEngine(W, H, "tvl1", tvl1_nscales=nscales, variant=_variants()[variant],
                        **({"tvl1_math": math} if math else {})) as eng:
        out = eng.calc(f0, f1)
        iters = _iters(eng.stats().iters_table())
    assert iters == simple_iters and iters == ref_iters
    assert np.array_equal(_bits(out), _bits(simple)), "impl 0 differs from impl 1"
    assert np.array_equal(_bits(out), _bits(ref)), "impl 0 differs from the oracle"
