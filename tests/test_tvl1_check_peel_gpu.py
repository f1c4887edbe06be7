"""The lean tile loop with the convergence check peeled off (denseflow_amd/csrc/tvl1_tile.h: TVL1_CHECK_PEEL — iterations
without a check run a primal half that has none of its terms; the iteration that checks branches, wave-uniformly, into a
second copy of the primal half that has them).

Bit identity, not tolerance: flows, the executed-iteration table and the number of evaluated convergence sums per level
of EVERY pair of a four-pair call, from impl 0 (the fused lean kernels) against impl 1 (k_tvl1_step_simple, which shares
none of that code) and against the CPU oracle.  The cases put the check everywhere it can fall inside a step:

  * tvl1_iterations 1, 2, 3, 4, 5, 9 with the default epsilon and fuse_k 1 .. 4: segment-final steps of 1, 2, 3 and 4
    iterations, ending on a check or on the loop bound; the head (two iterations) alone, cut short, and followed by steps;
  * epsilon 0: no check is ever due, every iteration takes the body without one;
  * a large epsilon: the first check (the oracle evaluates the error in every second iteration) passes, in the head;
  * one pair of identical frames beside three moving ones: its error is exactly 0 and it leaves at its first check while
    the others go on;
  * 200 x 104: interior tiles and all four borders at the finest level (4 x 5 step tiles); 72 x 40: border tiles only, a
    single tile column at the coarser levels;
  * the default warp-and-head route and DFX_VAR_TVL1_NO_HEAD (every iteration in the step kernel);
  * the three exact hypot readings (tvl1_math 0, 2, 3).

The switch is a build flag: there is no runtime-selectable off form to hold to the same outputs."""
import collections

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

SHAPES = {"200x104": (200, 104, 12), "72x40": (72, 40, 5)}
BIG_EPSILON = 1000.0  # the oracle compares the mean squared update with epsilon^2: any first sum passes
CASES = {
    "it1": {"tvl1_iterations": 1},
    "it2": {"tvl1_iterations": 2},
    "it3": {"tvl1_iterations": 3},
    "it4": {"tvl1_iterations": 4},
    "it5": {"tvl1_iterations": 5},
    "it9": {"tvl1_iterations": 9},
    "eps0": {"tvl1_iterations": 9, "tvl1_epsilon": 0.0},
    "eps_big": {"tvl1_epsilon": BIG_EPSILON},
}
READINGS = {0: "0", 2: "VAR_TVL1_SQRT_HYPOT", 3: "VAR_TVL1_LIBM_HYPOT"}
_cache = {}


def _frames(shape):
    """Five frames = four pairs: two moving pairs, one pair of identical frames, one moving pair."""
    if shape not in _cache:
        w, h, seed = SHAPES[shape]
        clip = SynthClip(w, h, seed)
        fr = [clip.frame(0).copy(), clip.frame(1).copy(), clip.frame(2).copy(), clip.frame(2).copy(), clip.frame(4).copy()]
        for f in fr:
            f.setflags(write=False)
        _cache[shape] = fr
    return _cache[shape]


def _bits(flow):
    return np.ascontiguousarray(flow, np.float32).view(np.uint32)


def _table(rows, levels):
    rows = [list(r) for r in rows[:levels]]
    return rows + [[0] * len(rows[0])] * (levels - len(rows))


class _Ref:
    """The oracle's flow, iteration table and checks per level of one pair."""

    def __init__(self, flow, tr):
        flow.setflags(write=False)
        self.flow, self.levels, self.table = flow, tr.nscales, tr.iters_table()
        by_level = collections.Counter(c[0] for c in tr.checks())
        assert tr.n_checks == sum(by_level.values()), "the oracle's check trace overflowed"
        self.checks = [by_level.get(s, 0) for s in range(tr.nscales)]


def _run(dfx, shape, kw):
    w, h, _ = SHAPES[shape]
    with dfx.FlowEngine(w, h, "tvl1", max_batch=4, **kw) as eng:
        flows = eng.calc_optflows(_frames(shape), 1)
        st = eng.stats()
        tables, checks = eng.tvl1_batch_tables()
    assert st.batch == 4 and len(flows) == 4 and len(tables) == 4 and len(checks) == 4
    return flows, tables, checks


def _reference(dfx, oracle, shape, case, math=0):
    """Oracle and impl 1, once per (shape, case, reading); shared by every fuse_k and launch structure."""
    key = (shape, case, math)
    if key not in _cache:
        fr = _frames(shape)
        flag = READINGS[math]
        with oracle.variant(0 if flag == "0" else getattr(oracle, flag)):
            p = oracle.tvl1_default_params()
            if "tvl1_iterations" in CASES[case]:
                p.iterations = CASES[case]["tvl1_iterations"]
            if "tvl1_epsilon" in CASES[case]:
                p.epsilon = CASES[case]["tvl1_epsilon"]
            refs = [_Ref(*oracle.tvl1_calc(fr[i], fr[i + 1], p, want_trace=True)) for i in range(4)]
        kw = dict(CASES[case], impl=1, **({"tvl1_math": math} if math else {}))
        simple = _run(dfx, shape, kw)
        for f in simple[0]:
            f.setflags(write=False)
        _cache[key] = (refs, simple)
    return _cache[key]


def _hold(out, refs, simple, what):
    flows, tables, checks = out
    s_flows, s_tables, s_checks = simple
    for i in range(4):
        r = refs[i]
        levels = max(len(tables[i]), r.levels)
        t = _table(tables[i], levels)
        c = list(checks[i]) + [0] * (levels - len(checks[i]))
        print(f"{what} pair {i}: iterations {[row[:5] for row in t]} checks {c}")
        assert t == _table(s_tables[i], levels), f"{what}: pair {i}: iteration table differs from impl 1"
        assert t == _table(r.table, levels), f"{what}: pair {i}: iteration table differs from the oracle"
        assert c == list(s_checks[i]) + [0] * (levels - len(s_checks[i])), f"{what}: pair {i}: checks differ from impl 1"
        assert c == r.checks + [0] * (levels - r.levels), f"{what}: pair {i}: checks differ from the oracle"
        assert np.array_equal(_bits(flows[i]), _bits(s_flows[i])), f"{what}: pair {i}: flow differs from impl 1"
        assert np.array_equal(_bits(flows[i]), _bits(r.flow)), f"{what}: pair {i}: flow differs from the oracle"


def _structures():
    from denseflow_amd import engine as E

    return {"head": 0, "no_head": E.VAR_TVL1_NO_HEAD}


def test_the_cases_are_what_they_claim(dfx, oracle):
    """On the oracle alone (the error is evaluated in every second iteration, so a first check that passes ends a loop
    after two): the identical pair leaves every loop at its first check with a zero flow, a moving pair does not; without
    epsilon nothing is checked; with the large one every pair stops at its first check."""
    for shape in SHAPES:
        refs = _reference(dfx, oracle, shape, "it9")[0]
        assert not refs[2].flow.any() and all(set(r[:5]) == {2} for r in refs[2].table[:refs[2].levels])
        assert sum(refs[2].checks) == 5 * refs[2].levels
        assert any(9 in r[:5] for r in refs[0].table) and float(np.abs(refs[0].flow).max()) > 0.1
        refs = _reference(dfx, oracle, shape, "eps0")[0]
        assert all(sum(r.checks) == 0 and all(set(row[:5]) == {9} for row in r.table[:r.levels]) for r in refs)
        refs = _reference(dfx, oracle, shape, "eps_big")[0]
        assert all(all(set(row[:5]) == {2} for row in r.table[:r.levels]) and sum(r.checks) == 5 * r.levels for r in refs)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_lean_kernels_equal_the_simple_kernel_and_the_oracle(dfx, oracle, shape, case):
    refs, simple = _reference(dfx, oracle, shape, case)
    for name, variant in _structures().items():
        for k in (1, 2, 3, 4):
            out = _run(dfx, shape, dict(CASES[case], tvl1_fuse_k=k, variant=variant))
            _hold(out, refs, simple, f"{shape} {case} {name} fuse_k={k}")


@pytest.mark.parametrize("math,shape,case", [(0, "200x104", "it9"), (2, "200x104", "it5"), (3, "72x40", "it9"),
                                             (2, "72x40", "eps0"), (3, "200x104", "it3")])
def test_the_hypot_readings(dfx, oracle, math, shape, case):
    refs, simple = _reference(dfx, oracle, shape, case, math)
    kw = dict(CASES[case], **({"tvl1_math": math} if math else {}))
    for name, variant in _structures().items():
        out = _run(dfx, shape, dict(kw, variant=variant))
        _hold(out, refs, simple, f"{shape} {case} tvl1_math={math} {name}")
