"""-a=tvl1 away from the reference's float defaults: tau, lambda, theta and scale_step (with the level counts they lead
to) reach every kernel form, and the flows stay the oracle's bits.  The device arithmetic is the oracle's operation for
operation, so every comparison is np.array_equal against oracle.tvl1_calc with the same
parameters, together with the pyramid geometry, the executed inner-iteration table and the number of convergence checks.

Each parameter set has to move the oracle's own flow by more than 1e-3 px (max-abs) away from the default-parameter flow
on the same frames; the tests assert that on oracle output before the engine is touched, so a set that left the kernels
at their defaults could not pass by accident.

Shapes: 97x61 (a second 64-column tile of 33 columns, a height that is no multiple of 4 or 32), 130x97 (a third tile of two
columns), 65x17 (a second tile of one column, one level only), 65x33 (the same tile split with two levels).  Four frames with max_batch = 2 are three pairs in a full
and a ragged batch.  scale_step 0.5 is an exact 2x resize (bilinear weights 0 and 0.5), 0.95 with 8 scales keeps all 8
levels, 0.3 keeps two (the third falls below 16 px)."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

INVALID = 1
DISCRIMINATION = 1e-3  # px, max-abs between the oracle's flow under a set and under the defaults

# id -> oracle Tvl1Params fields; the engine takes the same values as tvl1_<name> (lambda_ -> tvl1_lambda)
SETS = {
    "A": dict(tau=0.1, lambda_=0.05, theta=0.5),
    "B": dict(tau=0.2, lambda_=0.4, theta=0.1),  # erratic flows of tens of pixels: wanted
    "C": dict(scale_step=0.5),
    "D": dict(scale_step=0.95, nscales=8),
    "E": dict(scale_step=0.3, nscales=4),
    "F": dict(tau=0.1, lambda_=0.05, theta=0.5, scale_step=0.6, nscales=6),
}
SIZES = {(97, 61): 9, (130, 97): 5, (65, 17): 4, (65, 33): 4, (65, 49): 7}  # (w, h) -> SynthClip seed
# 65x17 has one level whatever scale_step is (the second would be 8 or 14 rows), so set C cannot move the oracle's flow
# there: that case requires the oracle's flow to EQUAL the default-parameter flow instead, and 65x33 (a second tile of one
# column as well; 0.5 gives a second level of 32x16) is the size at which C has to discriminate.
SAME_AS_DEFAULTS = {("C", 65, 17)}
CASES = ([(s, 97, 61) for s in "ABCDEF"] + [(s, 130, 97) for s in "ABCDEF"] + [("A", 65, 17), ("C", 65, 17), ("C", 65, 33)])
FORMS = {"tuned": dict(), "impl1": dict(impl=1), "impl2": dict(impl=2)}

_clips, _refs = {}, {}


def _iters(rows):
    return [r[:5] for r in rows]


def _frames(w, h, n=4):
    if (w, h) not in _clips:
        _clips[(w, h)] = SynthClip(w, h, SIZES[(w, h)]).frames(n)
    return _clips[(w, h)]


def _engine_kw(name):
    return {"tvl1_" + k.rstrip("_"): v for k, v in SETS[name].items()}


class _Reading:
    """One reading of `hypotf` (tests/test_tvl1_gpu.py): dfx_params.tvl1_math and the oracle switch that gives its bits."""

    def __init__(self, oracle, math):
        self.math = math
        self._flags = {0: 0, 2: oracle.VAR_TVL1_SQRT_HYPOT, 3: oracle.VAR_TVL1_LIBM_HYPOT}[math]
        self._oracle = oracle

    def oracle(self):
        return self._oracle.variant(self._flags)

    def kw(self):
        return {"tvl1_math": self.math} if self.math else {}


def _ref(oracle, name, w, h, math=0):
    """The oracle's flows and traces of consecutive frames under set `name` (None: the defaults), computed once per case
    and never changed."""
    key = (name, w, h, math)
    if key not in _refs:
        frames = _frames(w, h)
        out = []
        with _Reading(oracle, math).oracle():
            for i in range(len(frames) - 1):
                p = oracle.tvl1_default_params()
                for k, v in (SETS[name] if name else {}).items():
                    setattr(p, k, v)
                flow, tr = oracle.tvl1_calc(frames[i], frames[i + 1], p, want_trace=True)
                flow.setflags(write=False)
                out.append((flow, tr))
        _refs[key] = out
    return _refs[key]


def _discriminates(oracle, name, w, h, math=0):
    """On oracle output only: the set moves every pair's flow by more than 1e-3 px away from the default-parameter flow."""
    ref, base = _ref(oracle, name, w, h, math), _ref(oracle, None, w, h, math)
    diffs = [float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, base)]
    print(f"tvl1 set {name} {w}x{h} math {math}: oracle against defaults, max-abs per pair {diffs}")
    assert all(np.isfinite(a[0]).all() for a in ref)
    if (name, w, h) in SAME_AS_DEFAULTS:
        assert ref[0][1].nscales == 1 and max(diffs) == 0.0, (name, w, h, diffs)
        return
    assert min(diffs) > DISCRIMINATION, (name, w, h, diffs)


def _check(dfx, oracle, name, w, h, form_kw, math=0):
    _discriminates(oracle, name, w, h, math)
    ref = _ref(oracle, name, w, h, math)
    frames = _frames(w, h)
    tr = ref[-1][1]
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2, **_engine_kw(name), **_Reading(oracle, math).kw(), **form_kw) as eng:
        flows = eng.calc_optflows(frames, 1)  # 3 pairs: a batch of two and a ragged one
        st = eng.stats()
        assert st.levels == tr.nscales
        assert [st.level_w[s] for s in range(st.levels)] == [tr.w[s] for s in range(tr.nscales)]
        assert [st.level_h[s] for s in range(st.levels)] == [tr.h[s] for s in range(tr.nscales)]
        last = eng.calc(frames[-2], frames[-1])
        st = eng.stats()
    assert st.levels == tr.nscales
    assert _iters(st.iters_table()) == _iters(tr.iters_table()), "inner-iteration counts differ from the oracle"
    assert st.tvl1_checks == tr.n_checks
    assert len(flows) == len(ref)
    for i, (got, (want, _)) in enumerate(zip(flows, ref)):
        assert np.array_equal(got, want), f"set {name} {w}x{h} {form_kw}: pair {i} differs, max-abs {np.max(np.abs(got - want))}"
    assert np.array_equal(last, ref[-1][0]), f"set {name} {w}x{h} {form_kw}: calc on the last pair differs"


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,w,h", CASES)
def test_parameter_sets_match_the_oracle(dfx, oracle, name, w, h, form):
    _check(dfx, oracle, name, w, h, FORMS[form])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("math", [2, 3])
@pytest.mark.parametrize("name,w,h", [("A", 97, 61), ("F", 97, 61), ("A", 130, 97), ("F", 130, 97), ("A", 65, 17)])
def test_parameter_sets_under_the_other_hypot_readings(dfx, oracle, name, w, h, math, form):
    _check(dfx, oracle, name, w, h, FORMS[form], math)


def test_expected_level_counts(oracle):
    """What the sets are meant to reach, on the oracle's trace: E keeps two levels at both sizes, D all eight, 65x17 one."""
    for (w, h), half in (((97, 61), (48, 30)), ((130, 97), (65, 48))):  # cvRound: 48.5 -> 48, 30.5 -> 30
        assert _ref(oracle, "E", w, h)[0][1].nscales == 2
        assert _ref(oracle, "D", w, h)[0][1].nscales == 8
        tr = _ref(oracle, "C", w, h)[0][1]
        assert (tr.w[1], tr.h[1]) == half
    assert _ref(oracle, "A", 65, 17)[0][1].nscales == 1 and _ref(oracle, "C", 65, 17)[0][1].nscales == 1


def test_set_size_replans_with_the_handles_own_scale_step(dfx, oracle):
    """130x97 -> 65x49 -> 130x97 on one handle with set F: every stop gives a fresh handle's bits (and the oracle's), and the
    handle holds after the third stop what it held after the first."""
    kw = dict(max_batch=2, **_engine_kw("F"))
    sizes = [(130, 97), (65, 49), (130, 97)]
    fresh = {}
    for w, h in set(sizes):
        _discriminates(oracle, "F", w, h)
        with dfx.FlowEngine(w, h, "tvl1", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(_frames(w, h), 1)
        for got, (want, _) in zip(fresh[(w, h)], _ref(oracle, "F", w, h)):
            assert np.array_equal(got, want), (w, h)
    held = []
    with dfx.FlowEngine(*sizes[0], "tvl1", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            got = eng.calc_optflows(_frames(w, h), 1)
            st = eng.stats()
            tr = _ref(oracle, "F", w, h)[-1][1]
            assert st.levels == tr.nscales
            assert [(st.level_w[s], st.level_h[s]) for s in range(st.levels)] == [(tr.w[s], tr.h[s]) for s in range(tr.nscales)]
            assert len(got) == len(fresh[(w, h)])
            for i, (a, b) in enumerate(zip(got, fresh[(w, h)])):
                assert np.array_equal(a, b), f"after set_size({w}, {h}): pair {i} differs"
            held.append(eng.device_bytes())
    assert held[2] == held[0], held


@pytest.mark.parametrize("kw", [dict(tvl1_scale_step=0.0), dict(tvl1_scale_step=1.0), dict(tvl1_scale_step=1.5),
                                dict(tvl1_theta=0.0)])
def test_refused_parameters(dfx, kw):
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(97, 61, "tvl1", **kw)
    assert e.value.status == INVALID
