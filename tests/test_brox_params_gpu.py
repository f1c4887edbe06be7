"""-a=brox away from the reference's float defaults: alpha, gamma and scale_factor — with the pyramids scale_factor leads to,
from one level to more than dfx.h's DFX_MAX_LEVELS = 32, and coarsest levels down to 1 x 2 pixels, far below the 16 px a
default pyramid stops at — reach every kernel form, and the flows stay the bits of oracle.brox_calc with the same parameters
(np.array_equal: the device evaluates the oracle's expressions in the oracle's order).

Each set has to move the oracle's own flow by more than 1e-3 px (max-abs) away from the default-parameter flow on the same
frames, or — for the sets without any solver work — make it exactly zero; the tests assert that on oracle output before the
engine is touched.

Shapes: 97x61 (a second 64-column block of 33 columns, odd height), 20x33 (narrower than a block, levels of a few pixels),
333x201 (several SOR tiles, odd borders).  Four frames with max_batch = 2 are three pairs in a full and a ragged batch."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

DISCRIMINATION = 1e-3  # px, max-abs between the oracle's flow under a set and under the defaults
MAX_LEVELS = 32        # DFX_MAX_LEVELS (include/dfx.h): what dfx_stats can report

# id -> oracle BroxParams fields; the engine takes the same values as brox_<name>
SETS = {
    "a": dict(alpha=0.05),
    "b": dict(alpha=1.0, gamma=0.0),
    "c": dict(gamma=5.0),
    "d": dict(scale_factor=0.5),
    "e": dict(scale_factor=0.95),          # 29 levels at 97x61
    "f": dict(scale_factor=0.1),           # coarsest level 2x4 at 20x33, 10x7 at 97x61
    "g": dict(scale_factor=0.05),          # coarsest level 1x2 at 20x33, 5x4 at 97x61
    "h": dict(outer_iterations=1),         # one level, no prolongation
    "i": dict(inner_iterations=0),         # no inner iteration: exact zeros
    "j": dict(solver_iterations=0),        # no sweep: exact zeros
}
ZERO_SETS = {"i", "j"}
SIZES = {(97, 61): 9, (20, 33): 2, (333, 201): 5, (224, 224): 1, (96, 80): 21, (64, 48): 3}  # (w, h) -> SynthClip seed
COARSEST = {("e", 97, 61): 29, ("f", 20, 33): (2, 4), ("f", 97, 61): (10, 7), ("g", 20, 33): (1, 2), ("g", 97, 61): (5, 4),
            ("h", 97, 61): 1, ("h", 20, 33): 1}
CASES = [(s, w, h) for (w, h) in ((97, 61), (20, 33)) for s in SETS] + [("d", 333, 201), ("e", 333, 201)]
FORMS = ["tuned", "impl1", "sor_per_tile"]

_clips, _refs = {}, {}


def _form_kw(form):
    from denseflow_amd import engine as E

    return {"tuned": dict(), "impl1": dict(impl=1), "sor_per_tile": dict(variant=E.VAR_BROX_SOR_PER_TILE)}[form]


def _frames(w, h, n=4):
    if (w, h, n) not in _clips:
        _clips[(w, h, n)] = SynthClip(w, h, SIZES[(w, h)]).frames(n)
    return _clips[(w, h, n)]


def _params(oracle, name):
    p = oracle.brox_default_params()
    for k, v in (SETS[name] if name else {}).items():
        setattr(p, k, v)
    return p


def _engine_kw(name):
    return {"brox_" + k: v for k, v in SETS[name].items()}


def _ref(oracle, name, w, h, n=4, step=1):
    """The oracle's flows (frame i -> i + step) under set `name` (None: the defaults), computed once and never changed."""
    key = (name, w, h, n, step)
    if key not in _refs:
        frames = _frames(w, h, n)
        out = [oracle.brox_calc(frames[i], frames[i + step], _params(oracle, name)) for i in range(n - step)]
        for f in out:
            f.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _discriminates(oracle, name, w, h, n=4, step=1):
    """On oracle output only: the set moves every pair's flow by more than 1e-3 px away from the default-parameter flow;
    the sets without solver work give exact zeros instead."""
    ref = _ref(oracle, name, w, h, n, step)
    if name in ZERO_SETS:
        assert all(not f.any() for f in ref), name
        return
    base = _ref(oracle, None, w, h, n, step)
    diffs = [float(np.max(np.abs(a - b))) for a, b in zip(ref, base)]
    print(f"brox set {name} {w}x{h}: oracle against defaults, max-abs per pair {diffs}")
    assert all(np.isfinite(f).all() for f in ref)
    assert min(diffs) > DISCRIMINATION, (name, w, h, diffs)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what}: pair {i} differs, max-abs {np.max(np.abs(a - b))}"


def _check_geometry(st, sizes):
    assert st.levels == min(len(sizes), MAX_LEVELS)
    assert [(st.level_w[l], st.level_h[l]) for l in range(st.levels)] == [tuple(s) for s in sizes[:MAX_LEVELS]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,w,h", CASES)
def test_parameter_sets_match_the_oracle(dfx, oracle, name, w, h, form):
    _discriminates(oracle, name, w, h)
    sizes = oracle.brox_pyramid_sizes(w, h, _params(oracle, name))
    want = COARSEST.get((name, w, h))
    if isinstance(want, int):
        assert len(sizes) == want
    elif want is not None:
        assert tuple(sizes[-1]) == want
    frames = _frames(w, h)
    with dfx.FlowEngine(w, h, "brox", max_batch=2, **_engine_kw(name), **_form_kw(form)) as eng:
        out = eng.calc_optflows(frames, 1)  # 3 pairs: a batch of two and a ragged one
        st = eng.stats()
    _check_geometry(st, sizes)
    _same(out, _ref(oracle, name, w, h), f"set {name} {w}x{h} {form}")


def test_more_levels_than_the_stats_can_report(dfx, oracle):
    """scale_factor 0.95 at 224x224 with the default outer_iterations = 77: the pyramid is deeper than DFX_MAX_LEVELS.  The
    engine runs all of it (the flow is the oracle's) and reports the first 32 levels."""
    w, h = 224, 224
    p = _params(oracle, "e")
    sizes = oracle.brox_pyramid_sizes(w, h, p)
    assert len(sizes) > MAX_LEVELS
    frames = _frames(w, h, 2)
    ref, base = oracle.brox_calc(frames[0], frames[1], p), oracle.brox_calc(frames[0], frames[1])
    assert np.max(np.abs(ref - base)) > DISCRIMINATION
    with dfx.FlowEngine(w, h, "brox", **_engine_kw("e")) as eng:
        out = eng.calc(frames[0], frames[1])
        st = eng.stats()
    assert st.levels == MAX_LEVELS
    assert [(st.level_w[l], st.level_h[l]) for l in range(MAX_LEVELS)] == [tuple(s) for s in sizes[:MAX_LEVELS]]
    assert np.array_equal(out, ref), f"max-abs {np.max(np.abs(out - ref))}"


@pytest.mark.parametrize("form", FORMS)
def test_step_2_batches_of_three_with_scale_factor_half(dfx, oracle, form):
    w, h, n = 96, 80, 6
    _discriminates(oracle, "d", w, h, n, 2)
    with dfx.FlowEngine(w, h, "brox", max_batch=3, **_engine_kw("d"), **_form_kw(form)) as eng:
        out = eng.calc_optflows(_frames(w, h, n), 2)  # 4 pairs: a batch of three and a ragged one
        st = eng.stats()
    _check_geometry(st, oracle.brox_pyramid_sizes(w, h, _params(oracle, "d")))
    _same(out, _ref(oracle, "d", w, h, n, 2), f"set d, step 2, {form}")


def test_set_size_replans_with_the_handles_own_scale_factor(dfx, oracle):
    """97x61 -> 64x48 -> 97x61 on one handle with set d: every stop gives a fresh handle's (and the oracle's) bits and level
    sizes, and the handle holds after the third stop what it held after the first."""
    kw = dict(max_batch=2, **_engine_kw("d"))
    sizes = [(97, 61), (64, 48), (97, 61)]
    fresh = {}
    for w, h in set(sizes):
        _discriminates(oracle, "d", w, h)
        with dfx.FlowEngine(w, h, "brox", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(_frames(w, h), 1)
        _same(fresh[(w, h)], _ref(oracle, "d", w, h), f"fresh handle at {w}x{h}")
    held = []
    with dfx.FlowEngine(*sizes[0], "brox", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            _same(eng.calc_optflows(_frames(w, h), 1), fresh[(w, h)], f"after set_size({w}, {h})")
            _check_geometry(eng.stats(), oracle.brox_pyramid_sizes(w, h, _params(oracle, "d")))
            held.append(eng.device_bytes())
    assert held[2] == held[0], held
