"""-a=farn beyond the reference's defaults: polyN 7, windows 1 .. 31, and the row-stream iteration kernel (M never in HBM)
for every window it is built for.  Every comparison is bit-exact: np.array_equal against oracle.farneback_calc(f0, f1, p)
and between the engine's own forms (default, DFX_VAR_FARN_M_IN_HBM, impl = 1, the two polynomial-expansion kernels).

Shapes are the smallest at which a form can go wrong: a second 64-column strip of one column, a second polynomial-expansion
workgroup (256 - 2 * 7 = 242 columns) of one and of eight columns, heights that are no multiple of the 16-row and 6-row
steps, several row segments, levels narrower and shorter than the window, and levels next to the 32-pixel cut."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

UNSUPPORTED = 4
# windows the row-stream kernel runs (farn_stream_has_half, denseflow_amd/csrc/farneback_plan.h): both iteration forms exist
ON_CHIP = {7, 9, 11, 13, 15, 17, 19, 21}

_clips, _refs = {}, {}


def _frames(w, h, seed, n=4):
    key = (w, h, seed, n)
    if key not in _clips:
        _clips[key] = SynthClip(w, h, seed).frames(n)
    return _clips[key]


def _params(oracle, **kw):
    p = oracle.farneback_default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ref(oracle, frames_key, frames, **kw):
    """The oracle's flows of consecutive frames, computed once per case and never changed."""
    key = (frames_key, tuple(sorted(kw.items())))
    if key not in _refs:
        out = [oracle.farneback_calc(frames[i], frames[i + 1], _params(oracle, **kw)) for i in range(len(frames) - 1)]
        for f in out:
            f.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what}: pair {i} differs, max-abs {np.max(np.abs(a - b))}"


# ------------------------------------------------------------------------------------------------ polyN 7

@pytest.mark.parametrize("sigma", [1.5, 1.1])
@pytest.mark.parametrize("w,h,seed", [(33, 40, 2), (97, 61, 9), (243, 49, 3), (250, 49, 4), (485, 33, 5)])
def test_poly_n_7_both_expansion_kernels_match_the_oracle(dfx, oracle, w, h, seed, sigma):
    from denseflow_amd import engine as E

    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=sigma)
    kw = dict(max_batch=2, farn_poly_n=7, farn_poly_sigma=sigma)  # 4 frames, 3 pairs, batches of 2
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:
        rows16 = eng.calc_optflows(frames, 1)
    with dfx.FlowEngine(w, h, "farn", variant=E.VAR_FARN_POLY_ONE_ROW, **kw) as eng:
        one_row = eng.calc_optflows(frames, 1)
    _same(rows16, one_row, "16 rows per workgroup against one row per workgroup")
    _same(rows16, ref, "polyN 7 against the oracle")


@pytest.mark.parametrize("knobs", ["zero_taps", "impl1", "m_in_hbm"])
def test_poly_n_7_cross_check_forms(dfx, oracle, knobs):
    from denseflow_amd import engine as E

    w, h, seed = 250, 49, 4
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=1.5)
    kn = {"zero_taps": dict(variant=E.VAR_FARN_EVAL_ZERO_TAPS), "impl1": dict(impl=1),
          "m_in_hbm": dict(variant=E.VAR_FARN_M_IN_HBM)}[knobs]
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_poly_n=7, farn_poly_sigma=1.5, **kn) as eng:
        out = eng.calc_optflows(frames, 1)
    _same(out, ref, knobs)


# ------------------------------------------------------------------------------------------------ windows

# (winSize, w, h, seed, numIters, numLevels).  65x43: the second strip is one column; 70x500: several row segments;
# 33x40 with windows 21 and 31: the window is wider than the coarse levels; odd iteration counts end in the other flow set.
WINDOW_CASES = [
    (1, 65, 43, 15, 2, 2), (1, 129, 49, 14, 1, 0),
    (3, 129, 49, 14, 3, 5), (3, 70, 500, 12, 2, 2),
    (7, 65, 43, 15, 1, 5), (7, 1000, 77, 6, 2, 2), (7, 70, 500, 12, 3, 0),
    (9, 129, 49, 14, 2, 0), (9, 70, 500, 12, 1, 2),
    (11, 1000, 77, 6, 3, 2), (11, 65, 43, 15, 2, 5),
    (15, 65, 43, 15, 3, 0), (15, 129, 49, 14, 2, 5), (15, 70, 500, 12, 1, 2), (15, 1000, 77, 6, 2, 2),
    (17, 129, 49, 14, 1, 2), (17, 70, 500, 12, 3, 5),
    (19, 65, 43, 15, 2, 2), (19, 1000, 77, 6, 1, 0), (19, 70, 500, 12, 2, 5),
    (21, 65, 43, 15, 1, 0), (21, 129, 49, 14, 3, 2), (21, 70, 500, 12, 2, 5), (21, 1000, 77, 6, 3, 2), (21, 33, 40, 2, 2, 5),
    (25, 129, 49, 14, 2, 5), (25, 70, 500, 12, 1, 0), (25, 65, 43, 15, 3, 2),
    (31, 65, 43, 15, 2, 2), (31, 1000, 77, 6, 3, 5), (31, 33, 40, 2, 1, 0), (31, 70, 500, 12, 2, 2),
]


@pytest.mark.parametrize("win,w,h,seed,iters,levels", WINDOW_CASES)
def test_windows_every_iteration_form_matches_the_oracle(dfx, oracle, win, w, h, seed, iters, levels):
    from denseflow_amd import engine as E

    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, win_size=win, num_iters=iters, num_levels=levels)
    kw = dict(max_batch=2, farn_win_size=win, farn_num_iters=iters, farn_num_levels=levels)
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:
        out = eng.calc_optflows(frames, 1)
    _same(out, ref, f"winSize {win} against the oracle")
    with dfx.FlowEngine(w, h, "farn", impl=1, **kw) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"winSize {win}, impl = 1")
    if win in ON_CHIP:  # the default ran the row-stream kernel: the M-in-HBM kernel is another form
        with dfx.FlowEngine(w, h, "farn", variant=E.VAR_FARN_M_IN_HBM, **kw) as eng:
            _same(eng.calc_optflows(frames, 1), ref, f"winSize {win}, M in HBM")


def test_combined_poly_n_7_window_15(dfx, oracle):
    from denseflow_amd import engine as E

    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=1.5, win_size=15, num_levels=3, num_iters=3)
    kw = dict(max_batch=2, farn_poly_n=7, farn_poly_sigma=1.5, farn_win_size=15, farn_num_levels=3, farn_num_iters=3)
    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM), dict(impl=1)):
        with dfx.FlowEngine(w, h, "farn", **kw, **knobs) as eng:
            _same(eng.calc_optflows(frames, 1), ref, str(knobs))


@pytest.mark.parametrize("win", [15, 21])
def test_windows_on_unrelated_frames(dfx, oracle, win):
    """Two textures and a noise frame: large, erratic flows, taps that leave the image, neighbours that do not sample
    neighbouring taps — the per-pixel gather and the invalid-tap handling of the new row-stream instantiations."""
    from denseflow_amd import engine as E

    w, h = 256, 128
    noise = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    frames = [SynthClip(w, h, 31).frame(0), SynthClip(w, h, 32).frame(5), noise, SynthClip(w, h, 31).frame(40)]
    ref = _ref(oracle, ("unrelated", w, h), frames, win_size=win)
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_win_size=win) as eng:
        out = eng.calc_optflows(frames, 1)
    assert max(float(np.abs(f).max()) for f in out) > 8.0, "the case is meant to produce flows that vary by many pixels"
    _same(out, ref, f"winSize {win} against the oracle")
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_win_size=win, variant=E.VAR_FARN_M_IN_HBM) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"winSize {win}, M in HBM")


# ------------------------------------------------------------------------------------------------ outputs

@pytest.mark.parametrize("iters", [1, 3])  # 1: the level's only iteration is its first, k_farn_merge_planar writes the planes
@pytest.mark.parametrize("bound", [None, 20.0])
def test_planar_output_is_the_interleaved_output(dfx, oracle, iters, bound):
    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=1.5, win_size=15, num_iters=iters)
    kw = dict(max_batch=2, farn_poly_n=7, farn_poly_sigma=1.5, farn_win_size=15, farn_num_iters=iters)
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:
        inter = eng.calc_optflows(frames, 1)
        got = eng.calc_optflows_planar(frames, 1, bound=bound)
    _same(inter, ref, "interleaved against the oracle")
    want = np.stack(inter).transpose(0, 3, 1, 2)
    if bound is not None:
        want = np.clip(want, -bound, bound).astype(np.float32) / np.float32(bound)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_u8_output_is_the_oracles_quantiser(dfx, oracle):
    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=1.5, win_size=15)
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_poly_n=7, farn_poly_sigma=1.5, farn_win_size=15) as eng:
        img_x, img_y = eng.calc_optflows_u8(frames, 1, 20)
    assert len(img_x) == len(img_y) == len(ref)
    for i, flow in enumerate(ref):
        ox, oy = oracle.flow_to_u8(flow, -20, 20)
        assert np.array_equal(img_x[i], ox) and np.array_equal(img_y[i], oy), i


# ------------------------------------------------------------------------------------------------ re-planning

def test_set_size_gives_the_bits_of_a_fresh_handle(dfx, oracle):
    """224x160 -> 97x61 -> 224x160 on one handle (winSize 15 on the row-stream kernel, polyN 7): every stop computes a fresh
    handle's bits, and the handle holds after the last stop what it held after the first — the smaller plan fits the
    buffers of the larger one, and coming back re-plans inside them."""
    kw = dict(max_batch=2, farn_poly_n=7, farn_poly_sigma=1.5, farn_win_size=15)
    sizes = [(224, 160), (97, 61), (224, 160)]
    fresh = {}
    for w, h in set(sizes):
        with dfx.FlowEngine(w, h, "farn", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(_frames(w, h, 77), 1)
    _same(fresh[(97, 61)], _ref(oracle, (97, 61, 77), _frames(97, 61, 77), poly_n=7, poly_sigma=1.5, win_size=15), "fresh handle")
    held = []
    with dfx.FlowEngine(*sizes[0], "farn", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            before = eng.device_bytes()
            _same(eng.calc_optflows(_frames(w, h, 77), 1), fresh[(w, h)], f"after set_size({w}, {h})")
            # read once the stop has computed its flows: frame slots and staging are allocated by the first FlowBuffer
            held.append(eng.device_bytes())
            if len(held) > 1:
                assert before == held[-1] == held[0], (before, held)  # the smaller stop and the way back move nothing
    assert held[2] == held[0], held


@pytest.mark.parametrize("win", [15, 21])
def test_on_chip_window_holds_fewer_device_bytes(dfx, win):
    from denseflow_amd import engine as E

    with dfx.FlowEngine(224, 160, "farn", max_batch=2, farn_win_size=win) as eng:
        on_chip = eng.device_bytes()
    with dfx.FlowEngine(224, 160, "farn", max_batch=2, farn_win_size=win, variant=E.VAR_FARN_M_IN_HBM) as eng:
        in_hbm = eng.device_bytes()
    assert on_chip < in_hbm, (on_chip, in_hbm)  # 4 planes per pair slot instead of 14


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.parametrize("kw", [dict(farn_poly_n=6), dict(farn_poly_n=9), dict(farn_win_size=33), dict(farn_win_size=14)])
def test_refused_parameters(dfx, kw):
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(128, 96, "farn", **kw)
    assert e.value.status == UNSUPPORTED


def test_defaults_are_still_the_oracles_bits(dfx, oracle):
    w, h = 224, 224
    clip = SynthClip(w, h, 1)
    f0, f1 = clip.frame(0), clip.frame(1)
    with dfx.FlowEngine(w, h, "farn") as eng:
        out = eng.calc(f0, f1)
    assert np.array_equal(out, oracle.farneback_calc(f0, f1))


# ------------------------------------------------------------------------------------------------ pyrScale
#
# farn_pyr_scale away from 0.5: the pyramid geometry (level count and sizes, pre-blur widths, the run-time resize factors and
# the 1 / pyrScale flow gain of the INIT form) follows the handle's value.  (pyrScale, numLevels, w, h, seed, levels expected
# from farn_plan's rule: crop while W * scale < 32 || H * scale < 32).  300 = 4 strips of 64 + 44 columns = one
# polynomial-expansion workgroup of 242 + 58 columns.  0.9 with 15 levels fills all DFX_LVL_MAX = 16 levels (pre-blur sigma
# 0.056: the kernel size clamps to 3, taps near {0, 1, 0}); 0.3 gives a pre-blur half width of 3 at level 1.
#
# Frames are 8 clip frames apart (12 px of motion per pair): on consecutive frames the coarse levels only refine what
# level 0 finds anyway, and the oracle's flow moves by 1e-5 .. 7e-4 px with pyrScale — below the 1e-3 px this file
# requires of every case before it touches the engine.  At this spacing it moves by 0.1 .. 20 px.
PYR_DT = 8
PYR_DISCRIMINATION = 1e-3
PYR_CASES = {1: (0.8, 5, 300, 200, 6), 2: (0.3, 5, 300, 200, 6), 3: (0.9, 15, 300, 200, 6), 4: (0.75, 8, 129, 97, 5)}
PYR_LEVELS = {1: 6, 2: 2, 3: 16}  # case 4: from _plan_levels


def _plan_levels(w, h, pyr_scale, num_levels):
    """farn_plan (denseflow_amd/csrc/engine_plan.h): levels 0 .. cropped."""
    scale, cropped = 1.0, 0
    while cropped < num_levels:
        scale *= pyr_scale
        if w * scale < 32 or h * scale < 32:
            break
        cropped += 1
    return cropped + 1


def _pyr_frames(w, h, seed, n=4):
    key = ("pyr", w, h, seed, n)
    if key not in _clips:
        clip = SynthClip(w, h, seed)
        _clips[key] = [clip.frame(PYR_DT * i) for i in range(n)]
    return _clips[key]


def _pyr_ref(oracle, case, **kw):
    """The oracle's flows of a pyrScale case after the check, on oracle output only, that pyrScale moves every one of them by
    more than 1e-3 px away from the flow the same parameters give at the default pyrScale and numLevels."""
    ps, nl, w, h, seed = PYR_CASES[case]
    frames = _pyr_frames(w, h, seed)
    ref = _ref(oracle, ("pyr", w, h, seed), frames, pyr_scale=ps, num_levels=nl, **kw)
    base = _ref(oracle, ("pyr", w, h, seed), frames, **kw)
    diffs = [float(np.max(np.abs(a - b))) for a, b in zip(ref, base)]
    print(f"farn pyrScale case {case} {kw}: oracle against the default pyramid, max-abs per pair {diffs}")
    assert all(np.isfinite(a).all() for a in ref)
    assert min(diffs) > PYR_DISCRIMINATION, (case, kw, diffs)
    return frames, ref


def _pyr_kw(case, win, iters):
    ps, nl = PYR_CASES[case][:2]
    return dict(max_batch=2, farn_pyr_scale=ps, farn_num_levels=nl, farn_win_size=win, farn_num_iters=iters)


# win 13: the tuned instantiation; 15: a row-stream instantiation; 25: the generic kernel; iters 1: INIT is a level's only launch
PYR_RUNS = [(c, win, 3) for c in (1, 2, 3, 4) for win in (13, 15)] + [(1, 25, 3), (1, 13, 1), (1, 15, 1)]


@pytest.mark.parametrize("case,win,iters", PYR_RUNS)
def test_pyr_scale_every_form_matches_the_oracle(dfx, oracle, case, win, iters):
    from denseflow_amd import engine as E

    ps, nl, w, h, _ = PYR_CASES[case]
    frames, ref = _pyr_ref(oracle, case, win_size=win, num_iters=iters)
    levels = _plan_levels(w, h, ps, nl)
    assert levels == PYR_LEVELS.get(case, levels)
    kw = _pyr_kw(case, win, iters)
    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM), dict(impl=1)):
        with dfx.FlowEngine(w, h, "farn", **kw, **knobs) as eng:
            out = eng.calc_optflows(frames, 1)  # 4 frames, 3 pairs, batches of 2
            st = eng.stats()
        assert st.levels == levels, (knobs, st.levels, levels)
        _same(out, ref, f"pyrScale {ps}, {nl} levels, winSize {win}, {iters} iterations, {knobs}")


@pytest.mark.parametrize("win", [13, 15, 25])
def test_pyr_scale_with_the_gaussian_window(dfx, oracle, win):
    from denseflow_amd import engine as E
    from tests import farneback_window_ref as WR

    ps, nl, w, h, seed = PYR_CASES[1]
    frames = _pyr_frames(w, h, seed)

    def gauss(**kw):
        key = (("pyr-gauss", w, h, seed), tuple(sorted(kw.items())))
        if key not in _refs:
            out = [WR.farneback_flow(oracle, frames[i], frames[i + 1], _params(oracle, **kw), "gaussian") for i in range(3)]
            for f in out:
                f.setflags(write=False)
            _refs[key] = out
        return _refs[key]

    ref, base = gauss(pyr_scale=ps, num_levels=nl, win_size=win, num_iters=3), gauss(win_size=win, num_iters=3)
    diffs = [float(np.max(np.abs(a - b))) for a, b in zip(ref, base)]
    print(f"farn pyrScale case 1, Gaussian winSize {win}: reference against the default pyramid, max-abs per pair {diffs}")
    assert min(diffs) > PYR_DISCRIMINATION, diffs
    kw = dict(farn_window=1, **_pyr_kw(1, win, 3))
    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM), dict(impl=1)):
        with dfx.FlowEngine(w, h, "farn", **kw, **knobs) as eng:
            _same(eng.calc_optflows(frames, 1), ref, f"Gaussian window, pyrScale {ps}, winSize {win}, {knobs}")


def test_pyr_scale_planar_output_is_the_interleaved_output(dfx, oracle):
    bound = 20.0
    w, h = PYR_CASES[1][2:4]
    frames, ref = _pyr_ref(oracle, 1, win_size=13, num_iters=3)
    with dfx.FlowEngine(w, h, "farn", **_pyr_kw(1, 13, 3)) as eng:
        inter = eng.calc_optflows(frames, 1)
        got = eng.calc_optflows_planar(frames, 1, bound=bound)
    _same(inter, ref, "interleaved against the oracle")
    want = np.clip(np.stack(inter).transpose(0, 3, 1, 2), -bound, bound).astype(np.float32) / np.float32(bound)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_pyr_scale_set_size_gives_the_bits_of_a_fresh_handle(dfx, oracle):
    """300x200 -> 97x61 -> 300x200 on one handle at pyrScale 0.8: re-planning follows the handle's pyrScale, every stop
    computes a fresh handle's (and the oracle's) bits, and the handle holds after the last stop what it held after the first."""
    kw = dict(max_batch=2, farn_pyr_scale=0.8)
    sizes = [(300, 200), (97, 61), (300, 200)]
    seeds = {(300, 200): 6, (97, 61): 9}
    fresh = {}
    for (w, h), seed in seeds.items():
        frames = _pyr_frames(w, h, seed)
        ref, base = _ref(oracle, ("pyr", w, h, seed), frames, pyr_scale=0.8), _ref(oracle, ("pyr", w, h, seed), frames)
        assert min(float(np.max(np.abs(a - b))) for a, b in zip(ref, base)) > PYR_DISCRIMINATION
        with dfx.FlowEngine(w, h, "farn", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(frames, 1)
            assert eng.stats().levels == _plan_levels(w, h, 0.8, 5)
        _same(fresh[(w, h)], ref, f"fresh handle at {w}x{h}")
    held = []
    with dfx.FlowEngine(*sizes[0], "farn", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            _same(eng.calc_optflows(_pyr_frames(w, h, seeds[(w, h)]), 1), fresh[(w, h)], f"after set_size({w}, {h})")
            assert eng.stats().levels == _plan_levels(w, h, 0.8, 5)
            held.append(eng.device_bytes())
    assert held[2] == held[0], held


@pytest.mark.parametrize("kw", [dict(farn_pyr_scale=0.0), dict(farn_pyr_scale=1.0), dict(farn_num_levels=16)])
def test_refused_pyramid_parameters(dfx, kw):
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(300, 200, "farn", **kw)
    assert e.value.status == 1  # DFX_ERR_INVALID
