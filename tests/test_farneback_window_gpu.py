"""-a=farn with the Gaussian update window (dfx_params.farn_window = DFX_FARN_WINDOW_GAUSSIAN): every kernel form — the
row-stream kernels of windows 7 .. 21 (plain, INIT, PLANAR), the generic kernel (windows 1 .. 5 and 23 .. 31, impl = 1,
DFX_VAR_FARN_M_IN_HBM) — against tests/farneback_window_ref.py, bit for bit (np.array_equal: the device arithmetic is the
reference's, operation for operation), and the box window after it, untouched.

Shapes are the smallest at which these kernels can go wrong: 65x43 (the second strip is one column), 129x49 (a third strip of
one column, a height that is no multiple of 6), 70x500 (several row segments), 1000x77 (many strips, levels next to the
32-pixel cut), 33x40 (levels narrower and shorter than the window).  Odd and even iteration counts end in different flow
sets; one-iteration levels run the INIT form as the only launch."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import farneback_window_ref as WR

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
GAUSS = 1  # DFX_FARN_WINDOW_GAUSSIAN
ON_CHIP = {7, 9, 11, 13, 15, 17, 19, 21}  # farn_stream_has_half (denseflow_amd/csrc/farneback_plan.h)

_clips, _refs = {}, {}


def _frames(w, h, seed, n=4):
    key = (w, h, seed, n)
    if key not in _clips:
        _clips[key] = SynthClip(w, h, seed).frames(n)
    return _clips[key]


def _ref(oracle, frames_key, frames, **kw):
    """The Gaussian reference flows of consecutive frames, computed once per case and never changed."""
    key = (frames_key, tuple(sorted(kw.items())))
    if key not in _refs:
        p = oracle.farneback_default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        out = [WR.farneback_flow(oracle, frames[i], frames[i + 1], p, "gaussian") for i in range(len(frames) - 1)]
        for f in out:
            f.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what}: pair {i} differs, max-abs {np.max(np.abs(a - b))}"


# ------------------------------------------------------------------------------------------------ every window form

# (winSize, w, h, seed, numIters, numLevels)
WINDOW_CASES = [
    (1, 65, 43, 15, 2, 2), (3, 129, 49, 14, 3, 5), (5, 70, 500, 12, 2, 2),
    (7, 65, 43, 15, 1, 5), (7, 70, 500, 12, 3, 0), (9, 129, 49, 14, 2, 0), (11, 1000, 77, 6, 3, 2),
    (13, 129, 49, 14, 3, 5), (13, 70, 500, 12, 2, 2), (15, 65, 43, 15, 3, 0), (15, 1000, 77, 6, 2, 2),
    (17, 70, 500, 12, 3, 5), (19, 65, 43, 15, 2, 2), (21, 129, 49, 14, 3, 2), (21, 70, 500, 12, 2, 5),
    (21, 33, 40, 2, 2, 5), (23, 129, 49, 14, 2, 5), (25, 65, 43, 15, 3, 2), (31, 33, 40, 2, 1, 0),
]


@pytest.mark.parametrize("win,w,h,seed,iters,levels", WINDOW_CASES)
def test_gaussian_window_every_iteration_form_matches_the_reference(dfx, oracle, win, w, h, seed, iters, levels):
    from denseflow_amd import engine as E

    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, win_size=win, num_iters=iters, num_levels=levels)
    kw = dict(max_batch=2, farn_window=GAUSS, farn_win_size=win, farn_num_iters=iters, farn_num_levels=levels)
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:  # 4 frames, 3 pairs, batches of 2
        _same(eng.calc_optflows(frames, 1), ref, f"Gaussian winSize {win} against the reference")
    with dfx.FlowEngine(w, h, "farn", impl=1, **kw) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"Gaussian winSize {win}, impl = 1")
    if win in ON_CHIP:  # the default ran the row-stream kernel: the generic kernel is another form
        with dfx.FlowEngine(w, h, "farn", variant=E.VAR_FARN_M_IN_HBM, **kw) as eng:
            _same(eng.calc_optflows(frames, 1), ref, f"Gaussian winSize {win}, M in HBM")


@pytest.mark.parametrize("win", [15, 21])
def test_gaussian_window_on_unrelated_frames(dfx, oracle, win):
    """Two textures and a noise frame: large, erratic flows, taps that leave the image, neighbours that do not sample
    neighbouring taps."""
    from denseflow_amd import engine as E

    w, h = 256, 128
    noise = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    frames = [SynthClip(w, h, 31).frame(0), SynthClip(w, h, 32).frame(5), noise, SynthClip(w, h, 31).frame(40)]
    ref = _ref(oracle, ("unrelated", w, h), frames, win_size=win)
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_window=GAUSS, farn_win_size=win) as eng:
        out = eng.calc_optflows(frames, 1)
    assert max(float(np.abs(f).max()) for f in out) > 8.0, "the case is meant to produce flows that vary by many pixels"
    _same(out, ref, f"Gaussian winSize {win} against the reference")
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_window=GAUSS, farn_win_size=win, variant=E.VAR_FARN_M_IN_HBM) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"Gaussian winSize {win}, M in HBM")


def test_gaussian_window_combined_with_poly_n_7(dfx, oracle):
    from denseflow_amd import engine as E

    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, poly_n=7, poly_sigma=1.5, win_size=15, num_levels=3, num_iters=3)
    kw = dict(max_batch=2, farn_window=GAUSS, farn_poly_n=7, farn_poly_sigma=1.5, farn_win_size=15, farn_num_levels=3,
              farn_num_iters=3)
    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM), dict(impl=1)):
        with dfx.FlowEngine(w, h, "farn", **kw, **knobs) as eng:
            _same(eng.calc_optflows(frames, 1), ref, str(knobs))


# ------------------------------------------------------------------------------------------------ outputs

@pytest.mark.parametrize("iters", [1, 3])  # 3: the PLANAR stream instantiation; 1: k_farn_merge_planar writes the planes
@pytest.mark.parametrize("bound", [None, 20.0])
def test_planar_output_is_the_interleaved_output(dfx, oracle, iters, bound):
    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, win_size=15, num_iters=iters)
    kw = dict(max_batch=2, farn_window=GAUSS, farn_win_size=15, farn_num_iters=iters)
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:
        inter = eng.calc_optflows(frames, 1)
        got = eng.calc_optflows_planar(frames, 1, bound=bound)
    _same(inter, ref, "interleaved against the reference")
    want = np.stack(inter).transpose(0, 3, 1, 2)
    if bound is not None:
        want = np.clip(want, -bound, bound).astype(np.float32) / np.float32(bound)
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_u8_output_is_the_oracles_quantiser(dfx, oracle):
    w, h, seed = 130, 97, 5
    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, win_size=15)
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_window=GAUSS, farn_win_size=15) as eng:
        img_x, img_y = eng.calc_optflows_u8(frames, 1, 20)
    assert len(img_x) == len(img_y) == len(ref)
    for i, flow in enumerate(ref):
        ox, oy = oracle.flow_to_u8(flow, -20, 20)
        assert np.array_equal(img_x[i], ox) and np.array_equal(img_y[i], oy), i


# ------------------------------------------------------------------------------------------------ re-planning, memory

def test_set_size_gives_the_bits_of_a_fresh_handle(dfx, oracle):
    """224x160 -> 97x61 -> 224x160 on one Gaussian handle (winSize 15, the row-stream kernel): every stop computes a fresh
    handle's bits — the taps follow from the parameters alone — and the handle holds after the last stop what it held
    after the first."""
    kw = dict(max_batch=2, farn_window=GAUSS, farn_win_size=15)
    sizes = [(224, 160), (97, 61), (224, 160)]
    fresh = {}
    for w, h in set(sizes):
        with dfx.FlowEngine(w, h, "farn", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(_frames(w, h, 77), 1)
    _same(fresh[(97, 61)], _ref(oracle, (97, 61, 77), _frames(97, 61, 77), win_size=15), "fresh handle")
    held = []
    with dfx.FlowEngine(*sizes[0], "farn", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            _same(eng.calc_optflows(_frames(w, h, 77), 1), fresh[(w, h)], f"after set_size({w}, {h})")
            held.append(eng.device_bytes())  # read once the stop has computed its flows (frame slots, staging)
    assert held[2] == held[0], held


@pytest.mark.parametrize("win", [15, 21])
def test_gaussian_handle_holds_the_box_handles_device_bytes(dfx, win):
    from denseflow_amd import engine as E

    kw = dict(max_batch=2, farn_win_size=win)
    with dfx.FlowEngine(224, 160, "farn", **kw) as eng:
        box = eng.device_bytes()
    with dfx.FlowEngine(224, 160, "farn", farn_window=GAUSS, **kw) as eng:
        gauss = eng.device_bytes()
    with dfx.FlowEngine(224, 160, "farn", farn_window=GAUSS, variant=E.VAR_FARN_M_IN_HBM, **kw) as eng:
        in_hbm = eng.device_bytes()
    assert gauss == box, (gauss, box)
    assert gauss < in_hbm, (gauss, in_hbm)  # 4 planes per pair slot instead of 14


# ------------------------------------------------------------------------------------------------ the box is untouched

def test_the_box_window_after_a_gaussian_handle_is_still_the_oracles_bits(dfx, oracle):
    w, h = 224, 224
    clip = SynthClip(w, h, 1)
    f0, f1 = clip.frame(0), clip.frame(1)
    want = oracle.farneback_calc(f0, f1)
    with dfx.FlowEngine(w, h, "farn", farn_window=GAUSS) as eng:
        gauss = eng.calc(f0, f1)
    assert not np.array_equal(gauss, want)
    with dfx.FlowEngine(w, h, "farn") as eng:
        assert np.array_equal(eng.calc(f0, f1), want)
    with dfx.FlowEngine(w, h, "farn", farn_window=0) as eng:
        assert np.array_equal(eng.calc(f0, f1), want)


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.parametrize("kw,status", [(dict(farn_window=2), INVALID), (dict(farn_window=-1), INVALID),
                                       (dict(farn_flags=4), UNSUPPORTED)])
def test_refused_parameters(dfx, kw, status):
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(128, 96, "farn", **kw)
    assert e.value.status == status


def test_default_params_choose_the_box(dfx):
    assert dfx.engine.default_params().farn_window == 0


def test_farn_window_is_ignored_by_tvl1(dfx):
    f0, f1 = _frames(96, 64, 5, 2)
    with dfx.FlowEngine(96, 64, "tvl1") as eng:
        want = eng.calc(f0, f1)
    with dfx.FlowEngine(96, 64, "tvl1", farn_window=GAUSS) as eng:
        assert np.array_equal(eng.calc(f0, f1), want)
