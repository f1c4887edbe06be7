"""-a=farn with fast pyramids (dfx_params.farn_fast_pyramids = 1): k_farn_pyrdown, k_farn_pyrup_flow
and the engine's fast route — the row-stream kernels started on a pyrUp'd flow, the generic kernels (impl = 1,
DFX_VAR_FARN_M_IN_HBM, windows 5 and 23), every output form — against tests/farneback_fastpyr_ref.py, bit for bit
(np.array_equal: the device arithmetic is the reference's, operation for operation), and the default path after it, untouched.

Shapes are the smallest at which these kernels can go wrong (CASES has what each one exercises); the level rule accepts all
of them (tests/test_farneback_fastpyr_ref.py).  4 frames, 3 pairs, batches of 2 unless noted."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import farneback_fastpyr_ref as FR

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
FAST = dict(farn_fast_pyramids=1)

_clips, _refs = {}, {}


def _frames(w, h, seed, n=4):
    key = (w, h, seed, n)
    if key not in _clips:
        _clips[key] = SynthClip(w, h, seed).frames(n)
    return _clips[key]


def _ref(oracle, frames_key, frames, window="box", fast=True, seeds=None, **fields):
    """The reference flows of consecutive frames, computed once per case and never changed."""
    key = (frames_key, window, fast, seeds is not None, tuple(sorted(fields.items())))
    if key not in _refs:
        p = oracle.farneback_default_params()
        for k, v in fields.items():
            setattr(p, k, v)
        out = [FR.farneback_flow(oracle, frames[i], frames[i + 1], p, fast=fast, window=window,
                                 seed=None if seeds is None else seeds[i]) for i in range(len(frames) - 1)]
        for f in out:
            f.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"{what}: pair {i} differs, max-abs {np.max(np.abs(a - b))}"


# ------------------------------------------------------------------------------------------------ every route

# (w, h, numLevels, numIters, seed)
CASES = [
    (97, 61, 0, 3, 3),     # no pyramid at all: only the missing level-0 blur; an odd size is accepted at 0 levels
    (66, 64, 1, 2, 4),     # a second 64-column strip of two columns; the coarsest level 33 x 32 is odd in x
    (132, 140, 2, 3, 5),   # two pyrDown steps, coarsest 33 x 35 odd both ways, pyrUp from an odd plane
    (132, 140, 2, 1, 5),   # one iteration per level: the former INIT-only launch
    (520, 72, 1, 2, 6),    # a pyrDown row across 256-lane and 64-column boundaries, level 1 at the 32-pixel cut (36 rows)
    (72, 520, 1, 3, 7),    # many row segments of the stream kernel under a pyrUp start
    (256, 256, 3, 2, 8),   # four levels, the coarsest exactly 32 x 32; an even iteration count ...
    (256, 256, 3, 3, 8),   # ... and an odd one: different final flow sets
    (1088, 72, 1, 1, 9),   # many strips; one iteration
]


@pytest.mark.parametrize("w,h,levels,iters,seed", CASES)
def test_fast_pyramids_on_every_route_match_the_reference(dfx, oracle, w, h, levels, iters, seed):
    from denseflow_amd import engine as E

    frames = _frames(w, h, seed)
    ref = _ref(oracle, (w, h, seed), frames, num_levels=levels, num_iters=iters)
    kw = dict(max_batch=2, farn_num_levels=levels, farn_num_iters=iters, **FAST)
    with dfx.FlowEngine(w, h, "farn", **kw) as eng:  # the row-stream kernel (winSize 13)
        _same(eng.calc_optflows(frames, 1), ref, f"{w}x{h} levels {levels} iters {iters}")
        st = eng.stats()
        assert st.levels == levels + 1
        assert [(st.level_w[k], st.level_h[k]) for k in range(st.levels)] == FR.fast_level_sizes(w, h, levels)
    with dfx.FlowEngine(w, h, "farn", impl=1, **kw) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"{w}x{h} levels {levels} iters {iters}, impl = 1")
    with dfx.FlowEngine(w, h, "farn", variant=E.VAR_FARN_M_IN_HBM, **kw) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"{w}x{h} levels {levels} iters {iters}, M in HBM")


# ------------------------------------------------------------------------------------------------ composition, 132 x 140 at 2

W2, H2, SEED2 = 132, 140, 5


def test_with_the_gaussian_window(dfx, oracle):
    frames = _frames(W2, H2, SEED2)
    ref = _ref(oracle, (W2, H2, SEED2), frames, window="gaussian", num_levels=2, num_iters=3, win_size=15)
    with dfx.FlowEngine(W2, H2, "farn", max_batch=2, farn_num_levels=2, farn_num_iters=3, farn_window=1, farn_win_size=15,
                        **FAST) as eng:
        _same(eng.calc_optflows(frames, 1), ref, "Gaussian winSize 15")


def test_with_poly_n_7(dfx, oracle):
    frames = _frames(W2, H2, SEED2)
    ref = _ref(oracle, (W2, H2, SEED2), frames, num_levels=2, num_iters=3, poly_n=7, poly_sigma=1.5)
    with dfx.FlowEngine(W2, H2, "farn", max_batch=2, farn_num_levels=2, farn_num_iters=3, farn_poly_n=7, farn_poly_sigma=1.5,
                        **FAST) as eng:
        _same(eng.calc_optflows(frames, 1), ref, "polyN 7")


@pytest.mark.parametrize("win", [5, 23])
def test_with_the_generic_routes_windows(dfx, oracle, win):
    frames = _frames(W2, H2, SEED2)
    ref = _ref(oracle, (W2, H2, SEED2), frames, num_levels=2, num_iters=3, win_size=win)
    with dfx.FlowEngine(W2, H2, "farn", max_batch=2, farn_num_levels=2, farn_num_iters=3, farn_win_size=win, **FAST) as eng:
        _same(eng.calc_optflows(frames, 1), ref, f"winSize {win}")


def test_with_an_initial_flow(dfx, oracle):
    """The seed of a pair is the default path's flow of that pair: interleaved host arrays, then the device form with the
    seed buffer being the output buffer."""
    import torch

    frames = _frames(W2, H2, SEED2)
    fields = dict(num_levels=2, num_iters=3)
    seeds = _ref(oracle, (W2, H2, SEED2), frames, fast=False, **fields)
    ref = _ref(oracle, (W2, H2, SEED2), frames, seeds=seeds, **fields)
    plain = _ref(oracle, (W2, H2, SEED2), frames, **fields)
    assert not np.array_equal(ref[0], plain[0])
    with dfx.FlowEngine(W2, H2, "farn", max_batch=2, farn_num_levels=2, farn_num_iters=3, **FAST) as eng:
        _same(eng.calc_optflows(frames, 1, init=seeds), ref, "seeded")
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.from_numpy(np.stack(seeds)).cuda()
        torch.cuda.synchronize()
        eng.calc_optflows_device(d_frames.data_ptr(), W2, W2 * H2, 4, 1, buf.data_ptr(), W2 * H2 * 2, init=buf.data_ptr())
        assert np.array_equal(buf.cpu().numpy(), np.stack(ref)), "device form, in place"
        _same(eng.calc_optflows(frames, 1), plain, "unseeded after seeded")


def test_on_unrelated_frames(dfx, oracle):
    """Two textures and a noise frame (as tests/test_farneback_window_gpu.py has them): large, erratic flows through pyrUp."""
    from denseflow_amd import engine as E

    w, h = 256, 128
    noise = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)
    frames = [SynthClip(w, h, 31).frame(0), SynthClip(w, h, 32).frame(5), noise, SynthClip(w, h, 31).frame(40)]
    ref = _ref(oracle, ("unrelated", w, h), frames, num_levels=2)
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_num_levels=2, **FAST) as eng:
        out = eng.calc_optflows(frames, 1)
    assert max(float(np.abs(f).max()) for f in out) > 8.0, "the case is meant to produce flows of many pixels"
    _same(out, ref, "unrelated frames")
    with dfx.FlowEngine(w, h, "farn", max_batch=2, farn_num_levels=2, variant=E.VAR_FARN_M_IN_HBM, **FAST) as eng:
        _same(eng.calc_optflows(frames, 1), ref, "unrelated frames, M in HBM")


# ------------------------------------------------------------------------------------------------ outputs

@pytest.mark.parametrize("iters", [1, 3])  # 1: level 0's only launch is the planar one, on the pyrUp'd flow
@pytest.mark.parametrize("bound", [None, 20.0])
def test_planar_output_is_the_interleaved_output(dfx, oracle, iters, bound):
    from denseflow_amd import engine as E

    frames = _frames(W2, H2, SEED2)
    ref = _ref(oracle, (W2, H2, SEED2), frames, num_levels=2, num_iters=iters)
    want = np.stack(ref).transpose(0, 3, 1, 2)
    if bound is not None:
        want = np.clip(want, -bound, bound).astype(np.float32) / np.float32(bound)
    want = np.ascontiguousarray(want).view(np.uint32)
    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM), dict(farn_num_levels=0)):
        kw = dict(dict(max_batch=2, farn_num_levels=2, farn_num_iters=iters, **FAST), **knobs)
        with dfx.FlowEngine(W2, H2, "farn", **kw) as eng:
            inter = eng.calc_optflows(frames, 1)
            got = eng.calc_optflows_planar(frames, 1, bound=bound)
        if kw["farn_num_levels"] == 2:
            _same(inter, ref, f"interleaved, {knobs}")
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want), knobs
        else:  # one level: the INIT launch and the merge kernel
            w0 = np.stack(inter).transpose(0, 3, 1, 2)
            if bound is not None:
                w0 = np.clip(w0, -bound, bound).astype(np.float32) / np.float32(bound)
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(w0).view(np.uint32)), knobs


def test_u8_output_is_the_oracles_quantiser(dfx, oracle):
    frames = _frames(W2, H2, SEED2)
    ref = _ref(oracle, (W2, H2, SEED2), frames, num_levels=2, num_iters=3)
    with dfx.FlowEngine(W2, H2, "farn", max_batch=2, farn_num_levels=2, farn_num_iters=3, **FAST) as eng:
        img_x, img_y = eng.calc_optflows_u8(frames, 1, 20)
    assert len(img_x) == len(img_y) == len(ref)
    for i, flow in enumerate(ref):
        ox, oy = oracle.flow_to_u8(flow, -20, 20)
        assert np.array_equal(img_x[i], ox) and np.array_equal(img_y[i], oy), i


# ------------------------------------------------------------------------------------------------ re-planning, memory

def test_set_size_gives_the_bits_of_a_fresh_handle_and_a_refused_size_changes_nothing(dfx, oracle):
    kw = dict(max_batch=2, farn_num_levels=2, farn_num_iters=3, **FAST)
    sizes = [(224, 160), (132, 140), (224, 160)]
    fresh = {}
    for w, h in set(sizes):
        with dfx.FlowEngine(w, h, "farn", **kw) as eng:
            fresh[(w, h)] = eng.calc_optflows(_frames(w, h, 77), 1)
        _same(fresh[(w, h)], _ref(oracle, (w, h, 77), _frames(w, h, 77), num_levels=2, num_iters=3), f"fresh handle {w}x{h}")
    held = []
    with dfx.FlowEngine(*sizes[0], "farn", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            _same(eng.calc_optflows(_frames(w, h, 77), 1), fresh[(w, h)], f"after set_size({w}, {h})")
            held.append(eng.device_bytes())  # read once the stop has computed its flows (frame slots, staging)
        assert held[2] == held[0], held
        with pytest.raises(dfx.DfxError) as e:
            eng.set_size(130, 132)  # 65 x 66 is level 1 of 2
        assert e.value.status == UNSUPPORTED and "up to 1" in str(e.value)
        _same(eng.calc_optflows(_frames(224, 160, 77), 1), fresh[(224, 160)], "after the refused set_size")
        assert eng.device_bytes() == held[0]


def test_a_fast_handle_holds_no_more_than_a_default_handle(dfx):
    from denseflow_amd import engine as E

    for knobs in (dict(), dict(variant=E.VAR_FARN_M_IN_HBM)):
        with dfx.FlowEngine(224, 160, "farn", max_batch=2, **knobs) as eng:
            default = eng.device_bytes()
        with dfx.FlowEngine(224, 160, "farn", max_batch=2, **FAST, **knobs) as eng:
            fast = eng.device_bytes()
        assert fast <= default, (fast, default, knobs)


# ------------------------------------------------------------------------------------------------ refusals

@pytest.mark.parametrize("w,h,kw,status,text", [
    (128, 96, dict(farn_fast_pyramids=2), INVALID, "farn_fast_pyramids"),
    (128, 96, dict(farn_fast_pyramids=-1), INVALID, "farn_fast_pyramids"),
    (128, 96, dict(farn_fast_pyramids=1, farn_pyr_scale=0.6), INVALID, "farn_pyr_scale"),
    (130, 132, dict(farn_fast_pyramids=1, farn_num_levels=2), UNSUPPORTED, "up to 1"),
    (1920, 1080, dict(farn_fast_pyramids=1, farn_num_levels=5), UNSUPPORTED, "up to 3"),
])
def test_refused_parameters(dfx, w, h, kw, status, text):
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(w, h, "farn", max_batch=1, **kw)
    assert e.value.status == status and text in str(e.value), str(e.value)


def test_1080p_at_three_levels_creates(dfx):
    with dfx.FlowEngine(1920, 1080, "farn", max_batch=1, farn_num_levels=3, **FAST) as eng:
        assert eng.device_bytes() > 0
    with dfx.FlowEngine(1921, 1081, "farn", max_batch=1, farn_num_levels=0, **FAST) as eng:  # any size at 0 levels
        assert eng.device_bytes() > 0


# ------------------------------------------------------------------------------------------------ the default path is untouched

def test_the_default_path_after_a_fast_handle_is_still_the_oracles_bits(dfx, oracle):
    w, h = 224, 224
    clip = SynthClip(w, h, 1)
    f0, f1 = clip.frame(0), clip.frame(1)
    want = oracle.farneback_calc(f0, f1)
    with dfx.FlowEngine(w, h, "farn", **FAST) as eng:
        fast = eng.calc(f0, f1)
    assert np.isfinite(fast).all() and not np.array_equal(fast, want)
    assert np.array_equal(fast, FR.farneback_flow(oracle, f0, f1, None, fast=True))
    with dfx.FlowEngine(w, h, "farn") as eng:
        assert np.array_equal(eng.calc(f0, f1), want)
    with dfx.FlowEngine(w, h, "farn", farn_fast_pyramids=0) as eng:
        assert np.array_equal(eng.calc(f0, f1), want)


def test_the_flag_is_ignored_by_tvl1(dfx):
    f0, f1 = _frames(96, 64, 5, 2)
    with dfx.FlowEngine(96, 64, "tvl1") as eng:
        want = eng.calc(f0, f1)
    with dfx.FlowEngine(96, 64, "tvl1", farn_fast_pyramids=1, farn_pyr_scale=0.6) as eng:
        assert np.array_equal(eng.calc(f0, f1), want)
