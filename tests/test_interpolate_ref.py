"""Properties of the NumPy restatement of the frame interpolation (tests/interpolate_ref.py): the vectorised form equals the
scalar loop in every bit over both flow forms, masks, passes, window sizes, times and channel counts; zero flows give the
plain blend with source 0 everywhere, a flow that leaves the frame everywhere gives the same values with source 3; a
one-sided disocclusion between two constant-flow layers is taken from the frame that shows it; the second tier never shows
without fill passes.  Quality, asserted as conditions: on SynthClip(97, 61, 9) 0, 2 -> 1 the interpolated frame's mean
absolute error is below half the plain blend's with the exact flows and with the CPU oracle's TVL1 and Farneback flows, on
HardClip(130, 97, 5) 0, 2 -> 1 it is below the blend's, and the share of pixels that fall back to the blend is at most 1 %
with 3 passes.  The figures themselves are printed (profiles/interpolate/quality.txt holds the printed lines).  No GPU is
touched."""
import itertools

import numpy as np
import pytest

from denseflow_amd.synth import HardClip, SynthClip
from tests import flow_project_ref as P
from tests import interpolate_ref as R
from tests.fb_check_ref import fb_check

F32 = np.float32
TS = (0.5, 0.25, 0.7)


def _planes(flow_hw2):
    return np.ascontiguousarray(np.moveaxis(np.asarray(flow_hw2, F32), -1, 0))


def _inputs(w, h, channels, seed=500):
    """(img0, img1, fwd, bwd, occ_fwd, occ_bwd) of one pair: random bytes, smooth flows of a few pixels, a tenth masked."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    shape = (h, w) if channels == 1 else (h, w, channels)
    img0, img1 = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    flows, _, occ = P.project_inputs(w, h, n=2, seed=seed)
    return img0, img1, flows[0], flows[1], occ[0], occ[1]


def _both_forms(args, kw):
    a, b = R.interpolate(*args, **kw), R.interpolate_loop(*args, **kw)
    assert R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1]), kw
    assert a[0].dtype == F32 and a[1].dtype == np.uint8 and a[1].max() <= 6 and not (a[1] == 7).any()
    return a


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("bidir,masks", [(False, False), (False, True), (True, False), (True, True)])
def test_the_vectorised_form_equals_the_scalar_loop(channels, bidir, masks):
    w, h = 13, 9
    img0, img1, fwd, bwd, of, ob = _inputs(w, h, channels)
    fwd = fwd.copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0)):
        fwd[k % 2].reshape(-1)[(5 * k + 2) % (w * h)] = F32(v)
    for passes, ksize, t in itertools.product((0, 1, 3), (3, 5), TS):
        kw = dict(t=t, fill_passes=passes, ksize=ksize, occ_fwd=of if masks else None, occ_bwd=ob if masks and bidir else None)
        _both_forms((img0, img1, fwd, bwd if bidir else None), kw)


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (5, 1), (23, 17)])
def test_the_two_forms_agree_at_other_sizes(w, h):
    for channels, bidir in ((1, True), (3, False)):
        img0, img1, fwd, bwd, of, ob = _inputs(w, h, channels)
        for passes, ksize, t, mw in ((0, 3, 0.5, 0.25), (2, 5, 0.25, 0.0), (3, 3, 0.7, 1.0)):
            kw = dict(t=t, fill_passes=passes, ksize=ksize, min_weight=mw, occ_fwd=of, occ_bwd=ob if bidir else None)
            _both_forms((img0, img1, fwd, bwd if bidir else None), kw)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("t", TS)
def test_zero_flows_give_the_plain_blend_from_both_frames(channels, t):
    img0, img1, *_ = _inputs(29, 11, channels)
    z = np.zeros((2, 11, 29), F32)
    for bwd in (None, z):
        o, source = R.interpolate(img0, img1, z, bwd, t=t)
        assert np.array_equal(R.stored(o, "uint8"), R.plain_blend(img0, img1, t)) and (source == 0).all()


@pytest.mark.parametrize("passes", [0, 3])
def test_a_flow_that_leaves_the_frame_everywhere_falls_back_to_the_blend(passes):
    img0, img1, *_ = _inputs(29, 11, 3)
    far = np.full((2, 11, 29), 1e4, F32)
    for bwd in (None, -far):
        o, source = R.interpolate(img0, img1, far, bwd, t=0.25, fill_passes=passes)
        assert np.array_equal(R.stored(o, "uint8"), R.plain_blend(img0, img1, 0.25)) and (source == 3).all()


def test_a_one_sided_disocclusion_is_taken_from_the_frame_that_shows_it():
    """A static background and a foreground block of 8 columns that moves 8 px to the right between the frames.  At t = 0.5
    the block is at columns 20 .. 27.  Columns 16 .. 19 are behind the block in frame 0 and visible in frame 1: nothing of
    F01 lands there (a hole of the forward projection), the background of F10 does, so they come from frame 1 alone; columns
    28 .. 31 are visible in frame 0 only and come from frame 0 alone.  Both show the background's own bytes."""
    w, h = 48, 8
    rng = np.random.default_rng(5)
    bg, fg = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, 8), dtype=np.uint8)
    img0, img1 = bg.copy(), bg.copy()
    img0[:, 16:24], img1[:, 24:32] = fg, fg
    fwd, bwd = np.zeros((2, h, w), F32), np.zeros((2, h, w), F32)
    fwd[0, :, 16:24], bwd[0, :, 24:32] = 8.0, -8.0
    for passes in (0, 3):
        o, source = R.interpolate(img0, img1, fwd, bwd, t=0.5, fill_passes=passes)
        q = R.stored(o, "uint8")
        assert (source[:, 16:20] == 2).all() and np.array_equal(q[:, 16:20], bg[:, 16:20])
        assert (source[:, 28:32] == 1).all() and np.array_equal(q[:, 28:32], bg[:, 28:32])
        assert (source[:, :16] == 0).all() and (source[:, 32:] == 0).all() and np.array_equal(q[:, :16], bg[:, :16])
    # with the forward flow alone both projections have the hole: only the filled flows reach it, as the second tier
    o, source = R.interpolate(img0, img1, fwd, None, t=0.5, fill_passes=0)
    assert (source[:, 16:20] == 3).all()
    o, source = R.interpolate(img0, img1, fwd, None, t=0.5, fill_passes=3)
    assert (source[:, 16:20] >= 4).all() and (source[:, 16:20] != 7).all()


def test_the_second_tier_never_shows_without_fill_passes():
    img0, img1, fwd, bwd, of, ob = _inputs(41, 23, 1)
    fwd = fwd * F32(3)  # more holes
    for b, masks in ((None, False), (bwd * F32(3), True)):
        _, source = R.interpolate(img0, img1, fwd, b, fill_passes=0, occ_fwd=of if masks else None, occ_bwd=ob if masks else None)
        assert (source <= 3).all() and (source == 3).any()
        _, source = R.interpolate(img0, img1, fwd, b, fill_passes=3, occ_fwd=of if masks else None, occ_bwd=ob if masks else None)
        assert (source >= 4).any() and not (source == 7).any()


# ---- quality: the held-out middle frame -----------------------------------------------------------------------------------
def _record(name, frames, fwd, bwd, truth, passes=3, masks=False):
    """(interpolated error, blend error, fallback share) in grey levels against the true middle frame; prints the line."""
    f0, f1 = frames
    of = fb_check(fwd, bwd)[0] if masks else None
    ob = fb_check(bwd, fwd)[0] if masks else None
    o, source = R.interpolate(f0, f1, fwd, bwd, t=0.5, fill_passes=passes, occ_fwd=of, occ_bwd=ob if bwd is not None else None)
    err = R.mean_abs_error(R.stored(o, "uint8"), truth)
    blend = R.mean_abs_error(R.plain_blend(f0, f1, 0.5), truth)
    share = float((source == 3).mean())
    print(f"{name}, {'both directions' if bwd is not None else 'forward only'}, {passes} passes: interpolated {err:.3f}, plain blend "
          f"{blend:.3f} grey levels (ratio {err / blend:.3f}); fallback share {share:.4f}; second tier {float((source >= 4).mean()):.4f}")
    return err, blend, share


def test_quality_on_the_synthetic_clip_with_the_exact_flows():
    clip = SynthClip(97, 61, 9)
    frames, truth = (clip.frame(0), clip.frame(2)), clip.frame(1)
    fwd, bwd = _planes(clip.true_flow(0, 2)), _planes(clip.true_flow(2, 0))
    for b, passes in ((bwd, 0), (bwd, 2), (bwd, 3), (bwd, 6), (None, 0), (None, 2), (None, 3)):
        err, blend, share = _record("SynthClip(97, 61, 9) 0, 2 -> 1, exact flows", frames, fwd, b, truth, passes)
        assert err < 0.5 * blend
        if passes == 3:
            assert share <= 0.01


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_quality_on_the_synthetic_clip_with_the_oracles_flows(oracle, algo):
    clip = SynthClip(97, 61, 9)
    calc = getattr(oracle, algo)
    frames, truth = (clip.frame(0), clip.frame(2)), clip.frame(1)
    fwd, bwd = _planes(calc(*frames)), _planes(calc(frames[1], frames[0]))
    err, blend, share = _record(f"SynthClip(97, 61, 9) 0, 2 -> 1, oracle {algo}", frames, fwd, bwd, truth)
    assert err < 0.5 * blend and share <= 0.01
    for passes in (0, 3):
        _record(f"SynthClip(97, 61, 9) 0, 2 -> 1, oracle {algo}", frames, fwd, None, truth, passes)
    # a longer baseline, recorded only
    frames6 = (clip.frame(0), clip.frame(6))
    fwd6, bwd6 = _planes(calc(*frames6)), _planes(calc(frames6[1], frames6[0]))
    _record(f"SynthClip(97, 61, 9) 0, 6 -> 3, oracle {algo}", frames6, fwd6, bwd6, clip.frame(3))


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_quality_on_the_hard_clip_with_the_oracles_flows(oracle, algo):
    clip = HardClip(130, 97, 5)
    calc = getattr(oracle, algo)
    frames, truth = (clip.frame(0), clip.frame(2)), clip.frame(1)
    fwd, bwd = _planes(calc(*frames)), _planes(calc(frames[1], frames[0]))
    err, blend, share = _record(f"HardClip(130, 97, 5) 0, 2 -> 1, oracle {algo}", frames, fwd, bwd, truth)
    assert err < blend and share <= 0.01
