"""The NumPy statement of the global-motion arithmetic (tests/global_motion_ref.py) recovers a known camera (no GPU).  The
background flow is SynthClip's exact flow over dt frames (a rotation plus a translation: exactly affine); over it lies a
rectangle of `fg` of the area moving by (-2.25, 1.25) * dt, plus Gaussian noise.  Flows are composed, not estimated, so the
CPU oracle is not needed for the assertions; one recorded line applies the fit to the oracle's TVL1 flow of a SynthClip
pair.  The model error is the largest distance, in pixels, between the fitted and the true camera flow over the
background."""
import numpy as np
import pytest

from tests import global_motion_ref as R

# (W, H, seed, dt, fg, sigma) -> (inlier counts of the five rounds or None, recorded error in px)
CASES = {
    (97, 61, 9, 6, 0.30, 0.05): ([5917, 5809, 4065, 4168, 4168], 0.0037),
    (97, 61, 9, 6, 0.45, 0.05): ([5917, 5917, 1607, 3317, 3317], 0.0028),
    (130, 97, 5, 2, 0.30, 0.1): (None, 0.0051),
    (61, 33, 2, 3, 0.30, 0.05): (None, 0.0086),
}
FIRST = (97, 61, 9, 6, 0.30, 0.05)

_cache = {}


def _case(key):
    if key not in _cache:
        flow, back, bg = R.synth_case(*key)
        for a in (flow, back, bg):
            a.setflags(write=False)
        _cache[key] = (flow, back, bg)
    return _cache[key]


def _model_error(res, back, bg):
    h, w = back.shape
    d = R.camera_flow(res["a"], w, h) - bg
    return float(np.hypot(d[0], d[1])[back].max())


@pytest.mark.parametrize("key", list(CASES))
def test_the_robust_affine_fit_recovers_the_camera(key):
    flow, back, bg = _case(key)
    counts, recorded = CASES[key]
    res = R.global_motion(flow)  # thr 0.5, growth 2, rounds 5, affine
    err = _model_error(res, back, bg)
    print(f"{key}: inliers {[int(c) for c in res['inliers'][:5]]} background {int(back.sum())} error {err:.4f} px")
    assert res["status"] == 0 and res["valid"] == flow.shape[1] * flow.shape[2]
    if counts is not None:
        assert [int(c) for c in res["inliers"][:5]] == counts
        assert counts[-1] == int(back.sum())  # the last round's inliers are the background exactly
        assert np.array_equal(res["moving"] == 0, back)
    assert np.all(res["inliers"][5:] == 0)
    assert err < 0.01 and abs(err - recorded) < 5e-5, err
    # the compensated flow of the background is the noise; the foreground keeps its motion relative to the camera
    assert float(np.hypot(*res["out"])[back].max()) < 0.5
    assert float(np.hypot(*res["out"])[~back].min()) > 0.5


def test_the_robust_fit_beats_plain_least_squares_by_100x():
    flow, back, bg = _case(FIRST)
    plain = _model_error(R.global_motion(flow, rounds=1), back, bg)
    robust = _model_error(R.global_motion(flow), back, bg)
    print(f"plain least squares {plain:.4f} px, five rounds {robust:.4f} px")
    assert abs(plain - 2.04) < 0.005
    assert robust * 100.0 <= plain


def test_three_rounds_lose_every_inlier_and_keep_the_first_model():
    flow, back, bg = _case(FIRST)
    res, first = R.global_motion(flow, rounds=3, growth=2.0), R.global_motion(flow, rounds=1)
    assert res["status"] == 6 and [int(c) for c in res["inliers"][:3]] == [5917, 0, 0]
    assert np.array_equal(res["a"].view(np.uint64), first["a"].view(np.uint64))
    assert np.array_equal(res["p"].view(np.uint32), first["p"].view(np.uint32))
    assert np.all(res["sums"] == 0)


def test_the_foreground_as_the_mask_and_one_round_equal_five_rounds():
    flow, back, bg = _case(FIRST)
    masked = R.global_motion(flow, mask=(~back).astype(np.uint8), rounds=1)
    five = R.global_motion(flow)
    assert masked["valid"] == back.sum() == masked["inliers"][0]
    assert np.array_equal(masked["sums"], five["sums"])  # the same pixels: the same integers, hence the same model
    assert np.array_equal(masked["a"].view(np.uint64), five["a"].view(np.uint64))
    err = _model_error(masked, back, bg)
    assert abs(err - 0.0037) < 5e-5


@pytest.mark.parametrize("key", list(CASES))
def test_the_closed_form_solve_agrees_with_linalg_solve(key):
    flow, back, bg = _case(key)
    res = R.global_motion(flow)
    S1, Sx, Sy, Sxx, Sxy, Syy, Su, Sxu, Syu, Sv, Sxv, Syv = (float(int(s)) for s in res["sums"])
    N = np.array([[S1, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]])
    want = np.concatenate([np.linalg.solve(N, np.array([Su, Sxu, Syu])), np.linalg.solve(N, np.array([Sv, Sxv, Syv]))]) / 256.0
    assert np.all(np.abs(res["P"] - want) <= 1e-9 * np.abs(want).max())
    # and the translation model is the mean of the fixed-point samples
    tr = R.global_motion(flow, model=R.TRANSLATION, rounds=1)
    s = tr["sums"]
    assert tr["P"][0] == int(s[6]) / int(s[0]) / 256.0 and tr["P"][3] == int(s[9]) / int(s[0]) / 256.0
    assert np.all(tr["P"][[1, 2, 4, 5]] == 0)


def test_the_pixel_origin_form_is_the_centred_model():
    flow, back, bg = _case(FIRST)
    res = R.global_motion(flow)
    h, w = back.shape
    xc, yc = R.coords(w, h)
    P = res["P"]
    centred = np.stack([P[0] + P[1] * xc + P[2] * yc, P[3] + P[4] * xc + P[5] * yc])
    assert np.abs(R.camera_flow(res["a"], w, h) - centred).max() < 1e-12


def test_excluded_values_and_degenerate_inputs():
    flow = np.array(_case(FIRST)[0])
    flow[0, 3, 5], flow[1, 7, 9], flow[0, 11, 2], flow[1, 0, 0] = np.nan, np.inf, 5000.0, -4096.0
    res = R.global_motion(flow)
    assert res["valid"] == flow[0].size - 4
    assert np.isnan(res["out"][0, 3, 5]) and res["moving"][3, 5] == 1 and res["moving"][0, 0] == 1
    none = R.global_motion(np.full((2, 4, 6), np.nan, np.float32), rounds=2)
    assert none["status"] == 3 and none["valid"] == 0 and np.all(none["a"] == 0) and np.all(none["moving"] == 1)
    line = np.zeros((2, 1, 9), np.float32)  # one row: the affine normal matrix is singular, a translation is not
    assert R.global_motion(line, rounds=1)["status"] == 1
    assert R.global_motion(line, rounds=1, model=R.TRANSLATION)["status"] == 0
    assert [float(t) for t in R.thresholds(0.5, 2.0, 5)] == [8.0, 4.0, 2.0, 1.0, 0.5]


def test_record_the_fit_on_the_oracles_tvl1_flow():
    """Recorded, not asserted beyond sanity: the camera of a SynthClip pair from the CPU oracle's TVL1 flow."""
    from denseflow_amd.synth import SynthClip
    from oracle import oracle_py

    w, h = 97, 61
    clip = SynthClip(w, h, 9)
    flow = np.ascontiguousarray(oracle_py.tvl1_calc(clip.frame(0), clip.frame(1)).transpose(2, 0, 1))
    bg = clip.true_flow(0, 1).astype(np.float64).transpose(2, 0, 1)
    res = R.global_motion(flow)
    d = R.camera_flow(res["a"], w, h) - bg
    print(f"oracle TVL1 flow {w}x{h}: a = {np.round(res['a'], 5)}, inliers {[int(c) for c in res['inliers'][:5]]}, "
          f"model error {np.hypot(d[0], d[1]).max():.4f} px, moving share {res['moving'].mean():.3f}")
    assert res["status"] == 0
