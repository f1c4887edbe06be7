"""The NumPy reference of the forward-backward check (tests/fb_check_ref.py) against itself and against what the check is
for: its scalar loop equals its vectorised form, its edge cases are the ones include/dfx.h states, and on the CPU oracle's
flows of a real pair the mask discriminates — so the device tests, which compare with this reference, cannot pass on an
all-0 or all-1 mask.  No GPU and no engine is touched here."""
import numpy as np
import pytest

from denseflow_amd.synth import HardClip, SynthClip
from tests import fb_check_ref as R

F32 = np.float32


def _planes(flow):  # (H, W, 2) of the oracle -> (2, H, W)
    return np.ascontiguousarray(flow.transpose(2, 0, 1))


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (17, 9), (40, 23)])
def test_the_loop_equals_the_vectorised_form(w, h):
    rng = np.random.default_rng(w * 100 + h)
    fwd, bwd = R.smooth_flow(rng, 2, h, w, 0.8 * w), R.smooth_flow(rng, 2, h, w, 0.8 * w)
    R.plant_specials(fwd[1], bwd[1])
    for i in range(2):
        for a1, a2 in ((R.ALPHA1, R.ALPHA2), (0.0, 0.0), (0.3, 2.0)):
            occ, err = R.fb_check(fwd[i], bwd[i], a1, a2)
            occ_l, err_l = R.fb_check_loop(fwd[i], bwd[i], a1, a2)
            assert occ.dtype == np.uint8 and err.dtype == F32 and occ.shape == err.shape == (h, w)
            assert np.array_equal(occ, occ_l)
            assert np.array_equal(err.view(np.uint32), err_l.view(np.uint32))
        assert set(np.unique(occ)) <= {0, 1}


@pytest.mark.parametrize("d", [0.0, 1.0, 2.5, 7.0, -3.25])
def test_a_constant_translation_is_consistent_where_it_stays_inside(d):
    w, h = 23, 11
    fwd, bwd = np.zeros((2, h, w), F32), np.zeros((2, h, w), F32)
    fwd[0], bwd[0] = d, -d
    occ, err = R.fb_check(fwd, bwd)
    x = np.arange(w, dtype=F32)
    stays = np.broadcast_to((x + F32(d) >= 0) & (x + F32(d) <= w - 1), (h, w))
    assert np.array_equal(occ, (~stays).astype(np.uint8))
    assert np.all(err[stays] == 0) and np.all(np.isposinf(err[~stays]))


def test_nan_inf_and_huge_flows_are_occluded_and_never_converted():
    w, h = 9, 7
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for plane in (0, 1):
            fwd, bwd = np.zeros((2, h, w), F32), np.zeros((2, h, w), F32)
            fwd[plane, 3, 4] = bad
            for f in (R.fb_check, R.fb_check_loop):
                occ, err = f(fwd, bwd)
                assert occ[3, 4] == 1 and np.isposinf(err[3, 4]), (bad, plane)
                assert occ.sum() == 1
    # a NaN in the flow that is sampled: inside, err NaN, occluded
    fwd, bwd = np.zeros((2, h, w), F32), np.zeros((2, h, w), F32)
    bwd[1, 2, 2] = np.nan
    occ, err = R.fb_check(fwd, bwd)
    assert occ[2, 2] == 1 and np.isnan(err[2, 2])


def test_the_last_column_and_row_are_inside_and_the_taps_clamp():
    w, h = 8, 5
    rng = np.random.default_rng(5)
    bwd = rng.uniform(-1, 1, (2, h, w)).astype(F32)
    fwd = np.zeros((2, h, w), F32)
    fwd[0, 1, 2], fwd[1, 1, 2] = w - 1 - 2, 0       # px exactly W - 1
    fwd[0, 2, 3], fwd[1, 2, 3] = 0, h - 1 - 2       # py exactly H - 1
    fwd[0, 0, 0], fwd[1, 0, 0] = w - 1, h - 1       # both
    occ, err = R.fb_check(fwd, bwd, 0.0, 1e9)
    for (x, y), (tx, ty) in {(2, 1): (w - 1, 1), (3, 2): (3, h - 1), (0, 0): (w - 1, h - 1)}.items():
        # ax = ay = 0 and x1 / y1 clamp onto x0 / y0: the sample is the tap itself
        du, dv = fwd[0, y, x] + bwd[0, ty, tx], fwd[1, y, x] + bwd[1, ty, tx]
        assert occ[y, x] == 0 and err[y, x] == du * du + dv * dv, (x, y)
    fwd[0, 1, 2] = np.nextafter(F32(w - 1 - 2), F32(np.inf))  # one ulp further: px > W - 1
    occ, err = R.fb_check(fwd, bwd, 0.0, 1e9)
    assert occ[1, 2] == 1 and np.isposinf(err[1, 2])


def test_negative_zero_is_inside():
    fwd, bwd = np.zeros((2, 3, 4), F32), np.zeros((2, 3, 4), F32)
    fwd[:] = F32(-0.0)
    for f in (R.fb_check, R.fb_check_loop):
        occ, err = f(fwd, bwd)
        assert not occ.any() and np.all(err == 0)


@pytest.mark.parametrize("d", [1.3, 0.7, 2.0])
def test_the_threshold_edge(d):
    w, h = 12, 4
    d = F32(d)
    fwd, bwd = np.zeros((2, h, w), F32), np.zeros((2, h, w), F32)
    fwd[0] = d
    inside = ~R.out_of_frame(fwd)
    assert inside.any()
    at = F32(d * d)
    occ, err = R.fb_check(fwd, bwd, 0.0, at)
    assert np.all(err[inside] == at) and not occ[inside].any()      # err <= thr holds with equality
    occ, _ = R.fb_check(fwd, bwd, 0.0, np.nextafter(at, F32(0)))
    assert occ[inside].all()                                          # one ulp below: occluded


def _shares(fwd, bwd):
    occ, _ = R.fb_check(fwd, bwd)
    out = R.out_of_frame(fwd)
    return float(occ.mean()), float(out.mean()), float((occ.astype(bool) & ~out).mean())


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_the_mask_discriminates_on_the_oracles_flows(oracle, algo):
    clip = SynthClip(97, 61, 9)
    a, b = clip.frame(0), clip.frame(6)
    calc = getattr(oracle, algo)
    fwd, bwd = _planes(calc(a, b)), _planes(calc(b, a))
    for f, g in ((fwd, bwd), (bwd, fwd)):
        occ, out, occ_in = _shares(f, g)
        print(f"{algo} SynthClip(97, 61, 9) 0 <-> 6: occluded {occ:.3f}, out of frame {out:.3f}, in frame and occluded {occ_in:.3f}")
        assert 0.005 <= occ_in <= 0.5
        assert occ < 1.0 and out < occ
    hard = HardClip(130, 97, 5)
    a, b = hard.frame(0), hard.frame(2)
    occ, out, occ_in = _shares(_planes(calc(a, b)), _planes(calc(b, a)))
    print(f"{algo} HardClip(130, 97, 5) 0 -> 2: occluded {occ:.3f}, out of frame {out:.3f}, in frame and occluded {occ_in:.3f}")
    assert 0.0 < occ < 1.0
