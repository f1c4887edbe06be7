"""The reference of the flow chain (tests/flow_chain_ref.py) against itself and against what a chain must be: the vectorised
form equals the scalar loop on random and special inputs; one link is the flow itself; the exact flows of SynthClip chained
over six links are the exact long-range flow to float rounding; hop -1 over the reversed list is hop 1; emit "all" holds the
last link's result as its last flow; occlusion at link 0 is occ[y][x].  The quality record (the chain of the CPU oracle's
adjacent flows against the oracle's direct long-range estimate) is printed, not asserted.  No GPU is touched."""
import math

import numpy as np
import pytest

from denseflow_amd.synth import ROTATION_DEG, SynthClip
from tests import flow_chain_ref as R
from tests.fb_check_ref import smooth_flow
from tests.warp_ref import plant_specials

F32, U32 = np.float32, np.uint32


def _planes(flow_hw2):
    return np.ascontiguousarray(np.moveaxis(np.asarray(flow_hw2, F32), -1, 0))


def _random_bits(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32).view(F32)


def _inputs(rng, kind, n, h, w):
    if kind == "smooth":
        return smooth_flow(rng, n, h, w, 3.0)
    if kind == "specials":
        f = smooth_flow(rng, n, h, w, 3.0)
        plant_specials(f[0])
        plant_specials(f[n // 2])
        return f
    if kind == "subnormal":
        return (smooth_flow(rng, n, h, w, 3.0).astype(np.float64) * 1e-39).astype(F32)
    return _random_bits(rng, (n, 2, h, w))


@pytest.mark.parametrize("kind", ["smooth", "specials", "subnormal", "bits"])
@pytest.mark.parametrize("border", R.BORDERS)
def test_the_vectorised_form_equals_the_scalar_loop(kind, border):
    rng = np.random.default_rng(480)
    for w, h in ((13, 9), (1, 1), (2, 3), (5, 1), (1, 7)):
        flows = _inputs(rng, kind, 4, h, w)
        if kind == "subnormal":
            assert (np.abs(flows[flows != 0]) < 1.2e-38).all()
        occ = R.sparse_mask(rng, 4, h, w, 0.1)
        for o in (None, occ):
            a, va = R.chain(flows, 4, 0, 1, border, o)
            b, vb = R.chain_loop(flows, 4, 0, 1, border, o)
            assert R.same_bits(a, b) and np.array_equal(va, vb), (kind, border, w, h, o is not None)


def test_same_bits_is_equal_patterns_and_nan_for_nan():
    want = np.array([1.0, -0.0, np.nan, np.inf], F32)
    assert R.same_bits(want.copy(), want)
    other_nan = want.copy()
    other_nan.view(U32)[2] = 0xFFC00001  # another sign and payload
    assert R.same_bits(other_nan, want)
    assert not R.same_bits(np.array([1.0, 0.0, np.nan, np.inf], F32), want)   # +0 is not -0
    assert not R.same_bits(np.array([1.0, -0.0, 1.0, np.inf], F32), want)     # a number is not NaN
    assert not R.same_bits(np.array([np.nan, -0.0, np.nan, np.inf], F32), want)


def test_one_link_is_the_flow_itself_wherever_its_taps_are_finite():
    rng = np.random.default_rng(1)
    flows = _inputs(rng, "specials", 3, 11, 17)
    for border in R.BORDERS:
        out, valid = R.chain(flows, 1, 0, 1, border)
        assert valid.all()  # link 0 samples the pixel itself: always inside
        f = flows[0]
        right, below = np.minimum(np.arange(17) + 1, 16), np.minimum(np.arange(11) + 1, 10)
        fin = np.isfinite(f) & np.isfinite(f[:, :, right]) & np.isfinite(f[:, below]) & np.isfinite(f[:, below][:, :, right])
        assert fin.mean() > 0.8 and not fin.all()
        assert np.array_equal(out[0][fin], f[fin])        # numerically: -0 comes out as +0 (0 + -0)
        assert not np.signbit(out[0][fin & (f == 0)]).any()
        assert np.isnan(out[0][~np.isfinite(f)]).all()    # 0 * (inf - x) is NaN, and NaN stays NaN


@pytest.mark.parametrize("w,h,seed,share", [(97, 61, 9, 0.857), (130, 97, 5, 0.899)])
def test_the_exact_adjacent_flows_chain_to_the_exact_long_range_flow(w, h, seed, share):
    """The clip's motion is a rotation and a translation, so every adjacent flow f_k is an affine function of the position and
    its bilinear sample is exact in real arithmetic: what is left is float32 rounding.  With u = 2^-24 (|fl(r) - r| <= u |r|),
    per component, F the largest |adjacent flow|, Amax the largest |A_k|, g = 2 sin(theta / 2) the Lipschitz constant of f_k
    (the norm of R - I) and e_k the error of A_k:
      the taps are roundings of f_k: u F, and a convex combination of them is no worse;
      t (or b) and s are each rounded once: u F each; the differences P01 - P00 and b - t are at most g + 2 u F and their
      roundings and the products' at most 4 u (g + 2 u F) together: less than u, taken as u;
      the position fl(x + Au) is off by u (W - 1) in x and u (H - 1) in y on top of e_k in each: the sample moves by at most
      g (2 e_k + u (W + H));  ax = px - floor(px) is exact;
      A_{k+1} = fl(A_k + s): u Amax.
    e_{k+1} <= (1 + 2 g) e_k + u (3 F + 1 + g (W + H) + Amax), over six links, plus u Amax for the rounding of the float32 long-
    range flow it is compared with."""
    clip = SynthClip(w, h, seed)
    flows = np.stack([_planes(clip.true_flow(k, k + 1)) for k in range(6)])
    out, valid = R.chain(flows, 6)
    truth = _planes(clip.true_flow(0, 6))
    ok = valid[-1] != 0
    assert abs(ok.mean() - share) < 0.002, ok.mean()
    u, g = 2.0 ** -24, 2 * math.sin(math.radians(ROTATION_DEG) / 2)
    big_f, a_max = float(np.abs(flows).max()), float(np.abs(out[:, :, ok]).max())
    step, e = u * (3 * big_f + 1 + g * (w + h) + a_max), 0.0
    for _ in range(6):
        e = (1 + 2 * g) * e + step
    bound = e + u * a_max
    err = float(np.abs(out[-1].astype(np.float64) - truth)[:, ok].max())
    print(f"SynthClip({w}, {h}, {seed}) exact flows chained 0 -> 6: valid share {ok.mean():.3f}, max |err| {err:.3g}, bound {bound:.3g}")
    assert bound < 1e-5  # the bound is float rounding, not a tolerance
    assert err <= bound, (err, bound)


def test_hop_minus_one_over_the_reversed_list_is_hop_one():
    rng = np.random.default_rng(2)
    flows, occ = smooth_flow(rng, 7, 23, 31, 3.0), R.sparse_mask(rng, 7, 23, 31)
    up = R.chain_batch(flows, 3, first=1, hop=1, anchors=2, anchor_step=2, emit="all", occ=occ)
    # anchor j of the reversed list starts at 6 - (1 + 2 j): anchors in descending order need a walk of their own
    for j in range(2):
        down = R.chain(flows[::-1], 3, 6 - (1 + 2 * j), -1, "zero", occ[::-1])
        assert R.same_bits(down[0], up[0][3 * j:3 * j + 3]) and np.array_equal(down[1], up[1][3 * j:3 * j + 3])


def test_emit_all_holds_every_link_and_the_last_one_last():
    rng = np.random.default_rng(3)
    flows = smooth_flow(rng, 8, 23, 31, 3.0)
    for border in R.BORDERS:
        last, vlast = R.chain_batch(flows, 6, anchors=3, emit="last", border=border)
        every, vevery = R.chain_batch(flows, 6, anchors=3, emit="all", border=border)
        assert last.shape == (3, 2, 23, 31) and every.shape == (18, 2, 23, 31) and vevery.shape == (18, 23, 31)
        assert R.same_bits(every[5::6], last) and np.array_equal(vevery[5::6], vlast)
        for k in range(1, 7):  # the first k links of a longer chain are the chain of length k
            shorter, vshorter = R.chain_batch(flows, k, anchors=3, emit="last", border=border)
            assert R.same_bits(every[k - 1::6], shorter) and np.array_equal(vevery[k - 1::6], vshorter)
        assert (np.diff(vevery.reshape(3, 6, 23, 31).astype(int), axis=1) <= 0).all()  # valid never comes back
    assert R.fit_anchors(8, 6) == 3 and R.chain_batch(flows, 6)[0].shape[0] == 3
    assert R.fit_anchors(8, 6, anchor_step=2) == 2 and R.fit_anchors(8, 9) == 0 and R.fit_anchors(8, 3, 7, -2, 1) == 1


def test_occlusion_at_link_zero_is_the_pixels_own_byte():
    rng = np.random.default_rng(4)
    flows, occ = smooth_flow(rng, 2, 23, 31, 3.0), R.sparse_mask(rng, 2, 23, 31, 0.3)
    for border in R.BORDERS:
        out, valid = R.chain(flows, 1, 1, 1, border, occ)
        assert np.array_equal(valid[0], (occ[1] == 0).astype(np.uint8))
        assert R.same_bits(out, R.chain(flows, 1, 1, 1, border)[0])  # the mask never changes a stored value


@pytest.mark.parametrize("w,h", [(97, 61), (130, 97)])
def test_both_values_of_valid_are_exercised_by_the_gpu_tests_inputs(w, h):
    """On the reference alone: the inputs of tests/test_flow_chain_gpu.py leave between 0.2 and 0.95 of the pixels valid after
    six links, with and without its 2 % masks."""
    flows, occ = R.chain_inputs(w, h)
    for o in (None, occ):
        share = R.chain(flows, 6, 0, 1, "zero", o)[1][-1].mean()
        assert 0.2 <= share <= 0.95, (w, h, o is not None, share)


def _epe(flow, truth, where):
    d = flow.astype(np.float64) - truth
    return float(np.sqrt(d[0] ** 2 + d[1] ** 2)[where].mean())


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_quality_record_on_the_oracles_flows(oracle, algo):
    """Recorded, not asserted: the end-point error against SynthClip's true flow of the oracle's six adjacent flows chained, and
    of its direct 0 -> 6 estimate (profiles/flow_chain/quality.txt holds this test's printed lines)."""
    clip = SynthClip(97, 61, 9)
    calc = getattr(oracle, algo)
    flows = np.stack([_planes(calc(clip.frame(k), clip.frame(k + 1))) for k in range(6)])
    direct = _planes(calc(clip.frame(0), clip.frame(6)))
    truth = _planes(clip.true_flow(0, 6)).astype(np.float64)
    out, valid = R.chain(flows, 6)
    ok, everywhere = valid[-1] != 0, np.ones((61, 97), bool)
    clamped = R.chain(flows, 6, border="clamp")[0][-1]
    print(f"{algo} SynthClip(97, 61, 9) 0 -> 6: share of pixels whose chain stays in frame {ok.mean():.3f}; EPE over those pixels: "
          f"chain {_epe(out[-1], truth, ok):.3f} px, direct estimate {_epe(direct, truth, ok):.3f} px; over all pixels: chain with the "
          f"clamp border {_epe(clamped, truth, everywhere):.3f} px, direct estimate {_epe(direct, truth, everywhere):.3f} px")
    assert np.isfinite(out).all()
