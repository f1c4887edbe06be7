"""The NumPy restatement of the flow median (tests/flow_median_ref.py) against the CPU oracle's cv::medianBlur
(cpu_tvl1_median_blur), against the identities the mask forms must keep, and on special values with the expected bit
patterns written out by hand — so the device tests, which compare with this restatement, stand on checked ground.  The
quality record (does the median or the fill help on the oracle's flows?) is printed, not asserted.  No GPU is touched."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import fb_check_ref
from tests import flow_median_ref as R

F32 = np.float32
U32 = np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


@pytest.mark.parametrize("quantised", [False, True])
@pytest.mark.parametrize("h,w", [(7, 9), (16, 16), (5, 31), (1, 1), (2, 3), (3, 2)])
@pytest.mark.parametrize("ksize", [3, 5])
def test_unmasked_equals_the_oracles_median_blur(oracle, ksize, h, w, quantised):
    rng = np.random.default_rng(1000 * h + 10 * w + ksize)
    flow = rng.standard_normal((2, h, w)).astype(F32)
    if quantised:  # many ties
        flow = (np.rint(flow * 4) / 4).astype(F32)
        flow[flow == 0] = 0.0  # no -0: the oracle compares floats, the definition keys
    assert not np.isnan(flow).any() and not np.signbit(flow[flow == 0]).any()
    got, none = R.flow_median_ref(flow, ksize)
    assert none is None
    for c in range(2):
        want = np.empty((h, w), F32)
        oracle.lib().cpu_tvl1_median_blur(np.ascontiguousarray(flow[c]), want, w, h, ksize)
        assert np.array_equal(_bits(got[c]), _bits(want)), (ksize, h, w, c)


@pytest.mark.parametrize("ksize", [3, 5])
def test_mask_identities(ksize):
    rng = np.random.default_rng(ksize)
    h, w = 13, 17
    flow = rng.standard_normal((2, h, w)).astype(F32)
    plain, _ = R.flow_median_ref(flow, ksize)
    out, mo = R.flow_median_ref(flow, ksize, np.zeros((h, w), np.uint8), "all")
    assert np.array_equal(_bits(out), _bits(plain)) and mo.dtype == np.uint8 and not mo.any()
    out, mo = R.flow_median_ref(flow, ksize, np.zeros((h, w), np.uint8), "fill")
    assert np.array_equal(_bits(out), _bits(flow)) and not mo.any()
    mask = (rng.random((h, w)) < 0.3).astype(np.uint8)
    out, mo = R.flow_median_ref(flow, ksize, mask, "fill")
    assert np.array_equal(_bits(out)[:, mask == 0], _bits(flow)[:, mask == 0])
    assert not mo[mask == 0].any()
    all_out, all_mo = R.flow_median_ref(flow, ksize, mask, "all")
    assert np.array_equal(_bits(out)[:, mask != 0], _bits(all_out)[:, mask != 0]) and np.array_equal(mo, all_mo)
    assert (_bits(all_out)[:, mask == 0] != _bits(flow)[:, mask == 0]).any()
    for mode in ("all", "fill"):
        out, mo = R.flow_median_ref(flow, ksize, np.full((h, w), 255, np.uint8), mode)
        assert np.array_equal(_bits(out), _bits(flow)) and mo.all() and set(np.unique(mo)) == {1}


def test_a_hole_fills_inward_by_r_per_pass():
    rng = np.random.default_rng(21)
    flow = rng.standard_normal((1, 2, 21, 21)).astype(F32)
    mask = np.zeros((1, 21, 21), np.uint8)
    mask[0, 7:14, 7:14] = 1
    out1, m1 = R.flow_median_batch(flow, 5, mask, "fill", 1)
    assert m1.any() and m1.sum() == 9 and m1[0, 9:12, 9:12].all()  # the ring of width r = 2 is filled, the 3 x 3 core is not
    out2, m2 = R.flow_median_batch(flow, 5, mask, "fill", 2)
    assert not m2.any()
    assert np.array_equal(_bits(out2)[:, :, mask[0] == 0], _bits(flow)[:, :, mask[0] == 0])
    assert np.array_equal(_bits(out1)[0][:, m1[0] == 1], _bits(flow)[0][:, m1[0] == 1])  # m == 0: out = in
    out9, m9 = R.flow_median_batch(flow, 5, mask, "fill", 9)  # stops early: the same as two
    assert np.array_equal(_bits(out9), _bits(out2)) and not m9.any()


NNAN, NINF, MONE, NZERO, PZERO, SUB, ONE, PINF, PNAN = (0xFFC00002, 0xFF800000, 0xBF800000, 0x80000000, 0x00000000,
                                                        0x00000001, 0x3F800000, 0x7F800000, 0x7FC00001)
ASCENDING = [NNAN, NINF, MONE, NZERO, PZERO, SUB, ONE, PINF, PNAN]  # by key; by hand


def test_the_key_orders_special_values_as_stated():
    keys = R.key_of(np.array(ASCENDING, U32))
    assert np.all(keys[1:] > keys[:-1])
    assert np.array_equal(R.bits_of(keys), np.array(ASCENDING, U32))
    assert R.key_of(U32(0x7FFFFFFF)) == 0xFFFFFFFF and R.key_of(U32(0xFFFFFFFF)) == 0
    assert R.key_of(U32(0x80000001)) < R.key_of(U32(0x80000000)) < R.key_of(U32(0)) < R.key_of(U32(1))  # -sub < -0 < +0 < sub


def test_special_values_select_by_key():
    perm = [6, 0, 8, 3, 1, 4, 7, 2, 5]  # the nine values scattered over a 3 x 3 field
    u = np.array([ASCENDING[i] for i in perm], U32).reshape(3, 3)
    flow = np.stack([u, u.T]).view(F32)

    def centre(mask=None, mode="all"):
        out, mo = R.flow_median_ref(flow, 3, mask, mode)
        return int(_bits(out)[0, 1, 1]), int(_bits(out)[1, 1, 1]), (None if mo is None else int(mo[1, 1]))

    # all nine: rank 4 of the ascending list is +0, not -0 (a float comparison could not tell them apart)
    assert centre() == (PZERO, PZERO, None)
    # without +0 and 1.0: m = 7, rank 3 -> -0 with its sign
    mask = np.isin(u, [PZERO, ONE]).astype(np.uint8)
    assert centre(mask)[0] == NZERO
    # only the two NaNs: m = 2, rank 0 -> the negative NaN, payload and all
    mask = (~np.isin(u, [NNAN, PNAN])).astype(np.uint8)
    assert centre(mask)[0] == NNAN and centre(mask)[2] == 0
    # only the positive NaN: itself, not quieted further or replaced
    mask = (u != PNAN).astype(np.uint8)
    assert centre(mask)[0] == PNAN
    # subnormal, +0, -0 only: m = 3, rank 1 -> +0; without -0: m = 2, rank 0 -> +0; without +0: -0 then subnormal -> -0
    assert centre((~np.isin(u, [SUB, PZERO, NZERO])).astype(np.uint8))[0] == PZERO
    assert centre((~np.isin(u, [SUB, PZERO])).astype(np.uint8))[0] == PZERO
    assert centre((~np.isin(u, [SUB, NZERO])).astype(np.uint8))[0] == NZERO
    assert centre((~np.isin(u, [SUB, PINF])).astype(np.uint8))[0] == SUB  # the subnormal is not flushed
    # the corner (0, 0) sees (0,0) four times, (0,1) and (1,0) twice, (1,1) once: ONE x4, NNAN x2, NZERO x2, NINF x1
    # ascending: NNAN NNAN NINF NZERO NZERO ONE ONE ONE ONE -> rank 4 = -0
    assert [int(u[0, 0]), int(u[0, 1]), int(u[1, 0]), int(u[1, 1])] == [ONE, NNAN, NZERO, NINF]
    assert int(_bits(R.flow_median_ref(flow, 3)[0])[0, 0, 0]) == NZERO
    # a real sample with key 0xFFFFFFFF (bits 0x7FFFFFFF) next to excluded samples: it is still selected as itself
    f2 = np.full((2, 3, 3), 0x7FFFFFFF, U32).view(F32)
    m2 = np.ones((3, 3), np.uint8)
    m2[0, 0] = 0
    out, mo = R.flow_median_ref(f2, 3, m2, "all")
    assert np.all(_bits(out) == 0x7FFFFFFF)
    assert np.array_equal(mo, [[0, 0, 1], [0, 0, 1], [1, 1, 1]])  # m > 0 exactly where (0, 0) is in the window


def test_the_special_field_has_every_class_of_value():
    f = R.special_field()
    b = _bits(f)
    assert f.shape == (2, 6, 7) and np.isnan(f).sum() >= 16 and np.isinf(f).sum() >= 8
    assert (b == 0x80000000).any() and (b == 0).any() and ((b & 0x7F800000) == 0).sum() > 8 and (b == 0x7FFFFFFF).any()
    for ksize in (3, 5):
        out, _ = R.flow_median_ref(f, ksize)
        assert np.isin(_bits(out), b).all()  # always the bit pattern of an input sample


def _planes(flow):  # (H, W, 2) of the oracle -> (2, H, W)
    return np.ascontiguousarray(flow.transpose(2, 0, 1))


def _epe(flow, truth, where):
    d = flow.astype(np.float64) - truth
    e = np.sqrt(d[0] ** 2 + d[1] ** 2)
    return float(e[where].mean()) if where.any() else float("nan")


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_quality_record_on_the_oracles_flows(oracle, algo):
    """Recorded, not asserted: end-point error against SynthClip's true flow before and after (profiles/flow_median/quality.txt
    holds this test's printed lines)."""
    clip = SynthClip(97, 61, 9)
    a, b = clip.frame(0), clip.frame(6)
    calc = getattr(oracle, algo)
    fwd, bwd = _planes(calc(a, b)), _planes(calc(b, a))
    truth = _planes(clip.true_flow(0, 6)).astype(np.float64)
    occ, _ = fb_check_ref.fb_check(fwd, bwd)
    masked, clear = occ != 0, occ == 0
    flows, masks, passes = fwd[None], occ[None], 0
    while masks.any() and passes < 16:
        flows, masks = R.flow_median_batch(flows, 5, masks, "fill", 1)
        passes += 1
    print(f"{algo} SynthClip(97, 61, 9) 0 -> 6: masked share {masked.mean():.3f}; EPE over masked pixels {_epe(fwd, truth, masked):.3f}"
          f" -> {_epe(flows[0], truth, masked):.3f} px after fill (ksize 5, {passes} passes, {int(masks.sum())} pixels left)")
    line = f"{algo} SynthClip(97, 61, 9) 0 -> 6: EPE over unmasked pixels {_epe(fwd, truth, clear):.4f}"
    for ksize in (3, 5):
        out, _ = R.flow_median_ref(fwd, ksize)
        line += f" -> {_epe(out, truth, clear):.4f} (all, ksize {ksize}, no mask)"
        out, _ = R.flow_median_ref(fwd, ksize, occ, "all")
        line += f" / {_epe(out, truth, clear):.4f} (with the mask)"
    print(line + " px")
    assert np.array_equal(_bits(flows)[0][:, clear], _bits(fwd)[:, clear])  # fill never touches reliable flow
