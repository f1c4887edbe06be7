"""The NumPy reference of the backward warp (tests/warp_ref.py) against itself and against what the warp is for: its scalar
loop equals its vectorised form, its edge cases are the ones include/dfx.h states, and on the CPU oracle's flows the warp
error discriminates — so the device tests, which compare with this reference, cannot pass on a warp that samples nothing.
No GPU and no engine is touched here."""
import numpy as np
import pytest

from denseflow_amd.synth import HardClip, SynthClip
from tests import warp_ref as R

F32 = np.float32


def _planes(flow):  # (H, W, 2) of the oracle -> (2, H, W)
    return np.ascontiguousarray(flow.transpose(2, 0, 1))


def _image(rng, h, w, c):
    return rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)


@pytest.mark.parametrize("border", R.BORDERS)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (17, 9), (40, 23)])
def test_the_loop_equals_the_vectorised_form(w, h, c, border):
    rng = np.random.default_rng(w * 100 + h)
    flows = R.warp_flow(rng, 2, h, w)
    R.plant_specials(flows[1])
    for i in range(2):
        src, ref = _image(rng, h, w, c), _image(rng, h, w, c)
        occ = (rng.random((h, w)) < 0.3).astype(np.uint8)
        for mask in (None, occ):
            with np.errstate(all="raise"):
                s, valid = R.warp(src, flows[i], border, mask)
                s_l, valid_l = R.warp_loop(src, flows[i], border, mask)
            assert s.dtype == F32 and s.shape == src.shape and valid.dtype == np.uint8 and valid.shape == (h, w)
            assert np.array_equal(s.view(np.uint32), s_l.view(np.uint32))
            assert np.array_equal(valid, valid_l) and set(np.unique(valid)) <= {0, 1}
            assert s.min() >= 0 and s.max() <= 255
            cnt, sad = R.stats(s, ref, valid)
            q, q_ref = R.quantise(s_l).reshape(h, w, c).astype(int), ref.reshape(h, w, c).astype(int)
            assert cnt == sum(int(valid_l[y, x]) for y in range(h) for x in range(w))
            assert sad == sum(abs(q[y, x, k] - q_ref[y, x, k]) for y in range(h) for x in range(w) for k in range(c) if valid_l[y, x])
        for dtype in R.DTYPES:
            out = R.stored(s, dtype)
            assert out.shape == s.shape and out.dtype == {"uint8": np.uint8, "float32": F32}.get(dtype, np.uint16)


@pytest.mark.parametrize("c", [1, 3])
def test_a_zero_flow_is_the_identity(c):
    w, h = 19, 7
    src = _image(np.random.default_rng(3), h, w, c)
    for border in R.BORDERS:
        for f in (R.warp, R.warp_loop):
            s, valid = f(src, np.zeros((2, h, w), F32), border)
            assert np.array_equal(R.stored(s, "uint8"), src) and valid.all()
            assert np.array_equal(s, src.astype(F32))
            assert R.stats(s, src, valid) == (w * h, 0)
    for dtype in ("float16", "bfloat16"):  # bytes are exact in either half type
        assert np.array_equal(R.stored(s, dtype), R.stored(src.astype(F32), dtype))


@pytest.mark.parametrize("dx,dy", [(3, 0), (-2, 1), (0, -4), (5, 2)])
@pytest.mark.parametrize("c", [1, 3])
def test_an_integer_translation_is_an_exact_shift(c, dx, dy):
    w, h = 21, 13
    src = _image(np.random.default_rng(11), h, w, c)
    flow = np.zeros((2, h, w), F32)
    flow[0], flow[1] = dx, dy
    ys, xs = np.mgrid[0:h, 0:w]
    tx, ty = xs + dx, ys + dy
    stays = (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
    shifted = src[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)]  # the edge pixel where the target leaves the frame
    s, valid = R.warp(src, flow, "zero")
    q = R.stored(s, "uint8")
    assert np.array_equal(valid, stays.astype(np.uint8)) and 0 < stays.sum() < w * h
    assert np.array_equal(q[stays], shifted[stays]) and not q[~stays].any()
    s, valid = R.warp(src, flow, "clamp")
    assert np.array_equal(valid, stays.astype(np.uint8))  # valid is the unclamped test
    assert np.array_equal(R.stored(s, "uint8"), shifted)


def test_ties_round_to_even():
    rows = [np.arange(256), np.array([254, 255]), np.array([255, 254])]
    for row in rows:
        w = len(row)
        src = np.stack([row, row]).astype(np.uint8)
        flow = np.zeros((2, 2, w), F32)
        flow[0] = 0.5
        for f in (R.warp, R.warp_loop):
            s, valid = f(src, flow, "clamp")
            q = R.quantise(s)
            assert np.all(s[0, :-1] == (row[:-1] + row[1:]) / 2)  # exactly k + 0.5
            even = ((row[:-1] + row[1:]) / 2 + 0.5) // 2 * 2        # the even neighbour of k + 0.5
            assert np.array_equal(q[0, :-1], even.astype(np.uint8))
    assert tuple(R.quantise(np.array([0.5, 1.5, 2.5, 253.5, 254.5], F32))) == (0, 2, 2, 254, 254)


def test_nan_inf_and_huge_flows_never_reach_a_conversion():
    w, h = 9, 7
    src = _image(np.random.default_rng(2), h, w, 3)
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for plane in (0, 1):
            flow = np.zeros((2, h, w), F32)
            flow[plane, 3, 4] = bad
            for f in (R.warp, R.warp_loop):
                with np.errstate(all="raise"):
                    s, valid = f(src, flow, "zero")
                    sc, valid_c = f(src, flow, "clamp")
                assert valid[3, 4] == 0 and valid.sum() == w * h - 1 and np.array_equal(valid, valid_c)
                assert not s[3, 4].any(), (bad, plane)
                if np.isnan(bad):
                    assert not sc[3, 4].any()
                else:  # clamped onto the edge it left by
                    edge = (0 if bad < 0 else w - 1, 3) if plane == 0 else (4, 0 if bad < 0 else h - 1)
                    assert np.array_equal(sc[3, 4], src[edge[1], edge[0]].astype(F32)), (bad, plane)
                others = np.ones((h, w), bool)
                others[3, 4] = False
                assert np.array_equal(s[others], src[others].astype(F32)) and np.array_equal(sc[others], src[others].astype(F32))


def test_the_last_column_and_row_are_inside_and_the_taps_clamp():
    w, h = 8, 5
    src = _image(np.random.default_rng(5), h, w, 1)
    flow = np.zeros((2, h, w), F32)
    flow[0, 1, 2] = w - 1 - 2                       # px exactly W - 1
    flow[1, 2, 3] = h - 1 - 2                       # py exactly H - 1
    flow[0, 0, 0], flow[1, 0, 0] = w - 1, h - 1     # both
    for border in R.BORDERS:
        s, valid = R.warp(src, flow, border)
        for (x, y), (tx, ty) in {(2, 1): (w - 1, 1), (3, 2): (3, h - 1), (0, 0): (w - 1, h - 1)}.items():
            assert valid[y, x] == 1 and s[y, x] == src[ty, tx], (x, y)  # ax = ay = 0 and x1 / y1 clamp onto x0 / y0
    flow[0, 1, 2] = np.nextafter(F32(w - 1 - 2), F32(np.inf))  # one ulp further: px > W - 1
    s, valid = R.warp(src, flow, "zero")
    assert valid[1, 2] == 0 and s[1, 2] == 0
    s, valid = R.warp(src, flow, "clamp")
    assert valid[1, 2] == 0 and s[1, 2] == src[1, w - 1]
    where = R.plant_specials(np.zeros((2, 23, 40), F32))
    assert len(set(where.values())) == len(R.SPECIALS)


def test_an_occlusion_mask_removes_exactly_its_pixels():
    w, h = 33, 14
    rng = np.random.default_rng(8)
    src, ref = _image(rng, h, w, 3), _image(rng, h, w, 3)
    flow = R.warp_flow(rng, 1, h, w)[0]
    occ = (rng.random((h, w)) < 0.4).astype(np.uint8) * 7  # any non-zero value occludes
    s, valid = R.warp(src, flow)
    s_m, valid_m = R.warp(src, flow, occ=occ)
    inside = R.inside_of(flow)
    assert np.array_equal(s, s_m)  # the mask never changes a stored value
    assert np.array_equal(valid, inside.astype(np.uint8)) and np.array_equal(valid_m, (inside & (occ == 0)).astype(np.uint8))
    cnt, sad = R.stats(s, ref, valid)
    cnt_m, sad_m = R.stats(s_m, ref, valid_m)
    assert cnt - cnt_m == int((inside & (occ != 0)).sum()) > 0
    gone = inside & (occ != 0)
    assert sad - sad_m == int(np.abs(R.quantise(s).astype(int) - ref.astype(int)).sum(axis=2)[gone].sum())


def _error(src, ref, flow, valid_of=None):
    """(mean absolute error over the valid set of valid_of (default: of flow itself), valid share)."""
    s, valid = R.warp(src, flow)
    if valid_of is not None:
        valid = R.warp(src, valid_of)[1]
    cnt, sad = R.stats(s, ref, valid)
    return sad / (cnt * 1.0), cnt / valid.size


def test_the_warp_error_discriminates_on_the_oracles_flows(oracle):
    clip, hard = SynthClip(97, 61, 9), HardClip(130, 97, 5)
    cases = [("SynthClip(97, 61, 9) 0 -> 1", clip.frame(0), clip.frame(1), ("tvl1_calc", "farneback_calc")),
             ("SynthClip(97, 61, 9) 0 -> 6", clip.frame(0), clip.frame(6), ("tvl1_calc",)),
             ("HardClip(130, 97, 5) 0 -> 2", hard.frame(0), hard.frame(2), ())]
    for name, a, b, asserted in cases:
        for algo in ("tvl1_calc", "farneback_calc"):
            flow = _planes(getattr(oracle, algo)(a, b))
            err, share = _error(b, a, flow)
            zero, _ = _error(b, a, np.zeros_like(flow), valid_of=flow)  # the zero flow over the same valid set
            print(f"{name} {algo}: zero flow {zero:.3f}, with the flow {err:.3f}, ratio {err / zero:.3f}, valid share {share:.3f}")
            if algo in asserted:
                assert err <= 0.25 * zero, (name, algo, err, zero)
                assert share > 0.5, (name, algo, share)
