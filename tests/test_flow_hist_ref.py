"""The NumPy reference of the motion descriptors of flows (tests/flow_hist_ref.py, the text of include/dfx.h section (0.5.2))
held against what the definition promises (no GPU): the direction table of the header, the conservation of the weights, the
derivative of an affine field, the invariance of MBH under an integer camera pan, the masked-neighbour rule, every
normalisation including empty cells, and — printed and recorded in profiles/flow_hist/quality.txt, not asserted — how far the
float32 / integer definition lies from the same rule in float64 with the true arctan2."""
import numpy as np
import pytest

from tests import flow_hist_ref as R
from tests.fb_check_ref import smooth_flow

F32 = np.float32


def _const(u, v, h=4, w=4):
    f = np.empty((1, 2, h, w), F32)
    f[0, 0], f[0, 1] = u, v
    return f


def _hof(u, v, thr=-1.0, bins=8):
    return R.flow_hist_sums(_const(u, v), "hof", 4, bins, thr)[0, 0, 0]


def test_the_direction_table_of_the_header():
    assert _hof(1.0, 0.0).tolist() == [4096, 0, 0, 0, 0, 0, 0, 0, 0]
    down = _hof(0.0, 1.0)
    assert down[2] == 4096 and down.sum() == 4096  # y down: counter-clockwise in image coordinates
    for v in (0.0, -0.0):  # no seam at the branch cut of atan2
        left = _hof(-1.0, v)
        assert left[4] == 4096 and left.sum() == 4096, (v, left)
    diag = _hof(1.0, 1.0)
    assert diag[1] == 5792 and diag.sum() == 5792  # 16 * rint(sqrt(2) * 256) = 16 * 362
    assert _hof(0.1, 0.1, 0.4).tolist() == [0] * 8 + [4096]
    assert _hof(0.1, 0.1, -1.0)[8] == 0  # a negative threshold disables the rule, the slot keeps its place
    assert _hof(0.0, 0.0, 0.0)[8] == 4096 and _hof(0.0, 0.0, -1.0).sum() == 0
    up = _hof(0.0, -1.0)
    assert up[6] == 4096
    # odd bins: 180 degrees lies between bins 4 and 5 of 9
    left9 = _hof(-1.0, 0.0, bins=9)
    assert left9[4] == 2048 and left9[5] == 2048
    assert R.slots(("hof", "mbhx", "mbhy"), 8) == 25


@pytest.mark.parametrize("cell", R.CELLS)
@pytest.mark.parametrize("bins", [2, 8, 9, 16])
def test_the_total_of_a_cell_is_the_sum_of_q_of_the_pixels_that_take_part(cell, bins):
    rng = np.random.default_rng(cell * 100 + bins)
    n, h, w = 2, 37, 45
    flows = smooth_flow(rng, n, h, w, 5.0)
    mask = (rng.random((n, h, w)) < 0.15).astype(np.uint8)
    sums = R.flow_hist_sums(flows, ("hof", "mbhx", "mbhy"), cell, bins, -1.0, mask)
    vec = R.vectors(flows, mask)
    ch, cw = sums.shape[1:3]
    for name, base, length in R.channels(7, bins):
        gx, gy, part = vec[name]
        Q = R.bin_weights(gx, gy, bins)[1] * part
        padded = np.zeros((n, ch * cell, cw * cell), np.int64)
        padded[:, :h, :w] = Q
        want = padded.reshape(n, ch, cell, cw, cell).sum((2, 4))
        assert np.array_equal(sums[..., base:base + length].sum(-1), want), name
    assert (sums >= 0).all()
    # with the still rule, the HOF total is the sum of Q of the moving pixels plus 256 per still pixel
    sums_s = R.flow_hist_sums(flows, "hof", cell, bins, 2.0, mask)
    u, v, part = vec["hof"]
    m, Q = R.bin_weights(u, v, bins)[:2]
    still = part & (m <= F32(2.0))
    assert still.any() and (part & ~still).any()
    assert sums_s[..., bins].sum() == 256 * still.sum()
    assert sums_s[..., :bins].sum() == (Q * (part & ~still)).sum()


def test_an_affine_field_has_a_constant_derivative_halved_on_the_borders():
    h, w, a, b = 9, 11, 0.75, -0.5
    y, x = np.mgrid[:h, :w].astype(F32)
    flows = np.zeros((1, 2, h, w), F32)
    flows[0, 0] = F32(a) * x + F32(b) * y  # exact: small multiples of 1/4
    gx, gy, part = R.vectors(flows)["mbhx"]
    assert part.all()
    assert np.all(gx[0, :, 1:-1] == F32(2 * a)) and np.all(gx[0, :, 0] == F32(a)) and np.all(gx[0, :, -1] == F32(a))
    assert np.all(gy[0, 1:-1] == F32(2 * b)) and np.all(gy[0, 0] == F32(b)) and np.all(gy[0, -1] == F32(b))
    vx, vy, _ = R.vectors(flows)["mbhy"]
    assert not vx.any() and not vy.any()


def test_mbh_does_not_see_an_integer_camera_pan_and_hof_does():
    rng = np.random.default_rng(5)
    n, h, w = 2, 33, 41
    flows = (rng.integers(-64 * 64 + 1, 64 * 64, (n, 2, h, w)) / 64.0).astype(F32)  # multiples of 1/64 below 64
    panned = flows.copy()
    panned[:, 0] += F32(7.0)  # exact float adds
    panned[:, 1] += F32(-3.0)
    assert np.array_equal((panned[:, 0] - F32(7.0)), flows[:, 0])
    for cell in (4, 16):
        a = R.flow_hist_sums(flows, ("hof", "mbhx", "mbhy"), cell, 8, 0.4)
        b = R.flow_hist_sums(panned, ("hof", "mbhx", "mbhy"), cell, 8, 0.4)
        assert np.array_equal(a[..., 9:], b[..., 9:])
        assert not np.array_equal(a[..., :9], b[..., :9])
        for norm in R.NORMS:
            va, vb = R.normalise(a, 7, 8, norm), R.normalise(b, 7, 8, norm)
            assert np.array_equal(va[..., 9:].view(np.uint32), vb[..., 9:].view(np.uint32))


def test_a_pixel_with_a_masked_or_unknown_neighbour_leaves_mbh_and_stays_in_hof():
    h, w = 8, 8
    y, x = np.mgrid[:h, :w].astype(F32)
    flows = np.zeros((1, 2, h, w), F32)
    flows[0, 0], flows[0, 1] = x * x + y, y * y + F32(1)
    mask = np.zeros((1, h, w), np.uint8)
    mask[0, 3, 4] = 200
    flows[0, 0, 6, 1] = np.nan
    flows[0, 1, 0, 7] = np.inf  # a corner: its clamped neighbours are itself, (6, 0) and (7, 1)
    vec = R.vectors(flows, mask)
    part = vec["mbhx"][2][0]
    want = np.ones((h, w), bool)
    for yy, xx in ((3, 4), (6, 1), (0, 7)):
        for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)):
            if 0 <= yy + dy < h and 0 <= xx + dx < w:
                want[yy + dy, xx + dx] = False
    assert np.array_equal(part, want) and np.array_equal(vec["mbhy"][2][0], want)
    hof_part = vec["hof"][2][0]
    assert hof_part.sum() == h * w - 3 and not hof_part[3, 4] and not hof_part[6, 1] and not hof_part[0, 7]
    sums = R.flow_hist_sums(flows, 7, 8, 8, -1.0, mask)
    assert np.isfinite(R.normalise(sums, 7, 8, "l2")).all()
    # the same pixels masked or NaN: the same histograms
    flows2, mask2 = flows.copy(), mask.copy()
    flows2[0, :, 3, 4] = np.nan
    mask2[0, 6, 1] = 1
    assert np.array_equal(sums, R.flow_hist_sums(flows2, 7, 8, 8, -1.0, mask2))


def test_every_normalisation_and_the_empty_cell():
    rng = np.random.default_rng(11)
    n, h, w, cell, bins = 1, 16, 24, 8, 8
    flows = smooth_flow(rng, n, h, w, 3.0)
    mask = np.zeros((n, h, w), np.uint8)
    mask[0, :8, 8:16] = 1  # cell (0, 1) is empty
    vals, sums = {}, None
    for norm in R.NORMS:
        vals[norm], sums = R.flow_hist(flows, 7, cell, bins, 0.4, norm, mask)
        assert vals[norm].shape == (n, 25, 2, 3) and vals[norm].dtype == F32 and sums.shape == (n, 2, 3, 25)
    assert not sums[0, 0, 1].any()
    for norm in R.NORMS:
        assert not vals[norm][0, :, 0, 1].any() and np.isfinite(vals[norm]).all()
    S = sums.transpose(0, 3, 1, 2).astype(np.float64)
    assert np.array_equal(vals["none"], (S / 256).astype(F32))
    for name, base, length in R.channels(7, bins):
        s = S[:, base:base + length]
        full = s.sum(1) > 0
        assert np.allclose(vals["l1"][:, base:base + length].sum(1)[full], 1.0, atol=1e-6)
        assert np.allclose((vals["l1_sqrt"][:, base:base + length].astype(np.float64) ** 2).sum(1)[full], 1.0, atol=1e-6)
        assert np.allclose((vals["l2"][:, base:base + length].astype(np.float64) ** 2).sum(1)[full], 1.0, atol=1e-6)
        assert np.array_equal(vals["l1_sqrt"][:, base:base + length],
                              np.sqrt(vals_f64(s, "l1")).astype(F32))
    # all-zero input: every value 0 under every norm, nothing divided by zero
    zero = np.zeros((1, 2, 5, 7), F32)
    for norm in R.NORMS:
        v, s = R.flow_hist(zero, 7, 4, 8, -1.0, norm)
        assert not v.any() and not s.any()


def vals_f64(s, norm):
    t = s.sum(1, keepdims=True)
    return np.where(t > 0, s / np.where(t > 0, t, 1.0), 0.0)


def test_how_far_the_definition_lies_from_float64_and_the_true_arctan2():
    """Printed and recorded (profiles/flow_hist/quality.txt), not asserted beyond sanity: the largest difference of a slot,
    as a share of its cell-and-channel's total weight, between the float32 / integer definition and the same rule in float64
    with numpy's arctan2, over smooth 97 x 61 flows, every cell size and bins 2 .. 16."""
    rng = np.random.default_rng(97 * 61)
    flows = smooth_flow(rng, 9, 61, 97, 6.0)
    worst = 0.0
    for cell in R.CELLS:
        for bins in (2, 3, 8, 9, 16):
            sums = R.flow_hist_sums(flows, 7, cell, bins, 0.4).astype(np.float64) / 256.0
            ref = R.flow_hist_f64(flows, 7, cell, bins, 0.4)
            rel = 0.0
            for _, base, length in R.channels(7, bins):
                total = np.maximum(ref[..., base:base + length].sum(-1, keepdims=True), 1.0)
                rel = max(rel, float((np.abs(sums - ref)[..., base:base + length] / total).max()))
            print(f"cell {cell:2d} bins {bins:2d}: largest slot difference {rel:.3e} of the cell's channel total")
            worst = max(worst, rel)
    print(f"worst {worst:.3e}")
    assert np.isfinite(worst)
