"""The NumPy restatement of the colour coding of flows (tests/flow_colour_ref.py; include/dfx.h section (0.5.1)) against what
it restates: the wheel's check values, the polynomial angle against arctan2 in float64 (bound 1e-6 half-turns: the
polynomial's own error, measured 6.6e-7, with margin — not a tolerance on the device, which must equal the restatement byte
for byte), the seam at +-0, the golden bytes of the header, the whole coding against the same formulas in float64 with the true
arctan2 (no byte off by more than 1, at most 1e-3 of the bytes off at all: about ten times the restatement's measured 8e-5),
the treatment of unknown pixels and the integer blend.  No GPU."""
import numpy as np
import pytest

from tests import flow_colour_ref as R

F32 = np.float32


def test_the_wheel_has_the_check_values_and_column_sums():
    W = R.colour_wheel()
    assert W.shape == (55, 3) and W.dtype == np.uint8
    want = {0: (255, 0, 0), 14: (255, 238, 0), 15: (255, 255, 0), 20: (43, 255, 0), 21: (0, 255, 0), 24: (0, 255, 191),
            25: (0, 255, 255), 35: (0, 24, 255), 36: (0, 0, 255), 48: (235, 0, 255), 49: (255, 0, 255), 54: (255, 0, 43)}
    for k, rgb in want.items():
        assert tuple(W[k]) == rgb, k
    assert W.astype(int).sum(0).tolist() == [7773, 5870, 7395]


def test_the_package_exports_the_same_wheel():
    import denseflow_amd

    assert np.array_equal(denseflow_amd.colour_wheel(), R.colour_wheel())
    assert denseflow_amd.colour_wheel().dtype == np.uint8


def test_atan2_turns_is_within_1e_6_half_turns_of_arctan2():
    rng = np.random.default_rng(20110301)
    y, x = rng.standard_normal(2_000_000).astype(F32), rng.standard_normal(2_000_000).astype(F32)
    axes = np.array([(0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (3, 3), (-2.5, 2.5), (1e-30, 1e-30),
                     (1e20, -1e20), (0, 1e-40), (1e-40, 0), (-1e-40, -1e-40)], F32)
    y, x = np.concatenate([y, axes[:, 0]]), np.concatenate([x, axes[:, 1]])
    a = R.atan2_turns(y, x)
    assert a.dtype == F32
    err = np.abs(a.astype(np.float64) - np.arctan2(y.astype(np.float64), x.astype(np.float64)) / np.pi)
    print(f"atan2_turns: max error {err.max():.3g} half-turns")
    assert err.max() <= 1e-6
    assert np.all(np.abs(a) <= 1)


def test_the_eight_zero_sign_combinations_agree_with_arctan2_in_quadrant():
    for y in (F32(0.0), F32(-0.0)):
        for x in (F32(0.0), F32(-0.0), F32(1.0), F32(-1.0)):
            got = float(R.atan2_turns(np.array([y]), np.array([x]))[0])
            want = float(np.arctan2(np.float64(y), np.float64(x)) / np.pi)
            assert abs(got - want) <= 1e-6 and np.signbit(got) == np.signbit(want), (y, x, got, want)
    # and a zero x with either sign of a nonzero y
    for y in (F32(1.0), F32(-1.0)):
        for x in (F32(0.0), F32(-0.0)):
            got = float(R.atan2_turns(np.array([y]), np.array([x]))[0])
            assert abs(got - float(np.arctan2(np.float64(y), np.float64(x)) / np.pi)) <= 1e-6


def test_the_golden_bytes_of_the_header():
    s = F32(1) / np.sqrt(F32(2))
    vecs = [(1, 0), (0, 1), (-1, 0), (0, -1), (s, s), (0, 0), (0.5, 0)]
    fl = np.zeros((1, 2, 1, len(vecs)), F32)
    for k, (u, v) in enumerate(vecs):
        fl[0, 0, 0, k], fl[0, 1, 0, k] = u, v
    want = [(255, 0, 0), (255, 229, 0), (0, 209, 255), (88, 0, 255), (255, 114, 0), (255, 255, 255), (255, 127, 127)]
    for norm in ("flow", "batch"):
        img, m2 = R.flow_colour(fl, norm)
        assert m2.tolist() == [1.0, 1.0]
        assert [tuple(p) for p in img[0, 0]] == want, norm
    bgr, _ = R.flow_colour(fl, "flow", order="bgr", layout="chw")
    assert bgr.shape == (1, 3, 1, len(vecs)) and [tuple(p[::-1]) for p in bgr[0, :, 0].T] == want
    one = np.array([1, 0], F32).reshape(1, 2, 1, 1)
    assert R.flow_colour(one, "fixed", max_rad=0.5)[0].ravel().tolist() == [191, 0, 0]
    # the seam: the sign of a zero v decides between the two ends of the wheel
    assert R.flow_colour(np.array([1, 0.0], F32).reshape(1, 2, 1, 1), "flow")[0].ravel().tolist() == [255, 0, 0]
    assert R.flow_colour(np.array([1, -0.0], F32).reshape(1, 2, 1, 1), "flow")[0].ravel().tolist() == [255, 0, 43]


def _colour_f64(flows, norm, max_rad=None):
    """The same formulas in float64 with the true arctan2: (RGB bytes (n, H, W, 3), rad before any clamp)."""
    fl = flows.astype(np.float64)
    u, v = fl[:, 0], fl[:, 1]
    n = fl.shape[0]
    m2 = (u * u + v * v).reshape(n, -1).max(1)
    Rr = {"fixed": np.full(n, max_rad or 0.0), "flow": np.sqrt(m2), "batch": np.full(n, np.sqrt(m2.max()))}[norm]
    D = (Rr + 2.0 ** -23).reshape(n, 1, 1)
    un, vn = u / D, v / D
    rad = np.sqrt(un * un + vn * vn)
    raw = rad
    if norm != "fixed":
        rad = np.minimum(rad, 1.0)
    a = np.arctan2(-vn, -un) / np.pi
    fk = np.clip((a + 1.0) * 27.0, 0.0, 54.0)
    k0 = np.floor(fk).astype(int)
    f = (fk - k0)[..., None]
    k1 = np.where(k0 == 54, 0, k0 + 1)
    wheel = R.colour_wheel().astype(np.float64) / 255.0
    col = (1.0 - f) * wheel[k0] + f * wheel[k1]
    rad3 = rad[..., None]
    col = np.where(rad3 <= 1.0, 1.0 - rad3 * (1.0 - col), col * 0.75)
    return np.clip(np.floor(255.0 * col), 0, 255).astype(np.uint8), raw


def _noise_flow(rng, n, h, w, mag):
    return (rng.standard_normal((n, 2, h, w)) * mag).astype(F32)


@pytest.mark.parametrize("w,h", [(97, 61), (131, 97)])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
def test_the_restatement_against_float64_with_the_true_arctan2(w, h, kind):
    from tests.fb_check_ref import smooth_flow

    rng = np.random.default_rng(7 * w + h + len(kind))
    flows = smooth_flow(rng, 3, h, w, 12.0) if kind == "smooth" else _noise_flow(rng, 3, h, w, 4.0)
    for norm, max_rad in (("flow", None), ("batch", None), ("fixed", 5.0)):
        got, _ = R.flow_colour(flows, norm, max_rad=max_rad)
        want, raw = _colour_f64(flows, norm, max_rad)
        keep = np.ones(raw.shape, bool)
        if norm == "fixed":
            keep = np.abs(raw - 1.0) >= 1e-5  # the branch's discontinuity
            assert (~keep).mean() <= 1e-3, "the inputs put too many pixels on the discontinuity"
            assert 0.05 < (raw > 1).mean() < 0.95  # both branches are taken
        d = np.abs(got.astype(int) - want.astype(int))[keep]
        print(f"{w}x{h} {kind} {norm}: {(d != 0).mean():.3g} of the bytes differ, max {d.max()}, left out {(~keep).mean():.3g}")
        assert d.max() <= 1
        assert (d != 0).mean() <= 1e-3


def test_unknown_values_are_marked_and_left_out_of_the_maximum():
    h, w = 9, 13
    rng = np.random.default_rng(5)
    fl = _noise_flow(rng, 1, h, w, 2.0)
    where = R.plant_specials(fl[0])
    unknown = (7, 8, 9)
    img, m2 = R.flow_colour(fl, "flow", unknown=unknown)
    k = R.known(fl)[0]
    for name in ("nan_u", "nan_v", "+inf", "-inf", "1e30", "-1e30", "above_1e9"):
        x, y = where[name]
        assert not k[y, x] and tuple(img[0, y, x]) == unknown, name
    for name in ("1e9", "-0.0", "u1_v+0", "u1_v-0"):
        x, y = where[name]
        assert k[y, x], name
    assert m2[0] == F32(1e9) * F32(1e9) and m2[1] == m2[0]  # 1e9 is known and then the maximum
    x, y = where["-0.0"]
    assert tuple(img[0, y, x]) == (255, 255, 255)
    assert np.isfinite(m2).all()


def test_masked_pixels_are_excluded_and_a_masked_maximum_changes_the_rest():
    h, w = 7, 11
    rng = np.random.default_rng(6)
    fl = _noise_flow(rng, 2, h, w, 1.0)
    fl[0, :, 3, 4] = (40.0, -30.0)  # the maximum of flow 0, by far
    mask = np.zeros((2, h, w), np.uint8)
    open_img, open_m2 = R.flow_colour(fl, "flow")
    mask[0, 3, 4] = 255
    img, m2 = R.flow_colour(fl, "flow", mask=mask, unknown=(1, 2, 3))
    assert open_m2[0] == F32(2500) and m2[0] < F32(40) and m2[1] == open_m2[1]
    assert tuple(img[0, 3, 4]) == (1, 2, 3)
    rest = np.ones((h, w), bool)
    rest[3, 4] = False
    assert (img[0][rest] != open_img[0][rest]).any(), "the masked maximum did not change the colours of the rest"
    assert np.array_equal(img[1], open_img[1])
    # batch: MB2 follows
    assert R.flow_colour(fl, "batch", mask=mask)[1][2] == max(m2[0], m2[1])


def test_all_unknown_and_all_zero_flows():
    h, w = 5, 6
    fl = np.full((2, 2, h, w), np.nan, F32)
    fl[1] = 0
    for norm in ("flow", "batch"):
        img, m2 = R.flow_colour(fl, norm, unknown=(10, 20, 30))
        assert m2.view(np.uint32).tolist() == [0, 0, 0]  # +0
        assert np.all(img[0] == np.array([10, 20, 30], np.uint8))
        assert np.all(img[1] == 255)
    mask = np.ones((2, h, w), np.uint8)
    img, m2 = R.flow_colour(np.ones((2, 2, h, w), F32), "flow", mask=mask, order="bgr", unknown=(10, 20, 30))
    assert m2.view(np.uint32).tolist() == [0, 0, 0] and np.all(img == np.array([10, 20, 30], np.uint8))


def test_the_blend_is_the_integer_formula():
    h, w = 6, 9
    rng = np.random.default_rng(8)
    fl = _noise_flow(rng, 2, h, w, 3.0)
    fl[1, 0, 2, 2] = np.nan  # unknown pixels are blended too
    plain, _ = R.flow_colour(fl, "flow", order="bgr", unknown=(9, 99, 199))
    gray = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    bgr = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    for a in (0, 256, 77):
        for frame, f3 in ((gray, np.repeat(gray[..., None], 3, -1)), (bgr, bgr)):
            got, _ = R.flow_colour(fl, "flow", order="bgr", unknown=(9, 99, 199), frame=frame, alpha256=a)
            want = (a * plain.astype(int) + (256 - a) * f3.astype(int) + 128) >> 8
            assert np.array_equal(got, want), a
            if a == 0:
                assert np.array_equal(got, f3)
            if a == 256:
                assert np.array_equal(got, plain)
        chw, _ = R.flow_colour(fl, "flow", order="bgr", layout="chw", unknown=(9, 99, 199), frame=bgr.transpose(0, 3, 1, 2),
                               frame_layout="chw", alpha256=a)
        hwc, _ = R.flow_colour(fl, "flow", order="bgr", unknown=(9, 99, 199), frame=bgr, alpha256=a)
        assert np.array_equal(chw, hwc.transpose(0, 3, 1, 2))
