"""tests/plane_warp_ref.py against what it must agree with (no GPU): the 8-bit warp's reference on pictures cast to float32,
the same formula in float64, the exact shifts and ties of nearest sampling, the typed planes' conversions, and its own scalar
loop."""
import numpy as np
import pytest

from tests import plane_warp_ref as R
from tests import reduced_ref, warp_ref

F32 = np.float32


def _flow(seed, h, w):
    rng = np.random.default_rng(seed)
    f = warp_ref.warp_flow(rng, 1, h, w)[0]
    warp_ref.plant_specials(f)
    return f


@pytest.mark.parametrize("border", R.BORDERS)
@pytest.mark.parametrize("form", ["gray", "chw", "hwc"])
def test_a_picture_cast_to_float32_warps_as_the_8_bit_warp_does(form, border):
    h, w = 23, 37
    rng = np.random.default_rng(11)
    flow = _flow(12, h, w)
    occ = (rng.random((h, w)) < 0.2).astype(np.uint8)
    img = rng.integers(0, 256, (h, w) if form == "gray" else (h, w, 3), dtype=np.uint8)
    want, want_valid = warp_ref.warp(img, flow, border, occ)  # float32 samples, zero where not taken
    hwc = img.reshape(h, w, -1).astype(F32)
    if form == "chw":  # through the channels-first form and back
        hwc = R.to_hwc(R.from_hwc(hwc, "chw"), "chw")
    got, valid = R.warp(hwc, flow, "bilinear", border, occ=occ)
    assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.reshape(h, w, -1).view(np.uint32))
    assert np.array_equal(valid, want_valid)


def test_bilinear_stays_within_the_derived_bound_of_float64():
    """Three roundings per lerp step on magnitudes of at most 3 max|tap|: |s - s64| <= 32 * 2^-24 * max|tap|."""
    h, w, c = 64, 96, 3
    worst = 0.0
    for seed, scale in enumerate((1e-3, 1.0, 1e3)):
        rng = np.random.default_rng(100 + seed)
        P = (rng.standard_normal((h, w, c)) * scale).astype(F32)
        flow = warp_ref.warp_flow(rng, 1, h, w)[0]
        s, take = R.bilinear(P, flow, "zero")
        _, _, px, py = R.position(flow, "zero")
        px, py = px.astype(np.float64), py.astype(np.float64)  # the float32 positions, then float64
        x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
        ax, ay = (px - x0)[..., None], (py - y0)[..., None]
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        D = P.astype(np.float64)
        t = D[y0, x0] + ax * (D[y0, x1] - D[y0, x0])
        b = D[y1, x0] + ax * (D[y1, x1] - D[y1, x0])
        s64 = t + ay * (b - t)
        top = np.max(np.abs(np.stack([D[y0, x0], D[y0, x1], D[y1, x0], D[y1, x1]])), axis=0)
        ratio = np.abs(s.astype(np.float64) - s64)[take] / (2.0 ** -24 * top[take])
        worst = max(worst, float(ratio.max()))
        assert take.sum() > 1000
    print(f"worst |s - s64| / (2^-24 max|tap|) = {worst:.2f}")
    assert worst <= 32.0


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32])
def test_nearest_zero_flow_is_the_identity_and_a_whole_flow_the_exact_shift(dtype):
    h, w, c = 9, 13, 2
    rng = np.random.default_rng(5)
    info = np.iinfo(dtype)
    P = rng.integers(info.min, info.max, (h, w, c), dtype=dtype, endpoint=True)
    got, valid = R.warp(P, np.zeros((2, h, w), F32), "nearest")
    assert got.dtype == P.dtype and np.array_equal(got, P) and valid.all()
    flow = np.zeros((2, h, w), F32)
    flow[0], flow[1] = 3, -2
    got, valid = R.warp(P, flow, "nearest")
    want = np.zeros_like(P)
    want[2:, :w - 3] = P[:h - 2, 3:]
    assert np.array_equal(got, want)
    want_mask = np.zeros((h, w), np.uint8)
    want_mask[2:, :w - 3] = 1
    assert np.array_equal(valid, want_mask)


def test_nearest_ties_go_to_even():
    h, w = 1, 8
    P = np.arange(w, dtype=np.int32).reshape(1, w, 1) + 100
    flow = np.zeros((2, h, w), F32)
    flow[0] = 0.5  # x + 0.5: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, .. ; 7.5 leaves the frame
    got, valid = R.warp(P, flow, "nearest")
    assert got[0, :, 0].tolist() == [100, 102, 102, 104, 104, 106, 106, 0]
    assert valid[0].tolist() == [1] * 7 + [0]
    got, _ = R.warp(P, flow, "nearest", border="clamp")
    assert got[0, 7, 0] == 107


def test_nearest_keeps_labels_a_float32_cast_would_lose():
    P = np.array([[[2 ** 24 + 1], [2 ** 31 - 1], [-(2 ** 24) - 3]]], np.int32)
    assert not np.array_equal(P.astype(F32).astype(np.int64), P)  # what a cast through float32 does
    got, _ = R.warp(P, np.zeros((2, 1, 3), F32), "nearest")
    assert np.array_equal(got, P)


def test_nearest_copies_nan_payloads_bit_for_bit():
    bits = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x80000000], np.uint32).reshape(1, 4, 1)
    got, _ = R.warp(bits.view(F32), np.zeros((2, 1, 4), F32), "nearest")
    assert np.array_equal(got.view(np.uint32), bits)


def test_half_sources_convert_exactly_and_results_round_as_the_typed_planes_do():
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f16 = R.to_f32(every, "float16")
    ok = ~np.isnan(f16)
    assert np.array_equal(f16[ok].astype(np.float16).view(np.uint16), every[ok])  # exact: the way back is the identity
    assert f16[1] == F32(2.0 ** -24) and f16[0x03FF] == F32(1023 * 2.0 ** -24)  # subnormals are kept
    assert np.array_equal(R.to_f32(every, "bfloat16").view(np.uint32), every.astype(np.uint32) << 16)
    h, w = 11, 17
    rng = np.random.default_rng(8)
    P = rng.standard_normal((h, w, 2)).astype(F32) * F32(300)
    flow = _flow(9, h, w)
    s, take = R.bilinear(P, flow, "clamp")
    for dt in ("float16", "bfloat16"):
        got, _ = R.warp(P, flow, "bilinear", "clamp", out_dtype=dt)
        want = np.where(take[..., None], reduced_ref.reduce_bits(s, dt).reshape(s.shape), np.uint16(0))
        assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert R.stored(np.array([65520.0, -65520.0, 65519.996], F32), "float16").tolist() == [0x7C00, 0xFC00, 0x7BFF]


@pytest.mark.parametrize("sample", R.SAMPLES)
def test_keep_leaves_everything_outside_valid_untouched(sample):
    h, w, c = 12, 19, 3
    rng = np.random.default_rng(21)
    P = rng.standard_normal((h, w, c)).astype(F32)
    flow = _flow(22, h, w)
    occ = (rng.random((h, w)) < 0.3).astype(np.uint8)
    before = rng.integers(0, 2 ** 32, (h, w, c), dtype=np.uint32).view(F32)
    for border in R.BORDERS:
        got, valid = R.warp(P, flow, sample, border, "keep", occ=occ, out=before)
        fresh, _ = R.warp(P, flow, sample, border, "zero", occ=occ)
        m = valid.astype(bool)
        assert 0 < m.sum() < m.size
        assert np.array_equal(got.view(np.uint32)[~m], before.view(np.uint32)[~m])
        assert np.array_equal(got.view(np.uint32)[m], fresh.view(np.uint32)[m])
    a, _ = R.warp(P, flow, sample, "zero", "keep", occ=occ, out=before)
    b, _ = R.warp(P, flow, sample, "clamp", "keep", occ=occ, out=before)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))  # with keep the border mode changes nothing that is stored


@pytest.mark.parametrize("invalid", ["zero", "keep"])
@pytest.mark.parametrize("border", R.BORDERS)
@pytest.mark.parametrize("sample,src,out", [("bilinear", "float32", "float32"), ("bilinear", "float16", "bfloat16"),
                                            ("bilinear", "bfloat16", "float16"), ("nearest", "float32", None)])
def test_the_vectorised_form_equals_the_scalar_loop(sample, src, out, border, invalid):
    h, w, c = 7, 10, 2
    rng = np.random.default_rng(31)
    P = rng.standard_normal((h, w, c)).astype(F32) * F32(50)
    P[1, 2, 0], P[3, 4, 1], P[2, 2, 0] = np.inf, np.nan, -0.0
    if src != "float32":
        P = R.stored(P, src)
    flow = _flow(32, h, w)
    occ = (rng.random((h, w)) < 0.25).astype(np.uint8)
    n_out = np.uint16 if (out or src) != "float32" else F32
    before = rng.integers(0, 2 ** 16, (h, w, c)).astype(n_out)
    kw = dict(sample=sample, border=border, invalid=invalid, src_dtype=src, out_dtype=out, occ=occ, out=before)
    a, va = R.warp(P, flow, **kw)
    b, vb = R.warp_loop(P, flow, **kw)
    assert np.array_equal(va, vb)
    assert R.same(a, b, None if sample == "nearest" else (out or src))
