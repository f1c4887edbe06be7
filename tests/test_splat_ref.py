"""Properties of the NumPy restatement of the forward warp (tests/splat_ref.py): the vectorised form equals the scalar loop in
every bit over every source form, mode, hole mode, importance and mask; a zero flow returns the frame byte for byte with no
hole and coverage 1; an integer shift is exact with the holes of the uncovered border; the (u, v) payload of a flow equals the
forward projection of tests/flow_project_ref.py with scale 1 in every bit, which ties the two definitions together; two sources
on one target average by their importances; the order of the sources does not matter; the sum mode conserves mass in integers;
the payload edges.  Quality, asserted as a condition: frame 0 of SynthClip(97, 61, 9) splatted by a flow to frame k is closer to
frame k than frame 0 itself by more than a factor of two, over the pixels that are no holes, with the exact flows for k = 1 and
k = 6 and with the CPU oracle's TVL1 and Farneback flows for k = 1.  The figures themselves are printed
(profiles/splat/quality.txt holds the printed lines).  No GPU is touched."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import flow_project_ref as P
from tests import splat_ref as R

F32, I64, U8 = np.float32, np.int64, np.uint8


def _planes(flow_hw2):
    return np.ascontiguousarray(np.moveaxis(np.asarray(flow_hw2, F32), -1, 0))


@pytest.mark.parametrize("form", ["gray", "hwc", "chw", "f1", "f2", "f3", "f4"])
def test_the_loop_and_the_vectorised_form_agree(form):
    w, h = 23, 11
    gray, bgr, pay, flows, imp, occ = R.splat_inputs(w, h, n=2)
    flows = flows * F32(2)  # more holes and collisions
    img = {"gray": gray, "hwc": bgr, "chw": np.ascontiguousarray(bgr.transpose(0, 3, 1, 2))}.get(form)
    layout = "chw" if form == "chw" else "hwc"
    if img is None:
        img = np.ascontiguousarray(pay[:, :int(form[1])])
    rng = np.random.default_rng(7)
    for t, use_imp, use_occ, mode, holes, dtype in ((1.0, False, False, "mean", "zero", None), (0.5, True, True, "mean", "keep", None),
                                                    (-1.0, True, False, "sum", "zero", F32), (1.0, False, True, "mean", "keep", F32),
                                                    (0.5, True, True, "sum", "keep", F32)):
        kw = dict(t=t, importance=imp if use_imp else None, occ=occ if use_occ else None, mode=mode, holes=holes, dtype=dtype,
                  layout=layout, min_weight=0.25)
        if holes == "keep":
            dt = U8 if dtype is None and img.dtype == U8 else F32
            kw["out"] = rng.integers(1, 200, img.shape).astype(dt)
        a, b = R.splat(img, flows, **kw), R.splat_loop(img, flows, **kw)
        for x, y in zip(a, b):
            assert R.same_bits(x, y)
        assert a[0].shape == img.shape and a[1].any() and not a[1].all()
        if holes == "keep":  # the holes hold what was there, and only they
            cf_out, cf_keep = R.channels_first(a[0], layout, img.dtype == U8)[0], R.channels_first(kw["out"], layout, img.dtype == U8)[0]
            m = np.broadcast_to(a[1][:, None] != 0, cf_out.shape)
            assert np.array_equal(cf_out[m], cf_keep[m])
            zero = R.splat(img, flows, **{**kw, "holes": "zero", "out": None})
            cf_zero = R.channels_first(zero[0], layout, img.dtype == U8)[0]
            assert R.same_bits(cf_out[~m], cf_zero[~m]) and not cf_zero[m].any()


def test_a_zero_flow_returns_the_frame_byte_for_byte():
    frame = SynthClip(97, 61, 9).frame(0)[None]
    out, hole, cov = R.splat(frame, np.zeros((1, 2, 61, 97), F32))
    assert out.dtype == U8 and np.array_equal(out, frame) and not hole.any() and (cov == F32(1)).all()
    bgr = R.splat_inputs(33, 9, n=1)[1]
    for layout, img in (("hwc", bgr), ("chw", np.ascontiguousarray(bgr.transpose(0, 3, 1, 2)))):
        out, hole, cov = R.splat(img, np.zeros((1, 2, 9, 33), F32), layout=layout)
        assert np.array_equal(out, img) and not hole.any() and (cov == F32(1)).all()


def test_an_integer_shift_is_exact_with_the_holes_of_the_border():
    w, h = 97, 61
    frame = SynthClip(w, h, 9).frame(0)[None]
    flow = np.empty((1, 2, h, w), F32)
    flow[:, 0], flow[:, 1] = 3, -2
    out, hole, cov = R.splat(frame, flow)
    assert int(hole.sum()) == 3 * h + 2 * w - 6 == 371
    assert np.array_equal(out[0, :h - 2, 3:], frame[0, 2:, :w - 3])
    assert not hole[0, :h - 2, 3:].any() and hole[0, h - 2:].all() and hole[0, :, :3].all()
    assert not out[hole != 0].any() and set(np.unique(cov)) == {F32(0), F32(1)}


@pytest.mark.parametrize("t,use_imp,use_occ", [(1.0, False, False), (0.5, True, True), (-1.0, True, False)])
def test_the_payload_of_a_flows_own_planes_is_the_forward_projection(t, use_imp, use_occ):
    flows, imp, occ = P.project_inputs(49, 17, n=2)
    flows[0, :, 3, 5] = (np.nan, 1.0)
    flows[1, :, 2, 7] = (1e30, -np.inf)
    kw = dict(t=t, importance=imp if use_imp else None, occ=occ if use_occ else None, min_weight=0.25)
    want = P.project(flows, scale=1.0, **kw)
    got = R.splat(flows, flows, **kw)
    assert got[1].any()
    for g, x in zip(got, want):
        assert R.same_bits(g, x)


def test_two_sources_on_one_target_average_by_their_importances():
    w, h = 5, 3
    img = np.zeros((1, h, w), U8)
    flow = np.full((1, 2, h, w), 1e6, F32)  # everything leaves the frame ...
    imp = np.ones((1, h, w), F32)
    p, q, a, b = 200, 31, 0.7, 3.3
    img[0, 1, 1], img[0, 1, 3] = p, q
    flow[0, :, 1, 1], flow[0, :, 1, 3] = (1, 0), (-1, 0)  # ... but two pixels that meet at (2, 1)
    imp[0, 1, 1], imp[0, 1, 3] = a, b
    out, hole, cov = R.splat(img, flow, importance=imp)
    aq, bq = int(np.rint(F32(a) * F32(256))), int(np.rint(F32(b) * F32(256)))
    assert int(hole.sum()) == w * h - 1 and hole[0, 1, 2] == 0
    assert out[0, 1, 2] == int(np.rint((aq * p + bq * q) / (aq + bq)))
    assert cov[0, 1, 2] == F32((aq + bq) / 256.0)
    outf = R.splat(img, flow, importance=imp, dtype=F32)[0]
    assert outf[0, 1, 2] == F32((aq * p + bq * q) / (aq + bq))


def test_the_order_of_the_sources_does_not_matter():
    w, h = 19, 8
    _, _, pay, flows, imp, occ = R.splat_inputs(w, h, n=1)
    flows = flows * F32(3)
    q, ok = R.payload(pay[0, :3])
    base = R.sums_loop(q, ok, flows[0], 1.0, imp[0], occ[0])
    rng = np.random.default_rng(3)
    for order in (range(w * h - 1, -1, -1), rng.permutation(w * h)):
        got = R.sums_loop(q, ok, flows[0], 1.0, imp[0], occ[0], order)
        assert R.same_bits(got[0], base[0]) and R.same_bits(got[1], base[1])
    vec = R.sums(q, ok, flows[0], 1.0, imp[0], occ[0])
    assert R.same_bits(vec[0], base[0]) and R.same_bits(vec[1], base[1])


def test_the_sum_mode_conserves_mass_in_integers():
    w, h = 31, 7
    gray, bgr, pay, flows, _, _ = R.splat_inputs(w, h, n=1)
    yy, xx = np.mgrid[0:h, 0:w]
    # every landing inside the frame: a contraction towards the centre, off the integer grid
    flow = np.stack([(w / 2 - xx) * 0.37, (h / 2 - yy) * 0.41]).astype(F32)
    for q in (gray[0][None].astype(I64), R.payload(pay[0])[0]):
        ws, s = R.sums(q, np.ones((h, w), bool), flow, 1.0)
        assert int(ws.sum()) == (1 << 24) * w * h
        for c in range(q.shape[0]):
            assert int(s[c].sum()) == (1 << 24) * int(q[c].sum())
    # ... and the stored float sum is S / 2^24 (/ 256 for a float32 source)
    out, hole, cov = R.splat(pay[:1], flow[None], mode="sum", min_weight=0.0)
    ws, s = R.sums(*R.payload(pay[0]), flow, 1.0)
    assert R.same_bits(out[0], (s.astype(np.float64) / 16777216.0 / 256.0).astype(F32))


def test_the_payload_edges():
    edges = R.payload_edges()
    vals = np.array([e[0] for e in edges], F32)
    q, ok = R.payload(vals[None, None, :])
    assert ok[0].tolist() == [e[1] for e in edges]
    assert q[0, 0].tolist() == [e[2] for e in edges]
    # one bad channel skips the whole pixel, the weight included
    w, h = len(edges), 1
    pay = np.ones((1, 2, h, w), F32)
    pay[0, 1, 0] = vals
    out, hole, cov = R.splat(pay, np.zeros((1, 2, h, w), F32), mode="mean")
    assert hole[0, 0].tolist() == [0 if e[1] else 1 for e in edges]
    assert cov[0, 0].tolist() == [1.0 if e[1] else 0.0 for e in edges]
    assert out[0, 0, 0].tolist() == [1.0 if e[1] else 0.0 for e in edges]
    assert out[0, 1, 0].tolist() == [e[2] / 256.0 for e in edges]
    assert not np.signbit(out[out == 0]).any()  # +0 in the holes and for a payload of -0


# ---- quality: frame 0 carried to frame k ----------------------------------------------------------------------------------
def _record(name, f0, fk, flow):
    out, hole, _ = R.splat(f0[None], flow[None])
    keep = hole[0] == 0
    err = float(np.abs(out[0].astype(np.float64) - fk)[keep].mean())
    plain = float(np.abs(f0.astype(np.float64) - fk)[keep].mean())
    share = float(hole.mean())
    print(f"{name}: MAE of frame 0 unwarped {plain:.2f}, of the splat {err:.2f} grey levels (ratio {err / plain:.3f}) over the "
          f"non-hole pixels; hole share {share:.3f}")
    return err, plain, share


@pytest.mark.parametrize("k", [1, 6])
def test_quality_on_the_synthetic_clip_with_the_exact_flows(k):
    clip = SynthClip(97, 61, 9)
    err, plain, _ = _record(f"SynthClip(97, 61, 9) 0 -> {k}, exact flow", clip.frame(0), clip.frame(k), _planes(clip.true_flow(0, k)))
    assert err < 0.5 * plain


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
def test_quality_on_the_synthetic_clip_with_the_oracles_flows(oracle, algo):
    clip = SynthClip(97, 61, 9)
    calc = getattr(oracle, algo)
    err, plain, _ = _record(f"SynthClip(97, 61, 9) 0 -> 1, oracle {algo}", clip.frame(0), clip.frame(1),
                            _planes(calc(clip.frame(0), clip.frame(1))))
    assert err < 0.5 * plain
    # a longer baseline, recorded only
    _record(f"SynthClip(97, 61, 9) 0 -> 6, oracle {algo}", clip.frame(0), clip.frame(6), _planes(calc(clip.frame(0), clip.frame(6))))
