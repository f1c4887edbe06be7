"""Properties of the NumPy restatement of the forward projection (tests/flow_project_ref.py): the vectorised form equals the
scalar loop on random, special and colliding inputs; an integer translation inverts exactly with the uncovered strip as its
holes; the inverse of an affine flow stays within the bound its Lipschitz constant gives; all pixels converging on one target
give one pixel of coverage W * H holding the integer mean; t = 0.5 gives half the flow and fewer holes; importance decides a
collision.  The quality record on the CPU oracle's flows is printed, not asserted (profiles/flow_project/quality.txt holds
the printed lines).  No GPU is touched."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import flow_project_ref as R
from tests.fb_check_ref import fb_check
from tests.flow_median_ref import flow_median_ref

F32, F64, U32 = np.float32, np.float64, np.uint32
W, H = 97, 61


def _planes(flow_hw2):
    return np.ascontiguousarray(np.moveaxis(np.asarray(flow_hw2, F32), -1, 0))


def _random_bits(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(U32).view(F32)


def _same(a, b):
    return all(R.same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("w,h", [(1, 1), (5, 1), (13, 9), (23, 17)])
def test_the_vectorised_form_equals_the_scalar_loop(w, h):
    rng = np.random.default_rng(490 + w)
    flows, imp, occ = R.project_inputs(w, h, n=2)
    flows[1] = np.round(flows[1])  # landings exactly on integers
    imp.reshape(-1)[:7 % imp.size or 1] = F32(np.nan)
    for k, v in enumerate((0.0, -1.0, 1e-3, 256.0, 1e9, np.inf)):
        imp.reshape(-1)[(3 + 5 * k) % imp.size] = F32(v)
    for t, scale, mw in ((1.0, None, 0.25), (0.5, 0.5, 0.0), (-1.0, 1.0, 1.0), (0.25, 0.75, 0.25)):
        for i, o in ((None, None), (imp, None), (None, occ), (imp, occ)):
            kw = dict(t=t, scale=scale, importance=i, occ=o, min_weight=mw)
            assert _same(R.project(flows, **kw), R.project_loop(flows, **kw)), (w, h, kw)
    special = flows.copy()
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 1e-40, -1e-40, -1.0, np.nextafter(F32(-1), F32(0)), float(w), float(h)]
    for k, v in enumerate(vals):
        special[k % 2, k % 2].reshape(-1)[(2 * k + 1) % (w * h)] = F32(v)
    bits = _random_bits(rng, (2, 2, h, w))
    for fl in (special, bits, (flows.astype(F64) * 1e-39).astype(F32)):
        for t in (1.0, -1.0, 0.25):
            assert _same(R.project(fl, t=t, importance=imp, occ=occ), R.project_loop(fl, t=t, importance=imp, occ=occ))
            assert _same(R.project(fl, t=t), R.project_loop(fl, t=t))


def test_the_edges_of_the_landing_test():
    """Exactly -1 and exactly W are skipped, one ulp inside them lands (with weight 0 on the dropped tap's neighbour or not at
    all), and a landing on an integer puts the whole weight on one tap."""
    w, h = 13, 9
    for x, land, cov_at in ((5, -1.0, None), (5, float(w), None), (5, float(np.nextafter(F32(-1), F32(0))), None),
                            (5, float(np.nextafter(F32(w), F32(0))), None), (5, 7.0, 7), (5, 12.0, 12), (5, 0.0, 0), (5, 6.5, 6)):
        flow = np.full((1, 2, h, w), np.nan, F32)
        flow[0, :, 4, x] = (F32(land) - F32(x), 0.0)
        out, hole, cov = R.project(flow, min_weight=0.0)
        assert _same((out, hole, cov), R.project_loop(flow, min_weight=0.0))
        if cov_at is None:  # one ulp inside W rounds to bx = 256 on the dropped column, one ulp inside -1 to bx = 0 on it
            assert hole.all() and not cov.any(), land
        elif land == 6.5:
            assert cov[0, 4, 6] == 0.5 and cov[0, 4, 7] == 0.5 and cov.sum() == 1.0
        else:
            assert cov[0, 4, cov_at] == 1.0 and cov.sum() == 1.0 and hole.sum() == w * h - 1


def test_an_integer_translation_inverts_exactly_and_leaves_the_uncovered_strip():
    flows = np.empty((1, 2, H, W), F32)
    flows[0, 0], flows[0, 1] = 3.0, -2.0
    out, hole, cov = R.project(flows, t=1.0, scale=-1.0)
    live = hole[0] == 0
    assert (out[0, 0][live] == -3.0).all() and (out[0, 1][live] == 2.0).all() and (cov[0][live] == 1.0).all()
    strip = np.ones((H, W), bool)
    strip[:H - 2, 3:] = False  # targets (x + 3, y - 2): columns 3 .. W-1 of rows 0 .. H-3
    assert np.array_equal(hole[0] != 0, strip) and int(hole.sum()) == 371
    assert (out[0][:, ~live] == 0).all() and not np.signbit(out[0][:, ~live]).any() and (cov[0][~live] == 0).all()


def _affine(A, b):
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u = A[0, 0] * (xx - cx) + A[0, 1] * (yy - cy) + b[0]
    v = A[1, 0] * (xx - cx) + A[1, 1] * (yy - cy) + b[1]
    return np.stack([u, v])


AFFINE_A, AFFINE_B = np.array([[0.04, -0.02], [0.025, 0.03]]), np.array([1.3, -0.7])


def test_the_inverse_of_an_affine_flow_stays_within_its_lipschitz_bound():
    """F(p) = A (p - c) + b with L = ||A||_2.  A source s that contributes to target q lands within 1 px per axis of q,
    |s + F(s) - q| < sqrt 2; the true preimage p* has p* + F(p*) = q; so |(I + A)(s - p*)| < sqrt 2, |s - p*| < sqrt 2 / (1 - L),
    |F(s) - F(p*)| < sqrt 2 L / (1 - L).  The output is a convex combination of the -F(s), each quantised to 1/256 px."""
    L = float(np.linalg.norm(AFFINE_A, 2))
    assert 0.04 < L < 0.06
    flow = _affine(AFFINE_A, AFFINE_B)
    out, hole, _ = R.project(flow[None].astype(F32), t=1.0, scale=-1.0)
    # the analytic inverse at target q: p* = c + (I + A)^-1 (q - c - b), F_inv(q) = p* - q
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    c = np.array([(W - 1) / 2, (H - 1) / 2])
    q = np.stack([xx - c[0] - AFFINE_B[0], yy - c[1] - AFFINE_B[1]])
    p = np.einsum("ij,jhw->ihw", np.linalg.inv(np.eye(2) + AFFINE_A), q)
    inv = np.stack([p[0] + c[0] - xx, p[1] + c[1] - yy])
    live = hole[0] == 0
    err = float(np.sqrt(((out[0] - inv) ** 2).sum(0))[live].max())
    bound = np.sqrt(2.0) * L / (1.0 - L) + 1.0 / 256.0
    print(f"affine flow, L = {L:.4f}: max |projected inverse - analytic inverse| {err:.4f} px, bound {bound:.4f} px, "
          f"hole share {1 - live.mean():.4f}")
    assert err <= bound and 0.0 < 1 - live.mean() < 0.05


def test_all_pixels_converging_on_one_target():
    tx, ty = 40, 25
    yy, xx = np.mgrid[0:H, 0:W]
    flow = np.stack([tx - xx, ty - yy]).astype(F32)[None]
    out, hole, cov = R.project(flow, t=1.0, scale=-1.0, min_weight=0.0)
    assert int((hole == 0).sum()) == 1 and hole[0, ty, tx] == 0 and cov[0, ty, tx] == 5917.0 == W * H
    su, sv = int((256 * (tx - xx)).sum()), int((256 * (ty - yy)).sum())
    want = [F32((F64(s) / F64(W * H)) * (F64(-1.0) / 256.0)) for s in (su, sv)]
    assert out[0, 0, ty, tx] == want[0] and out[0, 1, ty, tx] == want[1]
    assert abs(float(out[0, 0, ty, tx]) + (tx - (W - 1) / 2)) < 1e-5 and abs(float(out[0, 1, ty, tx]) + (ty - (H - 1) / 2)) < 1e-5
    assert _same((out, hole, cov), R.project_loop(flow, t=1.0, scale=-1.0, min_weight=0.0))


def test_half_way_gives_half_the_flow_and_fewer_holes():
    """At t = 0.5 a contributing source s has |s + F(s)/2 - q| < sqrt 2, so |s - q| < sqrt 2 + max|F| / 2 and the value
    -F(s)/2 is within L (sqrt 2 + max|F| / 2) / 2 + 1/512 of -F(q)/2."""
    A = 2.0 * AFFINE_A
    L = float(np.linalg.norm(A, 2))
    flow = _affine(A, AFFINE_B)
    f32 = flow[None].astype(F32)
    out1, hole1, _ = R.project(f32, t=1.0)
    out, hole, _ = R.project(f32, t=0.5)
    fmax = float(np.sqrt((flow ** 2).sum(0)).max())
    live = hole[0] == 0
    err = float(np.sqrt(((out[0] + 0.5 * flow) ** 2).sum(0))[live].max())
    bound = 0.5 * L * (np.sqrt(2.0) + 0.5 * fmax) + 1.0 / 512.0
    print(f"t = 0.5: max |out + F/2| {err:.4f} px, bound {bound:.4f} px; hole share {hole.mean():.4f} against {hole1.mean():.4f} at t = 1")
    assert live[H // 2, W // 2] and err <= bound
    assert hole.mean() < hole1.mean()


def test_importance_decides_a_collision():
    """Two constant-flow layers of (+8, 0) and (-8, 0) land on the same integer targets.  With equal importance 2^-8 (iq = 1)
    a target holds their mean, 0; with the first layer at 256 (iq = 65536) it holds (65536 * 8 - 8) / 65537 = 8 - 16 / 65537,
    times scale: within 1/256 px of that layer."""
    flow = np.zeros((1, 2, H, W), F32)
    flow[0, 0, :, :48], flow[0, 0, :, 48:] = 8.0, -8.0
    imp = np.full((1, H, W), 2.0 ** -8, F32)
    out, hole, cov = R.project(flow, scale=1.0, importance=imp, min_weight=0.0)
    both = slice(48, 56)  # targets of sources 40 .. 47 and of sources 56 .. 63
    assert (out[0, 0, :, both] == 0).all() and (hole[0, :, both] == 0).all() and (cov[0, :, both] == F32(2.0 / 256)).all()
    imp[0, :, :48] = 256.0
    out, hole, _ = R.project(flow, scale=1.0, importance=imp, min_weight=0.0)
    d = np.abs(out[0, 0, :, both].astype(F64) - 8.0)
    assert (d > 0).all() and d.max() <= 1.0 / 256.0 and abs(d.max() - 16.0 / 65537.0) <= 2.0 ** -21  # float32 below 8


def _epe(a, b, where):
    d = a.astype(F64) - b.astype(F64)
    return float(np.sqrt(d[0] ** 2 + d[1] ** 2)[where].mean()) if where.any() else float("nan")


@pytest.mark.parametrize("algo", ["tvl1_calc", "farneback_calc"])
@pytest.mark.parametrize("k", [1, 6])
def test_quality_record_on_the_oracles_flows(oracle, algo, k):
    """Recorded, not asserted: the projected inverse of the oracle's forward flow against the oracle's own backward flow, the
    hole plane against fb_check's backward occlusion mask, and both again after a 5 x 5 median fill of the holes."""
    clip = SynthClip(97, 61, 9)
    calc = getattr(oracle, algo)
    fwd, bwd = _planes(calc(clip.frame(0), clip.frame(k))), _planes(calc(clip.frame(k), clip.frame(0)))
    out, hole, cov = R.project(fwd[None], t=1.0, scale=-1.0)
    live = hole[0] == 0
    occ_b = fb_check(bwd, fwd)[0] != 0
    agree = float((occ_b == ~live).mean())
    inter, union = int((occ_b & ~live).sum()), int((occ_b | ~live).sum())
    filled, left = flow_median_ref(out[0], 5, mask=hole[0], mode="fill")
    for _ in range(7):
        if not left.any():
            break
        filled, left = flow_median_ref(filled, 5, mask=left, mode="fill")
    print(f"{algo} SynthClip(97, 61, 9) 0 -> {k}: hole share {1 - live.mean():.3f}, max coverage {cov.max():.2f}; EPE of the projected "
          f"inverse against the oracle's backward flow over non-hole pixels {_epe(out[0], bwd, live):.3f} px; holes against fb_check's "
          f"backward mask (share {occ_b.mean():.3f}): agreement {agree:.3f}, intersection / union {inter} / {union}; after the 5 x 5 "
          f"fill: EPE over all filled pixels {_epe(filled, bwd, left == 0):.3f} px, over the former holes "
          f"{_epe(filled, bwd, ~live & (left == 0)):.3f} px, {int((left != 0).sum())} pixels still unfilled")
    assert np.isfinite(out).all()
