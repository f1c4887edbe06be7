"""-a=tvl1 with the illumination channel (dfx_params.tvl1_gamma != 0) on the device: the fused tile kernel with the third
channel (impl 0) and the simple kernel with it (impl 1) against the three-channel reference of tests/tvl1_gamma_ref.py.
The device arithmetic is the reference's operation for operation, so every comparison is np.array_equal of the flows AND
equality of the executed inner-iteration table and the number of convergence sums evaluated.

Shapes (the smallest at which the tile kernel can go wrong): 97x61 (a second 64-column tile of 33 columns, a height that is
no multiple of 4 or 32), 130x97 (a third tile of two columns), 65x17 (a second tile of one column, one level), 65x33 (the
same tile split with two levels).  Four frames with max_batch = 2 are three pairs in a full batch and a ragged one.
gamma 0.4 at the default iteration count exits early at every level; gamma 2.0 with tvl1_iterations = 41 runs every warp to
the cap, and 41 is no multiple of any fusion K.  The reference is computed once per case and shared; that each gamma moves
the reference's flow away from the gamma = 0 flow is asserted in tests/test_tvl1_gamma_ref.py and again here, on reference
output, before an engine is touched."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import tvl1_gamma_ref as GR

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
DISCRIMINATION = 1e-3  # px
SIZES = {(97, 61): 9, (130, 97): 5, (65, 17): 4, (65, 33): 4}  # (w, h) -> SynthClip seed
FORMS = {"tuned": dict(), "impl1": dict(impl=1)}
SET_F = dict(tau=0.1, lam=0.05, theta=0.5, scale_step=0.6, nscales=6)  # reference keywords
_ENGINE_NAME = dict(tau="tvl1_tau", lam="tvl1_lambda", theta="tvl1_theta", scale_step="tvl1_scale_step",
                    nscales="tvl1_nscales", iterations="tvl1_iterations")

_clips, _refs = {}, {}


def _frames(w, h, n=4):
    if (w, h) not in _clips:
        _clips[(w, h)] = SynthClip(w, h, SIZES[(w, h)]).frames(n)
    return _clips[(w, h)]


def _engine_kw(ref_kw):
    return {_ENGINE_NAME[k]: v for k, v in ref_kw.items()}


def _ref_pairs(key, pairs, gamma, **ref_kw):
    """The reference's (flow, u3, table, checks) of each pair, computed once per key and never changed."""
    key = (key, gamma, tuple(sorted(ref_kw.items())))
    if key not in _refs:
        out = []
        for f0, f1 in pairs:
            r = GR.tvl1_gamma_calc(f0, f1, gamma, **ref_kw)
            r[0].setflags(write=False)
            out.append(r)
        _refs[key] = out
    return _refs[key]


def _ref(w, h, gamma, **ref_kw):
    fr = _frames(w, h)
    return _ref_pairs((w, h), list(zip(fr[:-1], fr[1:])), gamma, **ref_kw)


def _discriminates(w, h, gamma, **ref_kw):
    ref, base = _ref(w, h, gamma, **ref_kw), _ref(w, h, 0.0, **ref_kw)
    diffs = [float(np.max(np.abs(a[0] - b[0]))) for a, b in zip(ref, base)]
    print(f"gamma {gamma} {w}x{h} {ref_kw}: reference against gamma 0, max-abs per pair {diffs}; "
          f"inner iterations {[sum(map(sum, r[2])) for r in ref]}")
    assert all(np.isfinite(r[0]).all() and np.isfinite(r[1]).all() for r in ref)
    assert min(diffs) > DISCRIMINATION, (gamma, w, h, diffs)


def _table(st, warps=5):
    return [r[:warps] for r in st.iters_table()]


def _check(dfx, w, h, gamma, form_kw, **ref_kw):
    _discriminates(w, h, gamma, **ref_kw)
    ref, frames = _ref(w, h, gamma, **ref_kw), _frames(w, h)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2, tvl1_gamma=gamma, **_engine_kw(ref_kw), **form_kw) as eng:
        flows = eng.calc_optflows(frames, 1)  # 3 pairs: a batch of two and a ragged one
        st = eng.stats()
        assert _table(st) == ref[-1][2], "inner-iteration counts differ from the reference (last pair)"
        assert st.tvl1_checks == ref[-1][3]
        first = eng.calc(frames[0], frames[1])
        st = eng.stats()
    assert _table(st) == ref[0][2], "inner-iteration counts differ from the reference (first pair)"
    assert st.tvl1_checks == ref[0][3]
    assert len(flows) == len(ref)
    for i, (got, r) in enumerate(zip(flows, ref)):
        assert np.array_equal(got, r[0]), f"gamma {gamma} {w}x{h} {form_kw}: pair {i} differs, max-abs {np.max(np.abs(got - r[0]))}"
    assert np.array_equal(first, ref[0][0])
    return flows


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w,h", list(SIZES))
def test_gamma_04_matches_the_reference(dfx, w, h, form):
    _check(dfx, w, h, 0.4, FORMS[form])
    assert any(n < 300 for r in _ref(w, h, 0.4) for row in r[2] for n in row)  # early exits are part of the case


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("w,h", [(97, 61), (65, 33)])
def test_gamma_2_capped_at_41_iterations(dfx, w, h, form):
    _check(dfx, w, h, 2.0, FORMS[form], iterations=41)
    capped = [n == 41 for r in _ref(w, h, 2.0, iterations=41) for row in r[2] for n in row]
    # 97x61: every warp of every level runs to the cap; 65x33: most do (some warps of its coarse level converge earlier)
    assert all(capped) if (w, h) == (97, 61) else sum(capped) > len(capped) // 2


@pytest.mark.parametrize("form", list(FORMS))
def test_gamma_2_full_length_one_level(dfx, form):
    _check(dfx, 65, 17, 2.0, FORMS[form])


@pytest.mark.parametrize("w,h", [(97, 61), (130, 97)])
def test_every_fusion_depth_gives_the_same_bits(dfx, w, h):
    """tvl1_fuse_k 1, 3, 4 and the largest the tile supports (tvl1_fused_max_k(), asked of the library): all the reference's
    bits.  97x61 has border tiles only.  130x97 has an interior tile (the DPP path without border selects, lanes 0 / 63 fed
    by the halo alone) at level 0 for every K <= 12: tile column 1 starts at x = 64 - 2K >= 1 and ends before 130, tile row
    2 starts at y = 64 - 5K >= 1 and ends before 97."""
    k_max = dfx.load_library().dfxi_tvl1_fused_max_k()
    assert k_max >= 4
    for k in sorted({1, 3, 4, k_max}):
        _check(dfx, w, h, 0.4, dict(tvl1_fuse_k=k))


def test_brightness_step_and_unrelated_frames_stay_finite(dfx):
    """Large |gamma * u3| (a +20 grey-level step) and erratic flows (two unrelated clips): finite, and the reference's bits."""
    w, h = 97, 61
    f0, f1 = _frames(w, h)[:2]
    bright = np.clip(f1.astype(np.int32) + 20, 0, 255).astype(np.uint8)
    other = SynthClip(w, h, 23).frame(0)
    pairs = [(f0, bright), (f0, other)]
    ref = _ref_pairs("hard", pairs, 2.0, iterations=41)
    print("max |gamma*u3| per pair", [float(np.max(np.abs(2.0 * r[1]))) for r in ref],
          "max |flow|", [float(np.max(np.abs(r[0]))) for r in ref])
    for form_kw in FORMS.values():
        with dfx.FlowEngine(w, h, "tvl1", tvl1_gamma=2.0, tvl1_iterations=41, **form_kw) as eng:
            for (a, b), r in zip(pairs, ref):
                got = eng.calc(a, b)
                st = eng.stats()
                assert np.isfinite(got).all()
                assert np.array_equal(got, r[0]), np.max(np.abs(got - r[0]))
                assert _table(st) == r[2] and st.tvl1_checks == r[3]


@pytest.mark.parametrize("form", list(FORMS))
def test_gamma_with_a_non_default_parameter_set(dfx, form):
    _check(dfx, 130, 97, 0.4, FORMS[form], **SET_F)


def test_planar_and_u8_outputs(dfx, oracle):
    w, h = 130, 97
    ref, frames = _ref(w, h, 0.4), _frames(w, h)
    want = np.stack([r[0] for r in ref]).transpose(0, 3, 1, 2)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=2, tvl1_gamma=0.4) as eng:
        raw = eng.calc_optflows_planar(frames, 1)
        bounded = eng.calc_optflows_planar(frames, 1, bound=20)
        img_x, img_y = eng.calc_optflows_u8(frames, 1, 20)
    assert np.array_equal(raw, want)
    assert np.array_equal(bounded, np.clip(want, np.float32(-20), np.float32(20)) / np.float32(20))
    for i, r in enumerate(ref):
        ox, oy = oracle.flow_to_u8(r[0], -20, 20)
        assert np.array_equal(img_x[i], ox) and np.array_equal(img_y[i], oy), i


def test_set_size_replans_with_the_handles_own_plane_count(dfx):
    sizes = [(130, 97), (65, 33), (130, 97)]
    kw = dict(max_batch=2, tvl1_gamma=0.4)
    fresh = {s: _check(dfx, *s, 0.4, dict()) for s in set(sizes)}
    held = []
    with dfx.FlowEngine(*sizes[0], "tvl1", **kw) as eng:
        for w, h in sizes:
            eng.set_size(w, h)
            got = eng.calc_optflows(_frames(w, h), 1)
            st = eng.stats()
            assert _table(st) == _ref(w, h, 0.4)[-1][2] and st.tvl1_checks == _ref(w, h, 0.4)[-1][3]
            for i, (a, b) in enumerate(zip(got, fresh[(w, h)])):
                assert np.array_equal(a, b), f"after set_size({w}, {h}): pair {i} differs"
            held.append(eng.device_bytes())
    assert held[2] == held[0], held
    with dfx.FlowEngine(130, 97, "tvl1", max_batch=2) as a, dfx.FlowEngine(130, 97, "tvl1", max_batch=2, tvl1_gamma=0.0) as b, \
            dfx.FlowEngine(130, 97, "tvl1", max_batch=2, tvl1_gamma=-0.0) as c:
        plain = a.device_bytes()
        assert b.device_bytes() == plain and c.device_bytes() == plain
    with dfx.FlowEngine(130, 97, "tvl1", **kw) as g:
        # 6 more planes of round_up(130, 64) x 97 floats in each of the batch's pair slots
        assert g.device_bytes() - plain == 2 * 6 * 192 * 97 * 4


def test_default_path_is_untouched(dfx, oracle):
    w, h = 224, 224
    f0, f1 = SynthClip(w, h, 5).frames(2)
    want, tr = oracle.tvl1_calc(f0, f1, want_trace=True)
    with dfx.FlowEngine(w, h, "tvl1", tvl1_gamma=0.4) as eng:
        with_gamma = eng.calc(f0, f1)
    assert np.isfinite(with_gamma).all() and not np.array_equal(with_gamma, want)
    for kw in (dict(), dict(tvl1_gamma=0.0)):
        with dfx.FlowEngine(w, h, "tvl1", **kw) as eng:
            got = eng.calc(f0, f1)
            st = eng.stats()
        assert np.array_equal(got, want), kw
        assert _table(st) == [r[:5] for r in tr.iters_table()] and st.tvl1_checks == tr.n_checks


@pytest.mark.parametrize("kw,w,h,status", [
    (dict(tvl1_gamma=float("nan")), 97, 61, INVALID),
    (dict(tvl1_gamma=float("inf")), 97, 61, INVALID),
    (dict(tvl1_gamma=0.4, impl=2), 97, 61, UNSUPPORTED),
    (dict(tvl1_gamma=0.4, tvl1_math=1), 97, 61, UNSUPPORTED),
    (dict(tvl1_gamma=0.4, tvl1_math=2), 97, 61, UNSUPPORTED),
    (dict(tvl1_gamma=0.4, tvl1_math=3), 97, 61, UNSUPPORTED),
    (dict(tvl1_gamma=0.4, tvl1_iterations=0), 97, 61, UNSUPPORTED),  # no update would run; the gamma route needs iterations > 0
    (dict(tvl1_gamma=0.4, tvl1_iterations=0, impl=1), 97, 61, UNSUPPORTED),
    (dict(tvl1_gamma=0.4), 8192, 5958, INVALID),  # 22 planes x 4 B x 8192 x 5958 = 2^32 + 360 448: refused before any allocation
])
def test_refusals(dfx, kw, w, h, status):
    dfx.load_library()
    free_before = _free_device_bytes()
    with pytest.raises(dfx.DfxError) as e:
        dfx.FlowEngine(w, h, "tvl1", **kw)
    assert e.value.status == status
    if w == 8192:
        assert "88 B" in str(e.value)
        # nothing was allocated: a single work plane of that size is 8192 x 5958 x 4 B = 195 MB (a pair slot 4 GiB), so
        # free device memory has not gone down by as much as one plane
        held = free_before - _free_device_bytes()
        print(f"free device memory before the refused create {free_before}, taken by it {held}")
        assert held < 8192 * 5958 * 4


def _free_device_bytes():
    """hipMemGetInfo's free bytes of the current device, asked of the HIP runtime the library itself is linked to."""
    import ctypes as C

    with open("/proc/self/maps") as f:  # the very runtime the loaded library uses
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    free, total = C.c_size_t(0), C.c_size_t(0)
    for _ in range(2):  # the first call may create the device context, which takes memory itself
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_gamma_is_ignored_by_farneback(dfx):
    w, h = 97, 61
    f0, f1 = _frames(w, h)[:2]
    with dfx.FlowEngine(w, h, "farn") as a, dfx.FlowEngine(w, h, "farn", tvl1_gamma=0.4) as b:
        assert a.device_bytes() == b.device_bytes()
        assert np.array_equal(a.calc(f0, f1), b.calc(f0, f1))
