"""Both directions of every pair in one call (dfx_calc_batch_bidir_device; FlowEngine.calc_optflows_bidir /
calc_optflows_bidir_device / flow_tensor_bidir): the forward planes are the CPU oracle's flows of (a, b), the backward
planes its flows of (b, a) — bit for bit, and bit for bit what two planar device calls with step and -step give on a second
handle — and the masks are tests/fb_check_ref.py's check of the oracle's flows.  Four frames six apart with max_batch = 2: one
full and one ragged device batch, displacements large enough for real occlusions (tests/test_fb_check_ref.py asserts on the
reference alone that the mask of such a pair discriminates)."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import fb_check_ref as R
from tests.devmem import DevBuf

pytestmark = pytest.mark.gpu

F32 = np.float32
FRAME_IDS = (0, 6, 12, 18)
N, MAX_BATCH = len(FRAME_IDS), 2
ORACLE = {"tvl1": "tvl1_calc", "farn": "farneback_calc", "brox": "brox_calc"}

_frames_cache, _flow_cache = {}, {}


def _frames(w, h):
    if (w, h) not in _frames_cache:
        clip = SynthClip(w, h, 9)
        _frames_cache[(w, h)] = [clip.frame(t) for t in FRAME_IDS]
    return _frames_cache[(w, h)]


def _pairs(step):
    """(a, b) of output flow i: the reference's pair rule (src/denseflow_gpu.cpp:315-316)."""
    return [((i, i + step) if step > 0 else (i - step, i)) for i in range(max(N - abs(step), 0))]


def _oracle_flow(oracle, algo, key, frames, a, b):
    """The oracle's flow frames[a] -> frames[b] as (2, H, W), computed once per (clip, pair) and never changed."""
    k = (algo, key, a, b)
    if k not in _flow_cache:
        flow = getattr(oracle, ORACLE[algo])(frames[a], frames[b])
        flow = np.ascontiguousarray(flow.transpose(2, 0, 1))
        flow.setflags(write=False)
        _flow_cache[k] = flow
    return _flow_cache[k]


def _reference(oracle, algo, key, frames, step):
    """(fwd, bwd, occ_fwd, occ_bwd) as the bidirectional call must return them, from the oracle and fb_check_ref."""
    fwd = np.stack([_oracle_flow(oracle, algo, key, frames, a, b) for a, b in _pairs(step)])
    bwd = np.stack([_oracle_flow(oracle, algo, key, frames, b, a) for a, b in _pairs(step)])
    return fwd, bwd, R.fb_check_batch(fwd, bwd)[0], R.fb_check_batch(bwd, fwd)[0]


def _planar_device(eng, frames, step):
    """calc_optflows_planar_device on dense device buffers: the (M, 2, H, W) flows of `step`."""
    h, w = frames[0].shape
    m = max(len(frames) - abs(step), 0)
    with DevBuf(eng, init=np.stack(frames)) as d_fr, DevBuf(eng, 4 * m * 2 * h * w) as d_out:
        eng.calc_optflows_planar_device(d_fr.ptr(), w, w * h, len(frames), step, None, d_out.ptr(), w, h * w, 2 * h * w)
        return d_out.get(F32).reshape(m, 2, h, w)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# (algorithm, knobs, sizes): TVL1 tuned and simple, Farneback, Brox (at 97 x 61 only: its oracle takes seconds per pair)
CASES = [("tvl1", {}, [(97, 61), (130, 97)]), ("tvl1", dict(impl=1), [(97, 61), (130, 97)]),
         ("farn", {}, [(97, 61), (130, 97)]), ("brox", {}, [(97, 61)])]


@pytest.mark.parametrize("step", [1, -1, 2])
@pytest.mark.parametrize("case,w,h", [(i, w, h) for i, c in enumerate(CASES) for w, h in c[2]])
def test_both_directions_and_masks_are_the_oracles(dfx, oracle, case, w, h, step):
    algo, knobs, _ = CASES[case]
    frames = _frames(w, h)
    fwd_ref, bwd_ref, occ_f_ref, occ_b_ref = _reference(oracle, algo, (w, h), frames, step)
    m = N - abs(step)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH, **knobs) as eng, \
            dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH, **knobs) as twin:
        before = eng.device_bytes()
        fwd, bwd, occ_f, occ_b = eng.calc_optflows_bidir(frames, step)
        after = eng.device_bytes()
        pairs = eng.stats().pairs
        eng.calc_optflows_bidir(frames, step)
        again = eng.device_bytes()
        plain = _planar_device(eng, frames, step)  # a plain planar call after bidirectional ones: still the parent's bits
        twin_before = twin.device_bytes()
        twin_fwd, twin_bwd = _planar_device(twin, frames, step), _planar_device(twin, frames, -step)
        twin_after = twin.device_bytes()
    assert fwd.shape == bwd.shape == (m, 2, h, w) and fwd.dtype == bwd.dtype == F32
    assert occ_f.shape == occ_b.shape == (m, h, w) and occ_f.dtype == occ_b.dtype == np.uint8
    print(f"{algo} {knobs} {w}x{h} step {step}: max-abs fwd {np.max(np.abs(fwd - fwd_ref))} bwd {np.max(np.abs(bwd - bwd_ref))}, "
          f"occluded {occ_f_ref.mean():.3f} / {occ_b_ref.mean():.3f}")
    assert np.array_equal(fwd, fwd_ref) and np.array_equal(bwd, bwd_ref), "not the oracle's flows of (a, b) and (b, a)"
    assert _same(fwd, twin_fwd) and _same(bwd, twin_bwd), "not the planar device calls of step and -step"
    assert _same(plain, twin_fwd), "a planar call after a bidirectional one changed"
    assert np.array_equal(occ_f, occ_f_ref) and np.array_equal(occ_b, occ_b_ref)
    assert 0 < occ_f_ref.mean() < 1 and 0 < occ_b_ref.mean() < 1
    assert pairs == 2 * m
    # nothing is allocated that the planar calls have not allocated: a handle is created with max_batch + 1 frame slots,
    # which |step| = 1 fits (nothing may grow at all); a step of 2 grows the frame ring, for a planar call as for this one
    if abs(step) == 1:
        assert after == before
    assert after - before == twin_after - twin_before and again == after


def test_rgb_channels_first_source(dfx, oracle):
    w, h, ws, hs, step = 97, 61, 150, 90, 1
    gray = [SynthClip(ws, hs, 9).frame(t) for t in FRAME_IDS]
    rgb_chw = [np.stack([g, np.roll(g, 1, 1), 255 - g]) for g in gray]                # (3, hs, ws): R, G, B planes
    prepared = [oracle.prepare_frame(np.ascontiguousarray(f[::-1].transpose(1, 2, 0)), w, h) for f in rgb_chw]  # via BGR
    fwd_ref, bwd_ref, occ_f_ref, occ_b_ref = _reference(oracle, "tvl1", "rgb_chw", prepared, step)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as eng:
        eng.set_source_format(ws, hs, 3, order="rgb", layout="chw")
        fwd, bwd, occ_f, occ_b = eng.calc_optflows_bidir(rgb_chw, step)
    assert np.array_equal(fwd, fwd_ref) and np.array_equal(bwd, bwd_ref)
    assert np.array_equal(occ_f, occ_f_ref) and np.array_equal(occ_b, occ_b_ref)


def test_tvl1_gamma(dfx):
    """The illumination channel: against the three-channel NumPy reference of tests/tvl1_gamma_ref.py (the oracle has no
    gamma), at the size and iteration cap at which that reference takes a second per pair."""
    from tests import tvl1_gamma_ref as GR

    w, h, step, gamma = 65, 33, -1, 2.0
    clip = SynthClip(w, h, 4)
    frames = [clip.frame(t) for t in FRAME_IDS[:3]]
    calc = lambda a, b: np.ascontiguousarray(GR.tvl1_gamma_calc(frames[a], frames[b], gamma, iterations=41)[0].transpose(2, 0, 1))  # noqa: E731
    pairs = [(1, 0), (2, 1)]  # step -1: flow i is frame i + 1 -> frame i
    fwd_ref, bwd_ref = np.stack([calc(a, b) for a, b in pairs]), np.stack([calc(b, a) for a, b in pairs])
    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH, tvl1_gamma=gamma, tvl1_iterations=41) as eng:
        fwd, bwd, occ_f, occ_b = eng.calc_optflows_bidir(frames, step)
        assert eng.stats().pairs == 4
    assert np.array_equal(fwd, fwd_ref) and np.array_equal(bwd, bwd_ref)
    assert np.array_equal(occ_f, R.fb_check_batch(fwd_ref, bwd_ref)[0])
    assert np.array_equal(occ_b, R.fb_check_batch(bwd_ref, fwd_ref)[0])


def test_without_the_check_and_with_other_alphas(dfx, oracle):
    w, h, step = 97, 61, 2
    frames = _frames(w, h)
    fwd_ref, bwd_ref, _, _ = _reference(oracle, "farn", (w, h), frames, step)
    with dfx.FlowEngine(w, h, "farn", max_batch=MAX_BATCH) as eng:
        fwd, bwd, occ_f, occ_b = eng.calc_optflows_bidir(frames, step, check=False)
        _, _, occ_f2, occ_b2 = eng.calc_optflows_bidir(frames, step, alpha1=0.05, alpha2=2.0)
    assert occ_f is None and occ_b is None
    assert np.array_equal(fwd, fwd_ref) and np.array_equal(bwd, bwd_ref)
    assert np.array_equal(occ_f2, R.fb_check_batch(fwd_ref, bwd_ref, 0.05, 2.0)[0])
    assert np.array_equal(occ_b2, R.fb_check_batch(bwd_ref, fwd_ref, 0.05, 2.0)[0])


def test_segments_and_an_empty_buffer(dfx, oracle):
    w, h = 97, 61
    frames = _frames(w, h)
    with dfx.FlowEngine(w, h, "farn", max_batch=MAX_BATCH) as eng:
        eng.next_segments([2, 2])  # two clips: pairs (0, 1) and (2, 3), none across the boundary
        fwd, bwd, occ_f, occ_b = eng.calc_optflows_bidir(frames, 1)
        plain = eng.calc_optflows_bidir(frames, 1)[0]  # the declaration applied to one call only
        none = eng.calc_optflows_bidir(frames[:1], 1)
    want_f = np.stack([_oracle_flow(oracle, "farn", (w, h), frames, a, b) for a, b in ((0, 1), (2, 3))])
    want_b = np.stack([_oracle_flow(oracle, "farn", (w, h), frames, b, a) for a, b in ((0, 1), (2, 3))])
    assert np.array_equal(fwd, want_f) and np.array_equal(bwd, want_b)
    assert np.array_equal(occ_f, R.fb_check_batch(want_f, want_b)[0]) and np.array_equal(occ_b, R.fb_check_batch(want_b, want_f)[0])
    assert plain.shape[0] == 3
    assert none[0].shape == (0, 2, h, w) and none[2].shape == (0, h, w)


def test_flow_tensor_bidir_into_strided_slices(dfx, oracle):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    w, h, step = 97, 61, 1
    frames = _frames(w, h)
    m = N - 1
    fwd_ref, bwd_ref, occ_f_ref, occ_b_ref = _reference(oracle, "tvl1", (w, h), frames, step)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as eng:
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        big = torch.full((2, m + 2, 3, h + 2, w + 5), -777.25, dtype=torch.float32, device="cuda")
        bigm = torch.full((2, m + 1, h + 3, w + 7), 0xA5, dtype=torch.uint8, device="cuda")
        out = (big[0, 1:m + 1, 1:3, 1:h + 1, 2:w + 2], big[1, 1:m + 1, 1:3, 1:h + 1, 2:w + 2],
               bigm[0, 1:m + 1, 2:h + 2, 3:w + 3], bigm[1, 1:m + 1, 2:h + 2, 3:w + 3])
        ret = eng.flow_tensor_bidir(d_frames, step, out=out)
        assert all(r is o for r, o in zip(ret, out))
        fresh = eng.flow_tensor_bidir(d_frames, step)
        unchecked = eng.flow_tensor_bidir(d_frames, step, check=False)
        with pytest.raises(ValueError):
            eng.flow_tensor_bidir(d_frames, step, out=(out[0], out[1][:, :, :, :w - 1], out[2], out[3]))
        with pytest.raises(ValueError):
            eng.flow_tensor_bidir(d_frames, step, out=(out[0], out[1].contiguous(), out[2], out[3]))  # unequal strides
        got = [t.cpu().numpy() for t in out]
        big_h, bigm_h = big.cpu().numpy(), bigm.cpu().numpy()
    for g, ref in zip(got, (fwd_ref, bwd_ref, occ_f_ref, occ_b_ref)):
        assert np.array_equal(g, ref)
    for t, ref in zip(fresh, (fwd_ref, bwd_ref, occ_f_ref, occ_b_ref)):
        assert t.is_contiguous() and np.array_equal(t.cpu().numpy(), ref)
    assert unchecked[2] is None and unchecked[3] is None and np.array_equal(unchecked[1].cpu().numpy(), bwd_ref)
    inside = np.zeros(big_h.shape, bool)
    inside[:, 1:m + 1, 1:3, 1:h + 1, 2:w + 2] = True
    assert np.all(big_h[~inside] == F32(-777.25)), "a float outside the slices was written"
    inside = np.zeros(bigm_h.shape, bool)
    inside[:, 1:m + 1, 2:h + 2, 3:w + 3] = True
    assert np.all(bigm_h[~inside] == 0xA5), "a mask byte outside the slices was written"


def test_refusals_leave_the_handle_usable(dfx, oracle):
    w, h, step = 97, 61, 1
    frames = _frames(w, h)
    m = N - 1
    fwd_ref, bwd_ref, occ_f_ref, _ = _reference(oracle, "farn", (w, h), frames, step)
    with dfx.FlowEngine(w, h, "farn", max_batch=MAX_BATCH) as eng:
        with DevBuf(eng, init=np.stack(frames)) as d_fr, DevBuf(eng, 4 * m * 2 * h * w) as d_f, \
                DevBuf(eng, 4 * m * 2 * h * w) as d_b, DevBuf(eng, m * h * w) as d_of, DevBuf(eng, m * h * w) as d_ob:
            good = dict(fr=d_fr.ptr(), pitch=w, fs=w * h, n=N, step=step, f=d_f.ptr(), b=d_b.ptr(), rp=w, ps=h * w,
                        fls=2 * h * w, a1=R.ALPHA1, a2=R.ALPHA2, of=d_of.ptr(), ob=d_ob.ptr(), op=w, os=h * w)

            def call(**kw):
                a = dict(good, **kw)
                eng.calc_optflows_bidir_device(a["fr"], a["pitch"], a["fs"], a["n"], a["step"], a["f"], a["b"], a["rp"], a["ps"],
                                               a["fls"], a["a1"], a["a2"], a["of"], a["ob"], a["op"], a["os"])

            refused = [dict(of=None), dict(ob=None), dict(step=0), dict(fr=None), dict(f=None), dict(b=None), dict(n=-1),
                       dict(pitch=w - 1), dict(fs=w * h - 1), dict(rp=w - 1), dict(ps=h * w - 1), dict(fls=2 * h * w - 1),
                       dict(op=w - 1), dict(os=h * w - 1), dict(a1=float("nan")), dict(a2=-1.0), dict(a2=float("inf"))]
            for kw in refused:
                with pytest.raises(dfx.DfxError) as e:
                    call(**kw)
                assert e.value.status == 1, kw
            # a dfx_next_segments_src declaration is for host-pointer calls: refused like the other device-resident forms,
            # and consumed
            eng.next_segments([2, 2], src_sizes=[(w, h), (w, h)])
            with pytest.raises(dfx.DfxError) as e:
                call()
            assert e.value.status == 4
            call()
            assert np.array_equal(d_f.get(F32).reshape(m, 2, h, w), fwd_ref)
            assert np.array_equal(d_b.get(F32).reshape(m, 2, h, w), bwd_ref)
            assert np.array_equal(d_of.get().reshape(m, h, w), occ_f_ref)
    with dfx.FlowEngine(w, h, "frames") as eng:
        with DevBuf(eng, init=np.stack(frames)) as d_fr, DevBuf(eng, 4 * m * 2 * h * w) as d_f:
            with pytest.raises(dfx.DfxError) as e:
                eng.calc_optflows_bidir_device(d_fr.ptr(), w, w * h, N, 1, d_f.ptr(), d_f.ptr(), w, h * w, 2 * h * w)
            assert e.value.status == 4
