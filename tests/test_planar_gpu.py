"""Planar float output (dfx_calc_batch_planar*, FlowEngine.calc_optflows_planar / flow_tensor): every engine's last
kernel writes a u and a v plane per flow — the (M, 2, H, W) layout of a tensor consumer — raw or clamped to +-bound and
divided by it.  Checked against the CPU oracle, against the handle's own interleaved output, through every writer path,
with padded and unaligned strides, and through the torch binding.  Shapes are the smallest at which a writer can go wrong:
an odd width (single-float tail), TVL1's smallest sizes, two pixels in a second 64-wide tile."""
import ctypes as C

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

SIZES = [(67, 35), (64, 16), (16, 16), (130, 50)]
N_FRAMES, MAX_BATCH = 8, 3  # 7 or 6 pairs in batches of 3: the ragged last device batch is crossed
ORACLE = {"tvl1": "tvl1_calc", "farn": "farneback_calc", "brox": "brox_calc"}
# max-abs against the oracle, as each algorithm's own GPU test has it for the interleaved output: tests/test_tvl1_gpu.py and
# tests/test_brox_gpu.py compare with max-abs 0 (np.array_equal); tests/test_farneback_gpu.py:13 has TOL = 1e-3
TOL = {"tvl1": 0.0, "brox": 0.0, "farn": 1e-3}
SENTINEL = -777.25

_frames_cache, _ref_cache = {}, {}


def _frames(w, h):
    if (w, h) not in _frames_cache:
        _frames_cache[(w, h)] = SynthClip(w, h, 7).frames(N_FRAMES)
    return _frames_cache[(w, h)]


def _pairs(n, step):
    return [((i, i + step) if step > 0 else (i - step, i)) for i in range(max(n - abs(step), 0))]


def _ref(oracle, algo, w, h, step, **farn):
    """The oracle's flows of the shared clip as one (M, 2, H, W) array, computed once per case and never changed."""
    key = (algo, w, h, step, tuple(sorted(farn.items())))
    if key not in _ref_cache:
        params = None
        if farn:
            params = oracle.farneback_default_params()
            for k, v in farn.items():
                setattr(params, k, v)
        fr = _frames(w, h)
        flows = [getattr(oracle, ORACLE[algo])(fr[a], fr[b], params) for a, b in _pairs(N_FRAMES, step)]
        ref = np.stack(flows).transpose(0, 3, 1, 2).copy()
        ref.setflags(write=False)
        _ref_cache[key] = ref
    return _ref_cache[key]


def _planes_of(flows):
    return np.stack(flows).transpose(0, 3, 1, 2)


def _max_abs(a, b):
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("step", [1, -2])
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_raw_planes_match_the_oracle_and_the_interleaved_output(dfx, oracle, algo, w, h, step):
    ref = _ref(oracle, algo, w, h, step)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        got = eng.calc_optflows_planar(_frames(w, h), step)
        inter = eng.calc_optflows(_frames(w, h), step)
    assert got.shape == ref.shape == (N_FRAMES - abs(step), 2, h, w) and got.dtype == np.float32
    err = _max_abs(got, ref)
    print(f"{algo} {w}x{h} step {step}: max-abs {err}")
    assert err <= TOL[algo]
    assert np.array_equal(got, _planes_of(inter)), "the planes are not the interleaved flow, de-interleaved"


def _variants():
    from denseflow_amd import engine as E

    return [
        ("tvl1", dict(impl=0), {}), ("tvl1", dict(impl=1), {}), ("tvl1", dict(impl=2), {}),
        ("tvl1", dict(variant=E.VAR_TVL1_NO_HEAD), {}),
        ("farn", {}, {}), ("farn", dict(variant=E.VAR_FARN_M_IN_HBM), {}), ("farn", dict(impl=1), {}),
        ("farn", dict(farn_win_size=9), dict(win_size=9)),   # the generic iteration kernel
        ("farn", dict(farn_num_iters=1), dict(num_iters=1)),  # a level of one iteration: the row stream ends in k_farn_merge_planar
        ("brox", {}, {}), ("brox", dict(variant=E.VAR_BROX_SOR_PER_TILE), {}),
    ]


@pytest.mark.parametrize("case", range(11))
@pytest.mark.parametrize("w,h", [(67, 35), (130, 50)])
def test_every_writer_path(dfx, oracle, w, h, case):
    algo, knobs, farn = _variants()[case]
    ref = _ref(oracle, algo, w, h, 1, **farn)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH, **knobs) as eng:
        got = eng.calc_optflows_planar(_frames(w, h), 1)
        inter = eng.calc_optflows(_frames(w, h), 1)
    err = _max_abs(got, ref)
    print(f"{algo} {knobs} {w}x{h}: max-abs {err}")
    assert err <= TOL[algo]
    assert np.array_equal(got, _planes_of(inter))


@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_padded_unaligned_strides_touch_nothing_outside_the_windows(dfx, algo):
    import torch

    w, h, step = 67, 35, 1
    frames = _frames(w, h)
    m = N_FRAMES - 1
    row_pitch = w + 3
    plane_stride = h * row_pitch + 5
    flow_stride = 2 * plane_stride + 7
    lead, tail = 3, 11  # floats in front of the first plane (the base is then not even 8-byte aligned) and behind the last flow
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        want = eng.calc_optflows_planar(frames, step)
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.full((lead + m * flow_stride + tail,), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        eng.calc_optflows_planar_device(d_frames.data_ptr(), w, w * h, N_FRAMES, step, None, buf.data_ptr() + 4 * lead,
                                        row_pitch, plane_stride, flow_stride)
        got = buf.cpu().numpy()
    inside = np.zeros(got.shape, bool)
    for i in range(m):
        for p in range(2):
            o = lead + i * flow_stride + p * plane_stride
            win = got[o:o + h * row_pitch].reshape(h, row_pitch)[:, :w]
            assert np.array_equal(win, want[i, p]), (i, p)
            inside[o:o + h * row_pitch].reshape(h, row_pitch)[:, :w] = True
    assert inside.sum() == m * 2 * h * w
    assert np.all(got[~inside] == SENTINEL), "a float outside the W x H windows was written"
    assert np.all(got[:lead] == SENTINEL) and np.all(got[-tail:] == SENTINEL)


@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_flow_tensor_into_a_strided_slice(dfx, algo):
    import torch

    w, h, step = 67, 35, 1
    frames = _frames(w, h)
    m = N_FRAMES - 1
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        want = eng.calc_optflows_planar(frames, step)
        big = torch.full((m + 2, 3, h + 2, w + 5), SENTINEL, dtype=torch.float32, device="cuda")
        out = big[1:m + 1, 1:3, 1:h + 1, 2:w + 2]
        ret = eng.flow_tensor(torch.from_numpy(np.stack(frames)).cuda(), step, out=out)
        assert ret is out
        got = big.cpu().numpy()
    assert np.array_equal(got[1:m + 1, 1:3, 1:h + 1, 2:w + 2], want)
    got[1:m + 1, 1:3, 1:h + 1, 2:w + 2] = SENTINEL
    assert np.all(got == SENTINEL), "flow_tensor wrote outside `out`"


@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_normalised_output_is_the_clamped_flow_over_the_bound(dfx, oracle, algo):
    import torch

    w, h, step, b = 130, 50, -2, 2.0
    ref = _ref(oracle, algo, w, h, step)
    assert (np.abs(ref) > b).any() and (np.abs(ref) < b).any(), "the clamp must bind in some pixels and not in others"
    want = np.clip(ref, -b, b).astype(np.float32) / np.float32(b)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        got = eng.calc_optflows_planar(_frames(w, h), step, bound=b)
        dev = eng.flow_tensor(torch.from_numpy(np.stack(_frames(w, h))).cuda(), step, bound=b).cpu().numpy()
    print(f"{algo}: max-abs {_max_abs(got, want)}, clamped {(np.abs(ref) > b).mean():.3f} of the values")
    assert np.abs(got).max() == 1.0
    assert _same_bits(got, want)
    assert _same_bits(dev, want)


def test_the_stored_value_nan_clamp_and_one_ieee_division(dfx):
    """dfx_planar_value (dfx_device.h), the function every planar writer stores through, on chosen operands
    (dfxi_probe_planar_value, selftest.hip): NaN -> 0, the clamp, a correctly rounded division also for bounds that are no
    power of two; bound 0 returns the operand's bits."""
    lib = dfx.load_library()
    fn = lib.dfxi_probe_planar_value
    fn.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    fn.restype = C.c_int
    rng = np.random.default_rng(5)
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 2.0, -2.0, 3.0, -3.0, 1e-40, -1e-40, 1.17549435e-38,
                        3.4e38, 0.3, 19.999999, 20.000002], np.float32)
    x = np.concatenate([special, (rng.standard_normal(4096) * 8).astype(np.float32)])
    for b in (2.0, 20.0, 3.0, 0.7, 0.0):
        bound = np.full(x.shape, b, np.float32)
        out = np.empty_like(x)
        assert fn(0, x.ctypes.data, bound.ctypes.data, out.ctypes.data, x.size) == 0
        if b == 0.0:
            keep = ~np.isnan(x)
            assert _same_bits(out[keep], x[keep]) and np.isnan(out[~keep]).all()
            continue
        with np.errstate(invalid="ignore"):
            want = np.clip(x, -np.float32(b), np.float32(b)).astype(np.float32) / np.float32(b)
        want[np.isnan(x)] = 0.0
        assert _same_bits(out, want), (b, np.flatnonzero(out.view(np.uint32) != want.view(np.uint32))[:8])


def test_flow_tensor_after_work_on_torchs_current_stream(dfx):
    """Frames produced on torch's current stream right before the call, no manual synchronisation; a view with padded
    rows and frames gives the same."""
    import torch

    w, h = 67, 35
    frames = _frames(w, h)
    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as eng:
        want = eng.calc_optflows_planar(frames, 1)
        base = torch.from_numpy(np.stack(frames)).cuda()
        big = torch.zeros((N_FRAMES, h + 3, w + 9), dtype=torch.uint8, device="cuda")
        made = (base.to(torch.int32) * 3 - base.to(torch.int32) * 2).to(torch.uint8)  # kernels on the current stream
        got = eng.flow_tensor(made, 1)
        big[:, 2:h + 2, 4:w + 4] = made
        view = eng.flow_tensor(big[:, 2:h + 2, 4:w + 4], 1)
        assert got.shape == (N_FRAMES - 1, 2, h, w) and got.dtype == torch.float32 and got.is_cuda and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(view.cpu().numpy(), want)


def test_flow_tensor_bgr_source_segments_and_set_size(dfx):
    import torch

    w, h = 67, 35
    ws, hs = 80, 44
    rng = np.random.default_rng(11)
    gray = SynthClip(ws, hs, 9).frames(N_FRAMES)
    bgr = [np.stack([g, np.roll(g, 1, 1), 255 - g], -1) + rng.integers(0, 2, (hs, ws, 3), dtype=np.uint8) for g in gray]
    with dfx.FlowEngine(130, 50, "tvl1", max_batch=MAX_BATCH) as eng:
        first = eng.flow_tensor(torch.from_numpy(np.stack(_frames(130, 50))).cuda(), 1)
        assert first.shape == (N_FRAMES - 1, 2, 50, 130)
        eng.set_size(w, h)  # afterwards: what a fresh handle of that size gives
        d_frames = torch.from_numpy(np.stack(_frames(w, h))).cuda()
        resized = eng.flow_tensor(d_frames, 1).cpu().numpy()
        eng.next_segments([3, 5])  # two clips: 2 + 4 flows, none across the boundary
        joined = eng.flow_tensor(d_frames, 1).cpu().numpy()
        plain = eng.flow_tensor(d_frames, 1).cpu().numpy()  # the declaration applied to one call only
        eng.set_source_format(ws, hs, 3)
        colour = eng.flow_tensor(torch.from_numpy(np.stack(bgr)).cuda(), 1).cpu().numpy()
        with pytest.raises(ValueError):
            eng.flow_tensor(d_frames, 1)  # gray W x H frames no longer match the source format
    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as fresh:
        want = fresh.calc_optflows_planar(_frames(w, h), 1)
        clip_a = fresh.calc_optflows_planar(_frames(w, h)[:3], 1)
        clip_b = fresh.calc_optflows_planar(_frames(w, h)[3:], 1)
        fresh.set_source_format(ws, hs, 3)
        want_colour = fresh.calc_optflows_planar(bgr, 1)
    assert np.array_equal(resized, want) and np.array_equal(plain, want)
    assert joined.shape[0] == 6 and np.array_equal(joined, np.concatenate([clip_a, clip_b]))
    assert np.array_equal(colour, want_colour)


def test_refusals_leave_the_error_text(dfx):
    import torch

    w, h = 67, 35
    frames = _frames(w, h)

    def last_error(eng):
        return eng._L.dfx_last_error(eng._h).decode()

    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as eng:
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.full((N_FRAMES * 2 * h * (w + 4) + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rp, ps = w + 1, h * (w + 1)
        for strides in [(w - 1, ps, 2 * ps), (rp, ps - 1, 2 * ps), (rp, ps, 2 * ps - 1)]:
            with pytest.raises(dfx.DfxError) as e:
                eng.calc_optflows_planar_device(d_frames.data_ptr(), w, w * h, N_FRAMES, 1, None, buf.data_ptr(), *strides)
            assert e.value.status == 1 and "row_pitch_floats" in last_error(eng), strides
        for bound in (-1.0, float("inf"), float("nan")):
            eng.calc_optflows_planar(frames[:2], 1)  # a success in between: the text below is this refusal's
            with pytest.raises(dfx.DfxError) as e:
                eng.calc_optflows_planar(frames, 1, bound=bound)
            assert e.value.status == 1 and "norm_bound" in last_error(eng), bound
            with pytest.raises(dfx.DfxError) as e:
                eng.flow_tensor(d_frames, 1, bound=bound)
            assert e.value.status == 1 and "norm_bound" in last_error(eng), bound
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all()), "a refused call wrote"
    with dfx.FlowEngine(w, h, "frames") as eng:
        with pytest.raises(dfx.DfxError) as e:
            eng.calc_optflows_planar(frames, 1)
        assert e.value.status == 4 and "DFX_ALGO_FRAMES" in last_error(eng)
