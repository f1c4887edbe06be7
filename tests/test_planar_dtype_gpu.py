"""Typed planar output (dfx_calc_batch_planar_as*, dtype= of calc_optflows_planar / calc_optflows_planar_device /
flow_tensor): float16 and bfloat16 planes are the float32 value of the float32 twin, converted once, round to nearest
even, in the store that writes the plane.  Everything here is bit for bit against tests/reduced_ref.py applied to the SAME
handle's float32 planar output — no oracle tolerance enters.  The clip and the sizes are those of tests/test_planar_gpu.py:
an odd width (single-element tails), two pixels in a second 64-wide tile, and a contiguous 64 x 16 case on which the widest
(8-byte) store runs."""
import ctypes as C

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests import reduced_ref as R

pytestmark = pytest.mark.gpu

N_FRAMES, MAX_BATCH = 8, 3  # 7 or 6 pairs in batches of 3: the ragged last device batch is crossed
DTYPES = ["float16", "bfloat16"]
SENT = 0x5A5A  # the 16-bit pattern the buffers of the stride tests are filled with

_frames_cache = {}


def _frames(w, h):
    if (w, h) not in _frames_cache:
        _frames_cache[(w, h)] = SynthClip(w, h, 7).frames(N_FRAMES)
    return _frames_cache[(w, h)]


def _np_dtype(dtype):
    return np.float16 if dtype == "float16" else "bfloat16"


def _torch_dtype(dtype):
    import torch

    return torch.float16 if dtype == "float16" else torch.bfloat16


def _bits(a):
    """uint16 bit patterns of a float16 / uint16 numpy array or a half torch tensor."""
    import torch

    if isinstance(a, torch.Tensor):
        return a.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return np.ascontiguousarray(a).view(np.uint16)


def _same(got, want, dtype):
    """Bit-identical, a NaN standing for any NaN (its payload is unspecified)."""
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    if got.shape != want.shape:
        return False
    gn, wn = R.is_nan_bits(got, dtype), R.is_nan_bits(want, dtype)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn]))


def _variants():
    from denseflow_amd import engine as E

    return [
        ("tvl1", dict(impl=0)), ("tvl1", dict(impl=1)), ("tvl1", dict(impl=2)),
        ("tvl1", dict(variant=E.VAR_TVL1_NO_HEAD)),
        ("farn", {}), ("farn", dict(variant=E.VAR_FARN_M_IN_HBM)), ("farn", dict(impl=1)),
        ("farn", dict(farn_win_size=9)),   # the generic iteration kernel
        ("farn", dict(farn_num_iters=1)),  # a level of one iteration: the row stream ends in k_farn_merge_planar
        ("brox", {}), ("brox", dict(variant=E.VAR_BROX_SOR_PER_TILE)),
        ("tvl1", dict(tvl1_gamma=2.0)),    # the fused gamma tile kernel
        ("farn", dict(farn_window=1)),     # the Gaussian update window
    ]


def _probe_fns(dfx):
    lib = dfx.load_library()
    f32 = lib.dfxi_probe_planar_value
    f32.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    f32.restype = C.c_int
    return f32, lib.dfxi_probe_planar_value_as


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_stored_bits_on_chosen_operands(dfx, dtype):
    """dfxi_probe_planar_value_as stores through dfx_planar_store4, the function the writers use: its 16 bits are the
    restatement of what dfxi_probe_planar_value gives in float32, for every bound."""
    f32, typed = _probe_fns(dfx)
    rng = np.random.default_rng(5)
    x = np.concatenate([R.special_values(), np.array([np.nan, -np.nan, np.inf, -np.inf], np.float32),
                        (rng.standard_normal(4096) * 8).astype(np.float32)])
    if x.size % 4 == 0:  # the last lane holds fewer than 4 values
        x = x[:-1].copy()
    code = 1 if dtype == "float16" else 2  # DFX_PLANAR_F16 / DFX_PLANAR_BF16
    for b in (0.0, 2.0, 20.0, 3.0, 0.7):
        bound = np.full(x.shape, b, np.float32)
        y = np.empty_like(x)
        assert f32(0, x.ctypes.data, bound.ctypes.data, y.ctypes.data, x.size) == 0
        got = np.full(x.shape, SENT, np.uint16)
        assert typed(0, code, x.ctypes.data, b, got.ctypes.data, x.size) == 0
        want = R.reduce_bits(y, dtype)
        nan = np.isnan(y)
        assert nan.any() == (b == 0.0)  # the bounded mode maps NaN to 0 before the conversion
        assert R.is_nan_bits(got[nan], dtype).all()
        bad = np.flatnonzero(got[~nan] != want[~nan])
        assert bad.size == 0, (dtype, b, y[~nan][bad[:8]], got[~nan][bad[:8]], want[~nan][bad[:8]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(13))
@pytest.mark.parametrize("w,h", [(67, 35), (130, 50)])
def test_every_writer_path(dfx, w, h, case, dtype):
    algo, knobs = _variants()[case]
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH, **knobs) as eng:
        f32 = eng.calc_optflows_planar(_frames(w, h), 1)
        got = eng.calc_optflows_planar(_frames(w, h), 1, dtype=_np_dtype(dtype))
    assert got.shape == f32.shape == (N_FRAMES - 1, 2, h, w) and got.dtype.itemsize == 2
    assert np.abs(f32).max() > 0.1, "a flow of zeros checks nothing"
    assert _same(_bits(got), R.reduce_bits(f32, dtype), dtype), (algo, knobs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_strides_touch_nothing_outside_the_windows(dfx, algo, aligned, dtype):
    import torch

    step = 1
    m = N_FRAMES - 1
    if aligned:  # contiguous planes at a 256-byte aligned base: every lane's 4 pixels leave in one 8-byte store
        w, h, lead, tail = 64, 16, 0, 0
        row_pitch, plane_stride = w, h * w
        flow_stride = 2 * plane_stride
    else:  # 16-bit elements: the base is only 2-byte aligned, every stride odd
        w, h, lead, tail = 67, 35, 3, 11
        row_pitch = w + 3
        plane_stride = h * row_pitch + 5
        flow_stride = 2 * plane_stride + 7
    frames = _frames(w, h)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        want = R.reduce_bits(eng.calc_optflows_planar(frames, step), dtype)
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.full((lead + m * flow_stride + tail,), SENT, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        eng.calc_optflows_planar_device(d_frames.data_ptr(), w, w * h, N_FRAMES, step, None, buf.data_ptr() + 2 * lead,
                                        row_pitch, plane_stride, flow_stride, dtype=_np_dtype(dtype))
        got = buf.cpu().numpy().view(np.uint16)
    inside = np.zeros(got.shape, bool)
    for i in range(m):
        for p in range(2):
            o = lead + i * flow_stride + p * plane_stride
            win = got[o:o + h * row_pitch].reshape(h, row_pitch)[:, :w]
            assert _same(win, want[i, p], dtype), (i, p)
            inside[o:o + h * row_pitch].reshape(h, row_pitch)[:, :w] = True
    assert inside.sum() == m * 2 * h * w
    assert np.all(got[~inside] == SENT), "an element outside the W x H windows was written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_bounded_output(dfx, algo, dtype):
    import torch

    w, h, step, b = 130, 50, -2, 2.0
    frames = _frames(w, h)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        f32 = eng.calc_optflows_planar(frames, step, bound=b)
        got = eng.calc_optflows_planar(frames, step, bound=b, dtype=_np_dtype(dtype))
        dev = eng.flow_tensor(torch.from_numpy(np.stack(frames)).cuda(), step, bound=b, dtype=_torch_dtype(dtype))
        as_float = dev.float().abs().max().item()
    assert np.abs(f32).max() == 1.0 and (np.abs(f32) < 1.0).any()
    want = R.reduce_bits(f32, dtype)
    assert _same(_bits(got), want, dtype)
    assert _same(_bits(dev), want, dtype)
    assert as_float == 1.0


@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_host_and_device_forms_and_the_float32_typed_entry(dfx, algo):
    import torch

    w, h, step = 67, 35, -2
    frames = _frames(w, h)
    m = N_FRAMES - 2  # 6 flows in batches of 3 — and 7 below: the ragged last batch
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        f32 = eng.calc_optflows_planar(frames, step)
        f32_1 = eng.calc_optflows_planar(frames, 1)
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        eng.flow_tensor(d_frames, step)
        held = eng.device_bytes()
        # DFX_PLANAR_F32 through the typed entries: the float32 twin, bit for bit
        out = np.full((m, 2, h, w), np.float32(-777.25))
        up = (C.c_void_p * m)(*[out[k, 0].ctypes.data for k in range(m)])
        vp = (C.c_void_p * m)(*[out[k, 1].ctypes.data for k in range(m)])
        fr = [np.ascontiguousarray(f) for f in frames]
        fp = (C.c_void_p * N_FRAMES)(*[f.ctypes.data for f in fr])
        assert eng._L.dfx_calc_batch_planar_as(eng._h, fp, w, N_FRAMES, step, 0.0, 0, up, vp, w * 4) == 0
        assert np.array_equal(out.view(np.uint32), f32.view(np.uint32))
        d_out = torch.empty((m, 2, h, w), dtype=torch.float32, device="cuda")
        eng.calc_optflows_planar_device(d_frames.data_ptr(), w, w * h, N_FRAMES, step, None, d_out.data_ptr(), w, w * h,
                                        2 * w * h, dtype=np.float32)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), f32.view(np.uint32))
        for dtype in DTYPES:
            host = eng.calc_optflows_planar(frames, step, dtype=_np_dtype(dtype))
            host_1 = eng.calc_optflows_planar(frames, 1, dtype=_np_dtype(dtype))
            dev = eng.flow_tensor(d_frames, step, dtype=_torch_dtype(dtype))
            assert _same(_bits(host), R.reduce_bits(f32, dtype), dtype)
            assert _same(_bits(host_1), R.reduce_bits(f32_1, dtype), dtype)
            assert _same(_bits(dev), _bits(host), dtype)
        assert eng.device_bytes() == held, "a typed call allocated device memory a float32 planar call had not"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_flow_tensor_into_a_strided_slice(dfx, algo, dtype):
    import torch

    w, h, step = 67, 35, 1
    frames = _frames(w, h)
    m = N_FRAMES - 1
    tdt = _torch_dtype(dtype)
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        want = R.reduce_bits(eng.calc_optflows_planar(frames, step), dtype)
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        big = torch.full((m + 2, 3, h + 2, w + 5), SENT, dtype=torch.int16, device="cuda").view(tdt)
        out = big[1:m + 1, 1:3, 1:h + 1, 2:w + 2]
        ret = eng.flow_tensor(d_frames, step, out=out, dtype=tdt)
        assert ret is out
        fresh = eng.flow_tensor(d_frames, step, dtype=tdt)
        assert fresh.is_cuda and fresh.dtype == tdt and fresh.is_contiguous() and tuple(fresh.shape) == (m, 2, h, w)
        got = _bits(big)
        assert _same(_bits(fresh), want, dtype)
    assert _same(got[1:m + 1, 1:3, 1:h + 1, 2:w + 2], want, dtype)
    got[1:m + 1, 1:3, 1:h + 1, 2:w + 2] = SENT
    assert np.all(got == SENT), "flow_tensor wrote outside `out`"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["tvl1", "farn", "brox"])
def test_seeded(dfx, algo, dtype):
    import torch

    w, h, step = 67, 35, 1
    frames = _frames(w, h)
    m = N_FRAMES - 1
    tdt = _torch_dtype(dtype)
    rng = np.random.default_rng(17)
    seed = torch.from_numpy((rng.standard_normal((m, 2, h, w)) * 1.5).astype(np.float32)).cuda()
    with dfx.FlowEngine(w, h, algo, max_batch=MAX_BATCH) as eng:
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        out = torch.zeros((m, 2, h, w), dtype=tdt, device="cuda")
        if algo == "brox":
            with pytest.raises(dfx.DfxError) as e:
                eng.flow_tensor(d_frames, step, init=seed, out=out, dtype=tdt)
            assert e.value.status == 4 and "initial flow" in eng._L.dfx_last_error(eng._h).decode()
            return
        f32 = eng.flow_tensor(d_frames, step, init=seed).cpu().numpy()
        plain = eng.flow_tensor(d_frames, step).cpu().numpy()
        # a seed that is a non-contiguous view: made contiguous by the binding, read with its own strides by the library
        wide = torch.zeros((m, 2, h, w + 3), dtype=torch.float32, device="cuda")
        wide[..., :w] = seed
        eng.flow_tensor(d_frames, step, init=wide[..., :w], out=out, dtype=tdt)
        got = _bits(out)
    assert not np.array_equal(f32, plain), "the seed changed nothing: the case checks nothing"
    assert _same(got, R.reduce_bits(f32, dtype), dtype)


def test_seed_strides_of_their_own(dfx):
    """The C entry: a padded float32 seed and a differently padded half output in one call."""
    import torch

    w, h, step = 67, 35, 1
    frames = _frames(w, h)
    m = N_FRAMES - 1
    rng = np.random.default_rng(18)
    seed = (rng.standard_normal((m, 2, h, w)) * 1.5).astype(np.float32)
    with dfx.FlowEngine(w, h, "farn", max_batch=MAX_BATCH) as eng:
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        f32 = eng.flow_tensor(d_frames, step, init=torch.from_numpy(seed).cuda()).cpu().numpy()
        padded = torch.zeros((m, 2, h + 1, w + 3), dtype=torch.float32, device="cuda")
        padded[:, :, :h, :w] = torch.from_numpy(seed).cuda()
        out = torch.full((m, 2, h, w + 1), SENT, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        rc = eng._L.dfx_calc_batch_planar_as_init_device(
            eng._h, d_frames.data_ptr(), w, w * h, N_FRAMES, step, 0.0, 1, padded.data_ptr(), w + 3, (h + 1) * (w + 3),
            2 * (h + 1) * (w + 3), out.data_ptr(), w + 1, h * (w + 1), 2 * h * (w + 1))
        assert rc == 0, eng._L.dfx_last_error(eng._h).decode()
        got = out.cpu().numpy().view(np.uint16)
    assert _same(got[..., :w], R.reduce_bits(f32, "float16"), "float16")
    assert np.all(got[..., w:] == SENT)


def test_refusals_leave_the_error_text(dfx):
    import torch

    w, h = 67, 35
    frames = _frames(w, h)

    def last_error(eng):
        return eng._L.dfx_last_error(eng._h).decode()

    with dfx.FlowEngine(w, h, "tvl1", max_batch=MAX_BATCH) as eng:
        d_frames = torch.from_numpy(np.stack(frames)).cuda()
        buf = torch.full((N_FRAMES * 2 * h * (w + 4) + 64,), SENT, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        rp, ps = w + 1, h * (w + 1)
        for strides in [(w - 1, ps, 2 * ps), (rp, ps - 1, 2 * ps), (rp, ps, 2 * ps - 1)]:
            with pytest.raises(dfx.DfxError) as e:
                eng.calc_optflows_planar_device(d_frames.data_ptr(), w, w * h, N_FRAMES, 1, None, buf.data_ptr(), *strides,
                                                dtype=np.float16)
            assert e.value.status == 1 and "row_pitch" in last_error(eng), strides
        for bad in (3, -1):
            eng.calc_optflows_planar(frames[:2], 1)  # a success in between: the text below is this refusal's
            rc = eng._L.dfx_calc_batch_planar_as_device(eng._h, d_frames.data_ptr(), w, w * h, N_FRAMES, 1, 0.0, bad,
                                                        buf.data_ptr(), rp, ps, 2 * ps)
            assert rc == 1 and "dtype" in last_error(eng), bad
            rc = eng._L.dfx_calc_batch_planar_as_init_device(eng._h, d_frames.data_ptr(), w, w * h, N_FRAMES, 1, 0.0, bad,
                                                             buf.data_ptr(), rp, ps, 2 * ps, buf.data_ptr(), rp, ps, 2 * ps)
            assert rc == 1 and "dtype" in last_error(eng), bad
        with pytest.raises(dfx.DfxError) as e:
            eng.calc_optflows_planar(frames, 1, bound=-1.0, dtype=np.float16)
        assert e.value.status == 1 and "norm_bound" in last_error(eng)
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), "a refused call wrote"
    with dfx.FlowEngine(w, h, "frames") as eng:
        with pytest.raises(dfx.DfxError) as e:
            eng.calc_optflows_planar(frames, 1, dtype=np.float16)
        assert e.value.status == 4 and "DFX_ALGO_FRAMES" in last_error(eng)
