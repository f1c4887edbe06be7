"""dfx_next_segments_src: clips of different SOURCE sizes joined into one call give, bit for bit, what each clip gives on
its own under dfx_set_source_format.  Target 32 x 24; the three sources take the three paths of the preparation kernel:
32 x 24 (copy), 64 x 48 (exact 2x decimation) and 33 x 47 (linear).  Clips of 4, 3 and 1 frames: the 1-frame clip yields
no pair, and at step 2 the 3-frame clip yields one.  Rows are padded (every clip its own pitch)."""
import ctypes as C

import numpy as np
import pytest

import denseflow_amd
from denseflow_amd import engine as E
from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

W, H = 32, 24
SRC = [(32, 24), (64, 48), (33, 47)]
SEG = [4, 3, 1]
PAD = [5, 0, 31]  # bytes of row padding per clip
BATCH = 3  # six pairs at step 1: two device batches, the first one spans two clips


def _padded(frame, pad):
    """The frame as a view with `pad` more bytes per row (filled with a value no frame row may pick up)."""
    rows = frame.reshape(frame.shape[0], -1)
    buf = np.full((rows.shape[0], rows.shape[1] + pad), 0xA5, np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf[:, :rows.shape[1]].reshape(frame.shape)


def _clips(channels, src=SRC, seg=SEG, pad=PAD):
    clips = []
    for k, ((w, h), n, p) in enumerate(zip(src, seg, pad)):
        fr = SynthClip(w, h, 20 + k).frames(n + 2)
        if channels == 3:
            fr = [np.ascontiguousarray(np.stack([fr[i], fr[i + 1], fr[i + 2]], -1)) for i in range(n)]
        clips.append([_padded(f, p) for f in fr[:n]])
    return clips


def _per_clip(eng, clips, src, channels, step, call):
    out = []
    for (w, h), clip in zip(src, clips):
        eng.set_source_format(w, h, channels)
        out.append(call(eng, [np.ascontiguousarray(f) for f in clip], step))
    eng.set_source_format()
    return out


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("step", [1, 2])
def test_tvl1_three_clips_joined_equal_the_clips_on_their_own(channels, step):
    clips = _clips(channels)
    with denseflow_amd.FlowEngine(W, H, "tvl1", max_batch=BATCH) as eng:
        want = [f for fl in _per_clip(eng, clips, SRC, channels, step, lambda e, fr, s: e.calc_optflows(fr, s)) for f in fl]
        eng.next_segments(SEG, src_sizes=SRC, channels=channels)
        got = eng.calc_optflows([f for c in clips for f in c], step)
        eng.next_segments(SEG, src_sizes=SRC, channels=channels)
        ticket, sub = eng.submit_optflows([f for c in clips for f in c], step)
        eng.wait(ticket)
    assert len(want) == sum(max(n - step, 0) for n in SEG) == (5 if step == 1 else 3)
    assert len(got) == len(sub) == len(want)
    for i, (a, b, c) in enumerate(zip(got, sub, want)):
        assert a.shape == (H, W, 2) and np.array_equal(a, c) and np.array_equal(b, c), (channels, step, i)


@pytest.mark.parametrize("algo", ["farn", "brox"])
def test_one_linear_and_one_copy_clip(algo):
    src, seg, pad = [(33, 47), (32, 24)], [3, 3], [31, 5]
    clips = _clips(1, src, seg, pad)
    with denseflow_amd.FlowEngine(W, H, algo, max_batch=BATCH) as eng:
        want = [f for fl in _per_clip(eng, clips, src, 1, 1, lambda e, fr, s: e.calc_optflows(fr, s)) for f in fl]
        eng.next_segments(seg, src_sizes=src)
        got = eng.calc_optflows([f for c in clips for f in c], 1)
    assert len(got) == len(want) == 4
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_jpeg_files_of_joined_clips():
    clips = _clips(1)
    with denseflow_amd.FlowEngine(W, H, "tvl1", max_batch=BATCH) as eng:
        per = _per_clip(eng, clips, SRC, 1, 1, lambda e, fr, s: e.calc_optflows_jpeg(fr, s, 20))
        eng.next_segments(SEG, src_sizes=SRC)
        gx, gy = eng.calc_optflows_jpeg([f for c in clips for f in c], 1, 20)
    wx = [b for x, _ in per for b in x]
    wy = [b for _, y in per for b in y]
    assert len(gx) == 5 and gx == wx and gy == wy and all(len(b) > 0 for b in gx + gy)


def test_declaration_is_consumed_by_exactly_one_call():
    clips = _clips(1)
    flat = [f for c in clips for f in c]
    with denseflow_amd.FlowEngine(W, H, "farn", max_batch=BATCH) as eng:
        eng.next_segments(SEG, src_sizes=SRC)
        assert len(eng.calc_optflows(flat, 1)) == 5
        # the next call is an ordinary one again: W x H gray frames, one clip, and the handle's own pitch check
        plain = [np.ascontiguousarray(f) for f in clips[0]]
        assert len(eng.calc_optflows(plain, 1)) == 3
        L, h = eng._L, eng._h
        fp = (C.c_void_p * len(flat))(*[f.ctypes.data for f in flat])
        out = [np.empty((H, W, 2), np.float32) for _ in range(7)]
        op = (C.c_void_p * 7)(*[o.ctypes.data for o in out])
        rc = L.dfx_calc_batch(h, fp, 1, len(flat), 1, op, W * 8)  # pitch 1: refused without a pending declaration
        assert rc == E.ERR_INVALID
        # a declaration whose call is refused is gone as well
        eng.next_segments(SEG, src_sizes=SRC)
        eng._num_pairs(len(flat), 1), eng._check_shapes(flat), eng._arm()
        assert L.dfx_calc_batch(h, fp, 1, len(flat), 0, op, W * 8) == E.ERR_INVALID  # step 0
        assert L.dfx_calc_batch(h, fp, 1, len(flat), 1, op, W * 8) == E.ERR_INVALID  # pitch 1 counts again
        # bad declarations
        seg = (C.c_int * 1)(2)
        assert L.dfx_next_segments_src(h, seg, (C.c_int * 2)(33, 47), (C.c_size_t * 1)(32), 1, 1) == E.ERR_INVALID
        assert L.dfx_next_segments_src(h, seg, (C.c_int * 2)(33, 47), (C.c_size_t * 1)(33), 1, 2) == E.ERR_INVALID
        assert L.dfx_next_segments_src(h, seg, (C.c_int * 2)(0, 47), (C.c_size_t * 1)(33), 1, 1) == E.ERR_INVALID


def test_device_form_refuses_a_pending_declaration():
    with denseflow_amd.FlowEngine(W, H, "farn", max_batch=BATCH) as eng:
        L, h = eng._L, eng._h
        d_in, d_out = C.c_void_p(), C.c_void_p()
        assert L.dfx_device_malloc(h, C.byref(d_in), 2 * W * H) == E.OK
        assert L.dfx_device_malloc(h, C.byref(d_out), W * H * 8) == E.OK
        try:
            fr = SynthClip(W, H, 5).frames(2)
            assert L.dfx_memcpy_h2d(h, d_in, np.stack(fr).ctypes.data, 2 * W * H) == E.OK
            seg, wh, pitch = (C.c_int * 1)(2), (C.c_int * 2)(64, 48), (C.c_size_t * 1)(64)
            assert L.dfx_next_segments_src(h, seg, wh, pitch, 1, 1) == E.OK
            assert L.dfx_calc_batch_device(h, d_in, W, W * H, 2, 1, d_out, W * H * 2) == E.ERR_UNSUPPORTED
            # consumed by the refusal: the same call now runs, as one clip of the handle's own format
            assert L.dfx_calc_batch_device(h, d_in, W, W * H, 2, 1, d_out, W * H * 2) == E.OK
            got = np.empty((H, W, 2), np.float32)
            assert L.dfx_memcpy_d2h(h, got.ctypes.data, d_out, W * H * 8) == E.OK
            assert np.array_equal(got, eng.calc(fr[0], fr[1]))
        finally:
            L.dfx_device_free(h, d_in), L.dfx_device_free(h, d_out)
