"""Every way results leave the device gives the same bytes: the blocking dense-pitch calls of the Python binding are the
expectation, and the raw ABI must reproduce them (a) in the submit form with two FlowBuffers in flight and (b) with padded
destination rows and padded frame rows, blocking and submitted — for float flows, bounded planes, PNG planes + bounds and
JPEG files, at one frame size per copy regime of the FlowBuffer driver (denseflow_amd/csrc/dfx_pipeline.cpp):
    96 x 64    frames and results both go through the page-locked bounce buffers,
    224 x 224  frames bounce; a float flow (401 KB) goes by a direct copy, the u8 planes bounce,
    640 x 480  neither direction bounces.
Seven frames at max_batch = 2 are three full batches and a ragged one: both staging parities are reused, and the last
batch of a submitted FlowBuffer finishes on a deferred tail."""
import ctypes as C

import numpy as np
import pytest

from denseflow_amd.synth import SynthClip

pytestmark = pytest.mark.gpu

N, M, BOUND, PAD, FRAME_PAD, SENTINEL = 7, 6, 20.0, 24, 8, 0xA5


def _ptrs(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


class _Planes:
    """M destinations of h rows, `row` bytes each at a pitch of row + pad, filled with the sentinel."""

    def __init__(self, h, row, pad):
        self.row, self.pitch = row, row + pad
        self.buf = [np.full((h, self.pitch), SENTINEL, np.uint8) for _ in range(M)]
        self.ptrs = _ptrs(self.buf)

    def check(self, want, what):
        for i in range(M):
            assert np.array_equal(self.buf[i][:, :self.row], np.ascontiguousarray(want[i]).view(np.uint8).reshape(len(self.buf[i]), -1)), \
                (what, i)
            assert np.all(self.buf[i][:, self.row:] == SENTINEL), (what, i, "padding bytes were written")


class _Call:
    """One FlowBuffer through one raw entry point: destinations, the call, and the comparison with the expectation."""

    def __init__(self, L, eng, kind, frames, w, h, pad):
        self.L, self.eng, self.kind, self.w, self.h = L, eng, kind, w, h
        self.fp, self.fpitch = _ptrs(frames), frames[0].strides[0]
        self.ticket = C.c_uint64(0)
        if kind == "float":
            self.a = _Planes(h, w * 8, pad)
        elif kind in ("u8", "png"):
            self.a, self.b = _Planes(h, w, pad), _Planes(h, w, pad)
            self.bounds = np.full((M, 2), -1.0, np.float64)
        else:
            self.cap = int(L.dfx_jpeg_capacity(eng._h))
            self.jx = [np.full(self.cap, SENTINEL, np.uint8) for _ in range(M)]
            self.jy = [np.full(self.cap, SENTINEL, np.uint8) for _ in range(M)]
            self.px, self.py = _ptrs(self.jx), _ptrs(self.jy)
            self.sx, self.sy = (C.c_uint32 * M)(), (C.c_uint32 * M)()

    def issue(self, submit):
        L, h, t = self.L, self.eng._h, ([C.byref(self.ticket)] if submit else [])
        head = (h, self.fp, self.fpitch, N, 1)
        if self.kind == "float":
            rc = (L.dfx_submit_batch if submit else L.dfx_calc_batch)(*head, self.a.ptrs, self.a.pitch, *t)
        elif self.kind == "u8":
            rc = (L.dfx_submit_batch_u8 if submit else L.dfx_calc_batch_u8)(*head, -BOUND, BOUND, self.a.ptrs, self.b.ptrs,
                                                                            self.a.pitch, *t)
        elif self.kind == "png":
            rc = (L.dfx_submit_batch_png if submit else L.dfx_calc_batch_png)(
                *head, self.a.ptrs, self.b.ptrs, self.a.pitch, self.bounds.ctypes.data_as(C.POINTER(C.c_double)), *t)
        else:
            rc = (L.dfx_submit_batch_jpeg if submit else L.dfx_calc_batch_jpeg)(*head, -BOUND, BOUND, 95, self.px, self.py,
                                                                               self.cap, self.sx, self.sy, *t)
        assert rc == 0, (self.kind, submit, L.dfx_last_error(h))
        assert not submit or self.ticket.value != 0

    def check(self, want, what):
        what = (self.kind, what)
        if self.kind == "float":
            self.a.check(want["float"], what)
        elif self.kind == "u8":
            self.a.check(want["u8"][0], what)
            self.b.check(want["u8"][1], what)
        elif self.kind == "png":
            self.a.check(want["png"][0], what)
            self.b.check(want["png"][1], what)
            assert np.array_equal(self.bounds, want["png"][2]), what
        else:
            for files, bufs, sizes in ((want["jpeg"][0], self.jx, self.sx), (want["jpeg"][1], self.jy, self.sy)):
                for i in range(M):
                    assert sizes[i] == len(files[i]), what
                    assert bufs[i][:sizes[i]].tobytes() == files[i], what
                    assert np.all(bufs[i][sizes[i]:] == SENTINEL), what


@pytest.mark.parametrize("w,h", [(96, 64), (224, 224), (640, 480)])
def test_every_output_path_gives_the_blocking_dense_result(dfx, w, h):
    L = dfx.load_library()
    frames = [np.ascontiguousarray(f) for f in SynthClip(w, h, 5).frames(N)]
    padded = np.full((N, h, w + FRAME_PAD), SENTINEL, np.uint8)  # the same frames at a row pitch of W + 8
    padded[:, :, :w] = np.stack(frames)
    with dfx.FlowEngine(w, h, "farn", max_batch=2) as eng:
        want = {"float": eng.calc_optflows(frames, 1), "u8": eng.calc_optflows_u8(frames, 1, BOUND),
                "png": eng.calc_optflows_png(frames, 1), "jpeg": eng.calc_optflows_jpeg(frames, 1, BOUND)}
        assert len(want["float"]) == M and want["float"][0].shape == (h, w, 2)
        for kind in ("float", "u8", "png", "jpeg"):
            # (a) the submit form: the second FlowBuffer is issued while the first one's tail is still pending
            calls = [_Call(L, eng, kind, frames, w, h, 0) for _ in range(2)]
            for c in calls:
                c.issue(submit=True)
            for c in calls:
                assert L.dfx_wait(eng._h, c.ticket.value) == 0, L.dfx_last_error(eng._h)
                c.check(want, "submit, two in flight")
            # (b) destination rows of row + 24 bytes and frame rows of W + 8 bytes, blocking and submitted
            for submit in (False, True):
                c = _Call(L, eng, kind, list(padded), w, h, PAD)
                c.issue(submit)
                assert L.dfx_wait(eng._h, c.ticket.value if submit else 0) == 0, L.dfx_last_error(eng._h)
                c.check(want, "padded rows, submit" if submit else "padded rows, blocking")
