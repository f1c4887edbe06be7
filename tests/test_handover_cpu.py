"""CPU test of the hand-over of a device batch to the caller's buffers (denseflow_amd/csrc/dfx_handover.h, the header
the FlowBuffer driver, colour frame extraction and dfx_encode_jpeg compile): rows leave a bounce block for exactly their
destinations at any destination pitch, and entropy-coded segments become the files jpeg_assemble makes of them; a
capacity that is too small is DFX_ERR_UNSUPPORTED, and the may-not-fit test that keeps such a batch off a deferred tail
errs on the safe side only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DFX_OK, DFX_ERR_UNSUPPORTED = 0, 4


@pytest.fixture(scope="module")
def hand():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libhandover_harness.%d.so" % os.getpid())
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")  # jpeg_host.cpp shares a header with the kernels: types only
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", so, os.path.join(HERE, "handover_harness.cpp"),
                    os.path.join(ROOT, "denseflow_amd", "csrc", "jpeg_host.cpp")], check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    L.hh_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.hh_files.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                           C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.hh_may_not_fit.argtypes = [C.c_size_t, C.c_int, C.c_void_p, C.c_size_t]
    L.hh_assemble.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_ulonglong, C.c_void_p, C.c_size_t]
    L.hh_assemble.restype = C.c_size_t
    return L


def test_error_code_is_the_headers():
    text = open(os.path.join(ROOT, "include", "dfx.h")).read()
    assert "DFX_ERR_UNSUPPORTED = %d" % DFX_ERR_UNSUPPORTED in text


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("w,h", [(5, 3), (64, 4)])
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("two_planes", [False, True])
def test_rows_reach_exactly_their_destinations(hand, two_planes, nb, w, h, pad):
    rng = np.random.default_rng(w * 100 + nb * 10 + pad + two_planes)
    row = w if two_planes else w * 8
    pitch = row + pad
    # the bounce block as the download leaves it: float pairs back to back, or nb x planes and then nb y planes
    block = rng.integers(0, 256, (2 if two_planes else 1, nb, h, row), dtype=np.uint8)
    block[block == 0xA5] = 0  # the sentinel does not occur in the data
    dst = [np.full((n_dst, h, pitch), 0xA5, np.uint8) for n_dst in [nb, nb]]
    ptrs = [(C.c_void_p * nb)(*[d[j].ctypes.data for j in range(nb)]) for d in dst]
    assert hand.hh_rows(block.ctypes.data, int(two_planes), w, h, pitch, nb, ptrs[0], ptrs[1]) == DFX_OK
    for kind in range(2 if two_planes else 1):
        assert np.array_equal(dst[kind][:, :, :row], block[kind]), "a destination did not get its source rows"
        assert np.all(dst[kind][:, :, row:] == 0xA5), "bytes beyond the row were touched"
    if not two_planes:
        assert np.all(dst[1] == 0xA5), "a float batch has one destination per pair"


def _two_streams():
    """Two planes' entropy-coded segments in one landing buffer, each starting 4-byte aligned as the device lays them
    out: both contain 0xFF bytes (which assembly stuffs) and end on a partial byte."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, 41, dtype=np.uint8)
    a[[0, 7, 8, 39]] = 0xFF
    b = rng.integers(0, 256, 23, dtype=np.uint8)
    b[[3, 21]] = 0xFF
    bits = np.array([40 * 8 + 3, 22 * 8 + 5], np.uint64)
    a[40] &= 0xE0  # the bits beyond the segment are zero in the device stream
    b[22] = 0xF8   # ... and a last byte that becomes 0xFF once padded with ones is stuffed too
    base = np.array([0, 44], np.uint64)
    landing = np.zeros(44 + 24, np.uint8)
    landing[:41], landing[44:44 + 23] = a, b
    header = rng.integers(0, 256, 37, dtype=np.uint8)
    return header, landing, bits, base


def _direct(hand, header, landing, bits, base, j, capacity):
    out = np.zeros(capacity, np.uint8)
    n = hand.hh_assemble(header.ctypes.data, header.size, landing.ctypes.data + int(base[j]), int(bits[j]), out.ctypes.data, capacity)
    return out[:n]


def _files(hand, header, landing, bits, base, capacity):
    jpg = [np.full(capacity, 0xA5, np.uint8) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*[p.ctypes.data for p in jpg])
    sizes = np.zeros(2, np.uint32)
    msg = C.create_string_buffer(256)
    rc = hand.hh_files(header.ctypes.data, header.size, landing.ctypes.data, 2, bits.ctypes.data, base.ctypes.data, ptrs,
                       sizes.ctypes.data, capacity, msg, 256)
    return rc, jpg, sizes, msg.value.decode()


def test_files_are_what_jpeg_assemble_makes(hand):
    header, landing, bits, base = _two_streams()
    want = [_direct(hand, header, landing, bits, base, j, 256) for j in range(2)]
    assert all(len(f) > header.size + 2 for f in want)
    assert want[1][-4:].tobytes() == b"\xff\x00\xff\xd9"  # padded last byte stuffed, then EOI
    rc, jpg, sizes, msg = _files(hand, header, landing, bits, base, 256)
    assert rc == DFX_OK and msg == ""
    for j in range(2):
        assert sizes[j] == len(want[j]), "size slot not filled"
        assert np.array_equal(jpg[j][:sizes[j]], want[j])
        assert np.all(jpg[j][sizes[j]:] == 0xA5)
    # buffers of exactly the larger file's size still do
    exact = max(len(f) for f in want)
    rc, jpg, sizes, _ = _files(hand, header, landing, bits, base, exact)
    assert rc == DFX_OK and [int(s) for s in sizes] == [len(f) for f in want]


def test_a_capacity_one_byte_short_is_unsupported_and_never_deferred(hand):
    header, landing, bits, base = _two_streams()
    want = [_direct(hand, header, landing, bits, base, j, 256) for j in range(2)]
    short = max(len(f) for f in want) - 1
    rc, _, _, msg = _files(hand, header, landing, bits, base, short)
    assert rc == DFX_ERR_UNSUPPORTED and "jpg_capacity" in msg
    # the pre-check that keeps a batch off a deferred tail: true for that capacity, false where every byte could be stuffed
    assert hand.hh_may_not_fit(header.size, 2, bits.ctypes.data, short) == 1
    worst = header.size + 2 * max(int(b) // 8 + 1 for b in bits) + 2
    assert hand.hh_may_not_fit(header.size, 2, bits.ctypes.data, worst) == 0
    assert hand.hh_may_not_fit(header.size, 2, bits.ctypes.data, worst - 1) == 1
    assert _files(hand, header, landing, bits, base, worst)[0] == DFX_OK
