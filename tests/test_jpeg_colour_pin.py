"""PIN of the colour JPEG stage (the reference's imencode(".jpg", frame) of -s=0, /root/reference/src/denseflow_gpu.cpp:
82-105) against the real libjpeg: the host encoder for BGR frames (src/image_io.cpp: YCbCr 4:2:0, one interleaved scan)
writes libjpeg-turbo's bytes.  Live against Pillow where it imports, against tests/golden/jpeg_colour_golden.npz
everywhere (minted by tests/golden/make_jpeg_colour_golden.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import colour_cases as cc
from tests.test_host_shell import built  # noqa: F401  (fixture)

ROOT = cc.ROOT


@pytest.fixture(scope="module")
def colour_harness(built):  # noqa: F811
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libcolour_harness.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"), "-o", so,
           os.path.join(ROOT, "tests", "colour_harness.cpp"), os.path.join(ROOT, "build", "libzzdenseflow.a"),
           "-L" + os.path.join(ROOT, "denseflow_amd", "lib"), "-ldfx", "-lpthread", "-lz",
           "-Wl,-rpath," + os.path.join(ROOT, "denseflow_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    L = C.CDLL(so)
    L.ch_encode_jpeg_bgr.restype = C.c_longlong
    L.ch_encode_jpeg_bgr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong]
    L.ch_resize_bgr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    L.ch_imread_color.argtypes = [C.c_char_p, C.c_void_p, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def host_encode(L, bgr, quality, portable=0):
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w, _ = bgr.shape
    buf = np.zeros(w * h * 6 + 4096, np.uint8)
    L.ch_jpeg_force_portable(portable)
    n = L.ch_encode_jpeg_bgr(bgr.ctypes.data, w, h, quality, buf.ctypes.data, buf.size)
    L.ch_jpeg_force_portable(0)
    assert n > 0
    return buf[:n].tobytes()


def host_resize(L, bgr, dw, dh):
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    out = np.empty((dh, dw, 3), np.uint8)
    L.ch_resize_bgr(bgr.ctypes.data, bgr.shape[1], bgr.shape[0], out.ctypes.data, dw, dh)
    return out


@pytest.mark.parametrize("w,h", cc.SIZES)
def test_host_colour_encoder_writes_libjpegs_bytes(colour_harness, w, h):
    checked = 0
    for q in cc.qualities(w, h):
        for kind in cc.KINDS:
            bgr = cc.frame(kind, w, h, 0)
            want, _ = cc.reference(kind, w, h, q, bgr)
            if want is None:
                continue
            checked += 1
            assert host_encode(colour_harness, bgr, q) == want, (w, h, q, kind, "vector form")
            if w * h <= 100000:
                assert host_encode(colour_harness, bgr, q, portable=1) == want, (w, h, q, kind, "scalar form")
    if cc.have_pillow():
        assert checked == len(cc.qualities(w, h)) * len(cc.KINDS)
    else:
        assert checked > 0 or w * h > 640 * 360  # the golden file leaves 1080p to the boxes with Pillow


def test_golden_file_is_libjpegs_and_the_host_matches_it(colour_harness):
    """The committed fallback itself: every case in it equals the host encoder (and Pillow, where it imports)."""
    assert os.path.exists(cc.GOLDEN)
    for kind, w, h, q in cc.GOLDEN_CASES:
        want = cc.golden(kind, w, h, q)
        assert want is not None, (kind, w, h, q)
        bgr = cc.frame(kind, w, h, 0)
        assert host_encode(colour_harness, bgr, q) == want, (kind, w, h, q)
        if cc.have_pillow():
            assert cc.libjpeg(bgr, q) == want, (kind, w, h, q)


def test_colour_header_segments(colour_harness):
    """Segment list and SOF0 / SOS payloads of cv::imencode's colour file: two DQT, three components 1:0x22:0, 2:0x11:1,
    3:0x11:1, four DHT (DC0 AC0 DC1 AC1), one interleaved scan."""
    data = host_encode(colour_harness, cc.frame("smooth", 70, 45, 0), 95)
    seg = cc.segments(data)
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    sof = dict(seg)[0xC0]
    assert sof == bytes([8, 0, 45, 0, 70, 3, 1, 34, 0, 2, 17, 1, 3, 17, 1])
    assert dict(seg)[0xDA] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert [p[0] for m, p in seg if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    assert [p[0] for m, p in seg if m == 0xDB] == [0, 1]
    assert data[-2:] == b"\xff\xd9"


def test_random_colour_frames_against_libjpeg(colour_harness):
    """Property form of the live pin: W, H in 1 ... 150, any quality, seeded content; scalar and vector transforms."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    pytest.importorskip("PIL.Image")

    @settings(max_examples=150, deadline=None)
    @given(w=st.integers(1, 150), h=st.integers(1, 150), q=st.integers(1, 100), kind=st.integers(0, 3), seed=st.integers(0, 2 ** 31))
    def check(w, h, q, kind, seed):
        bgr = cc.frame(cc.KINDS[kind], w, h, seed)
        want = cc.libjpeg(bgr, q)
        assert host_encode(colour_harness, bgr, q) == want
        assert host_encode(colour_harness, bgr, q, portable=1) == want

    check()


def test_three_channel_resize_is_the_gray_resize_per_channel(colour_harness, oracle):
    """cv::resize treats channels independently: the host's 3-channel resizeLinear == the gray oracle on B, G, R."""
    for (sw, sh, dw, dh) in [(64, 48, 32, 24), (70, 45, 33, 17), (33, 17, 70, 45), (40, 30, 40, 30), (57, 43, 101, 25)]:
        src = cc.frame("noise", sw, sh, 3)
        got = host_resize(colour_harness, src, dw, dh)
        for c in range(3):
            assert np.array_equal(got[..., c], oracle.prepare_frame(np.ascontiguousarray(src[..., c]), dw, dh)), (sw, sh, dw, dh, c)


def test_ppm_reader_gives_bgr(colour_harness, tmp_path):
    rgb = cc.frame("noise", 13, 7, 1)[..., ::-1]
    (tmp_path / "a.ppm").write_bytes(b"P6\n13 7\n255\n" + np.ascontiguousarray(rgb).tobytes())
    (tmp_path / "b.pgm").write_bytes(b"P5\n13 7\n255\n" + bytes(13 * 7))
    buf = np.zeros(13 * 7 * 3, np.uint8)
    w, h = C.c_int(0), C.c_int(0)
    assert colour_harness.ch_imread_color(str(tmp_path / "a.ppm").encode(), buf.ctypes.data, buf.size, C.byref(w), C.byref(h)) == 1
    assert (w.value, h.value) == (13, 7) and np.array_equal(buf.reshape(7, 13, 3), rgb[..., ::-1])
    assert colour_harness.ch_imread_color(str(tmp_path / "b.pgm").encode(), buf.ctypes.data, buf.size, C.byref(w), C.byref(h)) == 0
