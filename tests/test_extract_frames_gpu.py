"""Colour frame extraction on the device (-s=0; reference /root/reference/src/denseflow_gpu.cpp:82-105) against its
pins: dfx_encode_jpeg_bgr == the host encoder == libjpeg-turbo (Pillow live, else tests/golden/jpeg_colour_golden.npz);
dfx_prepare_frames_bgr == the gray resize oracle on B, G, R; dfx_extract_frames == libjpeg-turbo of the oracle-resized
frames; the DFX_ALGO_FRAMES handle; the CLI on a folder of .ppm frames."""
import os
import subprocess

import numpy as np
import pytest

import denseflow_amd
from denseflow_amd import engine as E
from tests import colour_cases as cc
from tests.test_host_shell import built  # noqa: F401  (fixture)
from tests.test_jpeg_colour_pin import colour_harness, host_encode  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _want(colour_harness, kind, w, h, q, bgr):  # noqa: F811
    """The bytes a case must give: the host twin's, themselves held to libjpeg-turbo where a reference exists."""
    host = host_encode(colour_harness, bgr, q)
    ref, _ = cc.reference(kind, w, h, q, bgr)
    if ref is not None:
        assert host == ref, (kind, w, h, q, "host twin vs libjpeg-turbo")
    return host


def _resize_oracle(oracle, bgr, dw, dh):
    return np.stack([oracle.prepare_frame(np.ascontiguousarray(bgr[..., c]), dw, dh) for c in range(3)], -1)


@pytest.mark.parametrize("w,h", cc.SIZES)
def test_encode_jpeg_bgr_is_the_host_encoder_and_libjpeg(colour_harness, w, h):  # noqa: F811
    qs = (95,) if w * h > 500000 else cc.QUALITIES
    with denseflow_amd.FlowEngine(w, h, "frames") as eng:
        for q in qs:
            frames = [cc.frame(k, w, h, 0) for k in cc.KINDS]
            got = eng.encode_jpeg_bgr(frames, q)
            for k, f, g in zip(cc.KINDS, frames, got):
                assert g == _want(colour_harness, k, w, h, q, f), (w, h, q, k)
        # two calls in a row at one quality: the buffers are reused
        f = cc.frame("smooth", w, h, 5)
        first = eng.encode_jpeg_bgr([f], 95)
        assert eng.encode_jpeg_bgr([f], 95) == first == [_want(colour_harness, "smooth", w, h, 95, f)]


def test_encode_jpeg_bgr_noise_batch_grows_the_stream_buffer(colour_harness):  # noqa: F811
    w, h = 320, 240
    frames = [cc.frame("noise", w, h, s) for s in range(12)]  # ~8 bits per pixel at quality 100: beyond the 4 provided
    with denseflow_amd.FlowEngine(w, h, "frames") as eng:
        got = eng.encode_jpeg_bgr(frames, 100)
        again = eng.encode_jpeg_bgr(frames[:3], 100)
    assert got == [host_encode(colour_harness, f, 100) for f in frames]
    assert again == got[:3]


def test_encode_jpeg_bgr_mixed_flat_and_busy_frames(colour_harness):  # noqa: F811
    w, h = 257, 131
    kinds = ["constant", "noise", "smooth", "constant", "primaries", "noise", "constant"]
    frames = [cc.frame(k, w, h, i) for i, k in enumerate(kinds)]
    with denseflow_amd.FlowEngine(w, h, "frames", max_batch=3) as eng:
        got = eng.encode_jpeg_bgr(frames, 95)
    assert got == [host_encode(colour_harness, f, 95) for f in frames]


@pytest.mark.parametrize("sw,sh,dw,dh", [(64, 48, 101, 75), (70, 45, 33, 17), (128, 96, 64, 48), (57, 43, 57, 43), (321, 243, 160, 121)])
def test_prepare_frames_bgr_is_the_gray_oracle_per_channel(oracle, sw, sh, dw, dh):
    frames = [cc.frame(k, sw, sh, 2) for k in ("noise", "smooth", "primaries")]
    with denseflow_amd.FlowEngine(dw, dh, "frames") as eng:
        got = eng.prepare_frames_bgr(frames)
        # odd pitches: rows 5 bytes apart from dense
        L, n = eng._L, len(frames)
        import ctypes as C
        sp, dp = sw * 3 + 5, dw * 3 + 7
        src = np.zeros((n, sh, sp), np.uint8)
        for i, f in enumerate(frames):
            src[i, :, :sw * 3] = f.reshape(sh, sw * 3)
        dst = np.zeros((n, dh, dp), np.uint8)
        rc = L.dfx_prepare_frames_bgr(eng._h, (C.c_void_p * n)(*[src[i].ctypes.data for i in range(n)]), sp, sw, sh, n,
                                      (C.c_void_p * n)(*[dst[i].ctypes.data for i in range(n)]), dp)
        assert rc == 0
    for i, f in enumerate(frames):
        want = _resize_oracle(oracle, f, dw, dh)
        assert np.array_equal(got[i], want), (sw, sh, dw, dh, i)
        assert np.array_equal(dst[i, :, :dw * 3].reshape(dh, dw, 3), want) and not dst[i, :, dw * 3:].any()


@pytest.mark.parametrize("algo", ["frames", "farn"])
@pytest.mark.parametrize("submit", [False, True])
def test_extract_frames_is_libjpeg_of_the_oracle_resize(colour_harness, oracle, algo, submit):  # noqa: F811
    sw, sh = 128, 96
    frames = [cc.frame(k, sw, sh, i) for i, k in enumerate(["smooth", "noise", "primaries", "constant", "smooth", "noise", "smooth"])]
    for (dw, dh) in [(64, 48), (85, 64), (128, 96), (150, 113)]:
        with denseflow_amd.FlowEngine(dw, dh, algo, max_batch=3) as eng:  # 7 frames: three device batches
            got = eng.extract_frames(frames, 95, submit=submit)
            again = eng.extract_frames(frames[:4], 95, submit=submit)
        want = []
        for f in frames:
            r = _resize_oracle(oracle, f, dw, dh) if (dw, dh) != (sw, sh) else f
            b = host_encode(colour_harness, r, 95)
            if cc.have_pillow():
                assert b == cc.libjpeg(r, 95)
            want.append(b)
        assert got == want, (algo, submit, dw, dh)
        assert again == want[:4]


def test_frames_handle_refuses_flow_and_stays_small():
    with denseflow_amd.FlowEngine(1920, 1080, "frames") as eng:
        f = cc.frame("smooth", 1920, 1080, 0)
        assert len(eng.extract_frames([f] * 20, 95)) == 20
        held = eng.frames_device_bytes()
        print("frames handle at 1920x1080 holds", held, "bytes of device memory")
        assert 0 < held < (1 << 30)
    with denseflow_amd.FlowEngine(96, 64, "frames") as eng:
        g = np.zeros((64, 96), np.uint8)
        for call in (lambda: eng.calc(g, g), lambda: eng.calc_optflows([g, g], 1), lambda: eng.calc_optflows_u8([g, g], 1, 20),
                     lambda: eng.calc_optflows_jpeg([g, g], 1, 20), lambda: eng.submit_optflows([g, g], 1)):
            with pytest.raises(E.DfxError) as ei:
                call()
            assert ei.value.status == E.ERR_UNSUPPORTED


def _write_ppms(folder, frames):
    folder.mkdir(parents=True)
    for i, f in enumerate(frames):
        h, w, _ = f.shape
        (folder / f"f_{i:05d}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(f[..., ::-1]).tobytes())


@pytest.mark.parametrize("ns", [0, 48])
def test_cli_extracts_colour_frames(built, colour_harness, oracle, tmp_path, ns):  # noqa: F811
    sw, sh = 128, 96
    frames = [cc.frame(k, sw, sh, i) for i, k in enumerate(["smooth", "primaries", "noise", "smooth", "constant"])]
    _write_ppms(tmp_path / "clip", frames)
    dw, dh = (64, 48) if ns else (sw, sh)
    want = [host_encode(colour_harness, _resize_oracle(oracle, f, dw, dh) if ns else f, 95) for f in frames]
    outs = {}
    for tag, env in (("dev", {}), ("host", {"DF_HOST_JPEG": "1", "DF_HOST_RESIZE": "1"})):
        (tmp_path / tag).mkdir()
        args = [built, str(tmp_path / "clip"), "-o=" + str(tmp_path / tag), "--if", "-s=0"] + (["--ns=%d" % ns] if ns else [])
        r = subprocess.run(args, capture_output=True, text=True, env={**os.environ, **env}, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "GRAY frames" not in r.stdout
        assert "1 videos (5 frames, 0 tvl1 flows) processed" in r.stdout, r.stdout
        outs[tag] = [(tmp_path / tag / "clip" / f"img_{i:05d}.jpg").read_bytes() for i in range(5)]
        assert outs[tag] == want, tag
    if cc.have_pillow():
        import io

        from PIL import Image

        im = Image.open(io.BytesIO(outs["dev"][0]))
        assert im.mode == "RGB" and im.size == (dw, dh)
