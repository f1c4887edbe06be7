"""The host shell's colour -s=0 path without a device: linked against the test-only ABI fake (tests/stub_dfx.cpp, which
has none of the colour entry points) the shell must still link — no hard reference to them — and write libjpeg-turbo's
colour files for a folder of .ppm frames through its host twins; gray sources keep their gray files and their note."""
import io

import numpy as np
import pytest

from tests import colour_cases as cc
from tests.test_host_pipeline_stub import _run, stub  # noqa: F401  (fixture, runner)
from tests.test_host_shell import built  # noqa: F401  (fixture)
from tests.test_jpeg_colour_pin import colour_harness, host_encode, host_resize  # noqa: F401  (fixture)


def _write_ppms(folder, frames):
    folder.mkdir(parents=True)
    for i, f in enumerate(frames):
        h, w, _ = f.shape
        (folder / f"f_{i:05d}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(f[..., ::-1]).tobytes())


@pytest.mark.parametrize("ns", [0, 24])
def test_stub_linked_shell_writes_libjpegs_colour_files(stub, colour_harness, tmp_path, ns):  # noqa: F811
    sw, sh = 70, 45
    frames = [cc.frame(k, sw, sh, i) for i, k in enumerate(["smooth", "primaries", "noise", "constant"])]
    _write_ppms(tmp_path / "clip", frames)
    (tmp_path / "o").mkdir()
    r = _run(stub, [tmp_path / "clip", "-o=" + str(tmp_path / "o"), "--if", "-s=0"] + (["--ns=%d" % ns] if ns else []))
    assert "GRAY frames" not in r.stdout
    assert "1 videos (4 frames, 0 tvl1 flows) processed" in r.stdout, r.stdout
    dw, dh = (int(round(sw / sh * ns)), ns) if ns else (sw, sh)
    for i, f in enumerate(frames):
        got = (tmp_path / "o" / "clip" / f"img_{i:05d}.jpg").read_bytes()
        src = host_resize(colour_harness, f, dw, dh) if ns else f
        assert got == host_encode(colour_harness, src, 95)
        if cc.have_pillow():
            from PIL import Image

            assert got == cc.libjpeg(src, 95)
            im = Image.open(io.BytesIO(got))
            assert im.mode == "RGB" and im.size == (dw, dh)


def test_gray_sources_keep_their_gray_files_and_note(stub, tmp_path):  # noqa: F811
    rng = np.random.default_rng(4)
    w, h, n = 40, 24, 3
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]
    (tmp_path / "pg").mkdir()
    for i, p in enumerate(planes):
        (tmp_path / "pg" / f"f_{i:05d}.pgm").write_bytes(b"P5\n%d %d\n255\n" % (w, h) + p.tobytes())
    with open(tmp_path / "mono.y4m", "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d F25:1 Ip A1:1 Cmono\n" % (w, h))
        for p in planes:
            f.write(b"FRAME\n" + p.tobytes())
    for tag, src, extra in (("a", tmp_path / "pg", ["--if"]), ("b", tmp_path / "mono.y4m", [])):
        (tmp_path / tag).mkdir()
        r = _run(stub, [src, "-o=" + str(tmp_path / tag), "-s=0"] + extra)
        assert "-s=0 in this build writes GRAY frames" in r.stdout
        name = "pg" if tag == "a" else "mono"
        for i, p in enumerate(planes):
            got = (tmp_path / tag / name / f"img_{i:05d}.jpg").read_bytes()
            seg = cc.segments(got)
            assert [m for m, _ in seg] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA] and dict(seg)[0xC0][5] == 1  # one component
            if cc.have_pillow():
                from PIL import Image

                b = io.BytesIO()
                Image.fromarray(p, "L").save(b, "JPEG", quality=95)
                assert got == b.getvalue()
