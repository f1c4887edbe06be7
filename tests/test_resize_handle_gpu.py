"""The host shell on the device with a list of clips of different sizes: one handle per algorithm, re-planned per clip
(dfx_set_size), writes the files that DF_NO_RESIZE_HANDLE=1 (destroy and create per size, as before) writes."""
import os
import re
import subprocess

import pytest

from denseflow_amd.synth import SynthClip
from tests.test_host_shell import _write_pgm_dir, built  # noqa: F401

pytestmark = pytest.mark.gpu


def _files(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("algo,st", [("tvl1", "jpg"), ("farn", "png")])
def test_mixed_size_list_is_the_same_files_with_one_handle(built, tmp_path, algo, st):  # noqa: F811
    shapes = [(64, 48, 5), (96, 64, 4), (65, 33, 3), (64, 48, 4)]
    lines = []
    for i, (w, h, n) in enumerate(shapes):
        _write_pgm_dir(tmp_path / f"clip{i}", SynthClip(w, h, 70 + i).frames(n))
        lines.append(str(tmp_path / f"clip{i}"))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    outs, logs = {}, {}
    for tag, env in (("resize", {}), ("recreate", {"DF_NO_RESIZE_HANDLE": "1"})):
        r = subprocess.run([built, str(tmp_path / "list.txt"), "-o=" + str(tmp_path / tag), "-a=" + algo, "-s=1", "-b=20",
                            "-st=" + st, "-if"], capture_output=True, text=True, env={**os.environ, **env, "DF_TRACE": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag], logs[tag] = _files(tmp_path / tag), r.stdout + r.stderr
    assert len(re.findall(r"engine for \d+x\d+ ready", logs["resize"])) == 1
    assert re.findall(r"engine re-planned for (\d+x\d+)", logs["resize"]) == ["96x64", "65x33", "64x48"]
    assert len(re.findall(r"engine for \d+x\d+ ready", logs["recreate"])) == 4 and "re-planned" not in logs["recreate"]
    n_files = sum(1 for k in outs["resize"] if k.endswith("." + st))
    assert n_files == (2 if st == "jpg" else 1) * sum(n - 1 for _, _, n in shapes)
    assert outs["resize"] == outs["recreate"]


def test_mixed_source_sizes_with_one_target_write_the_same_files(built, tmp_path):  # noqa: F811
    """--nw / --nh: every clip has the same flow size and only the sources differ.  Such clips may share a library call
    (dfx_next_segments_src; whether they do depends on what is queued when the flow stage looks) — the files are the ones
    the clip-by-clip run writes, and the ones of DF_NO_JOIN=1."""
    shapes = [(64, 48, 5), (96, 64, 4), (33, 47, 3), (64, 48, 4), (48, 36, 2)]
    lines = []
    for i, (w, h, n) in enumerate(shapes):
        _write_pgm_dir(tmp_path / f"clip{i}", SynthClip(w, h, 80 + i).frames(n))
        lines.append(str(tmp_path / f"clip{i}"))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    outs, logs = {}, {}
    for tag, env in (("mixed", {}), ("parent", {"DF_NO_RESIZE_HANDLE": "1"}), ("single", {"DF_NO_JOIN": "1"})):
        r = subprocess.run([built, str(tmp_path / "list.txt"), "-o=" + str(tmp_path / tag), "-a=farn", "-s=1", "-b=20",
                            "-nw=48", "-nh=36", "-if"], capture_output=True, text=True,
                           env={**os.environ, **env, "DF_TRACE": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        outs[tag], logs[tag] = _files(tmp_path / tag), r.stdout + r.stderr
    print("calls that joined clips of different source sizes:", logs["mixed"].count("clips of different source sizes"))
    assert "clips of different source sizes" not in logs["parent"] + logs["single"]
    assert sum(1 for k in outs["mixed"] if k.endswith(".jpg")) == 2 * sum(n - 1 for _, _, n in shapes)
    assert outs["mixed"] == outs["parent"] == outs["single"]
