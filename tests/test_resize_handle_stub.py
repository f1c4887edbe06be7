"""The host shell against the test-only ABI fake (tests/stub_dfx.cpp, which has no dfx_set_size): the shell resolves the
entry point weakly, so here it keeps destroying and creating its handle when a clip's size differs from the last one's —
the path DF_NO_RESIZE_HANDLE=1 forces against the real library.  A list of three .pgm clips of different sizes must write
the same files either way, one engine per size.  What this guards is the weak resolution itself — a shell linked against
an ABI without dfx_set_size / dfx_next_segments_src must neither crash on the null symbols nor join clips of different
sizes; it cannot see a defect of dfx_set_size.  The GPU suite holds dfx_set_size itself against fresh handles
(tests/test_set_size_gpu.py)."""
import re

from denseflow_amd.synth import SynthClip
from tests.test_host_pipeline_stub import _files, _run, stub  # noqa: F401
from tests.test_host_shell import _write_pgm_dir, built  # noqa: F401


def test_a_list_of_clips_of_three_sizes_writes_the_same_files_either_way(stub, tmp_path):  # noqa: F811
    shapes = [(64, 48, 5), (96, 64, 4), (48, 80, 6)]
    lines = []
    for i, (w, h, n) in enumerate(shapes):
        _write_pgm_dir(tmp_path / f"clip{i}", SynthClip(w, h, 60 + i).frames(n))
        lines.append(str(tmp_path / f"clip{i}"))
    (tmp_path / "list.txt").write_text("\n".join(lines) + "\n")
    outs = {}
    for tag, env in (("resize", {}), ("recreate", {"DF_NO_RESIZE_HANDLE": "1"})):
        r = _run(stub, [tmp_path / "list.txt", "-o=" + str(tmp_path / tag), "-a=tvl1", "-s=1", "-b=20", "-if"],
                 {**env, "DF_TRACE": "1"})
        outs[tag] = _files(tmp_path / tag)
        # the fake has no dfx_set_size: every size gets an engine of its own, in both runs
        assert sorted(re.findall(r"engine for (\d+x\d+) ready", r.stdout + r.stderr)) == ["48x80", "64x48", "96x64"]
        assert "re-planned" not in r.stdout + r.stderr
    names = sorted(k for k in outs["resize"] if k.endswith(".jpg"))
    assert len(names) == 2 * sum(n - 1 for _, _, n in shapes)
    assert outs["resize"] == outs["recreate"]
