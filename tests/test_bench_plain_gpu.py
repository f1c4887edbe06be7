"""bench.py's plain run with REAL engines: the headline line alone (no side legs without --full) and --dump-outputs, which
must write the same flows for the same arguments run after run — the property two builds are compared by."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--frames", "9", "--width", "320", "--height", "240", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_line_and_dumped_flows_repeat(tmp_path):
    a = _run(tmp_path / "a", 2)
    b = _run(tmp_path / "b", 3)
    for out, steps in ((a, 2), (b, 3)):
        assert out["steps"] == steps and out["data"] == "synthetic" and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["config"]["pairs_per_step"] == 8
        assert "cpu_baseline" not in out and "parity_check" not in out and "pcie_inclusive" not in out["config"]
    assert os.listdir(tmp_path / "a") == ["flows.npy"]
    fa, fb = np.load(tmp_path / "a" / "flows.npy"), np.load(tmp_path / "b" / "flows.npy")
    assert fa.dtype == np.float32 and fa.shape == (8, 240, 320, 2) and np.isfinite(fa).all()
    assert np.abs(fa).max() > 0  # the synthetic clip moves
    assert np.array_equal(fa, fb)
