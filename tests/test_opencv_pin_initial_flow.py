"""Pinning caller-supplied initial flows (dfx_calc_batch_init*) against real OpenCV — active only when
tests/golden/opencv_tvl1_init.npz / opencv_farn_init.npz exist (scripts/pin_against_opencv.py on a machine with cv2.cuda:
OpticalFlowDual_TVL1 with useInitialFlow = true and FarnebackOpticalFlow with OPTFLOW_USE_INITIAL_FLOW on the two smallest
of the committed seeds, each seeded with half of that case's own unseeded OpenCV flow).  The files are absent here, so every
test SKIPS: the seeded paths are restated from memory of opencv_contrib 4.5.x cudaoptflow, rated MED, parity unpinned
(SURVEY.md A.11 — with its open point, scaleStep against the CPU class's 0.5 — and B.12).  With a file present the reference
(tests/initial_flow_ref.py) and the HIP path are held to OpenCV's flows by the graded statistic of tests/flow_stats.py, as
tests/test_opencv_pin.py holds the unseeded paths."""
import os
import re

import numpy as np
import pytest

from tests import flow_stats as FS
from tests import initial_flow_ref as IR

GOLDEN = {a: os.path.join(os.path.dirname(__file__), "golden", f"opencv_{a}_init.npz") for a in ("tvl1", "farn")}
ENGINE = {"tvl1": "tvl1", "farn": "farn"}


def _cases(algo):
    path = GOLDEN[algo]
    if not os.path.exists(path):
        pytest.skip(f"{path} absent: run scripts/pin_against_opencv.py where cv2.cuda exists (parity unpinned until then)")
    g = np.load(path)
    out = []
    for k in g.files:
        m = re.match(r"(.*)_seed$", k)
        if m:
            n = m.group(1)
            out.append((n, g[n + "_f0"], g[n + "_f1"], g[k].astype(np.float32), g[n + "_flow"]))
    return out


def _reference(oracle, algo, f0, f1, seed):
    if algo == "tvl1":
        return IR.tvl1_init_calc(oracle, f0, f1, seed)[0]
    return IR.farneback_init_calc(oracle, f0, f1, seed)[0]


@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_seeded_reference_reproduces_opencv_cuda(oracle, algo):
    stats = [(name, FS.pair_stat(_reference(oracle, algo, f0, f1, seed), flow)) for name, f0, f1, seed, flow in _cases(algo)]
    print(FS.table(stats), FS.gate(stats, f"{algo} seeded reference vs cv::cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["tvl1", "farn"])
def test_hip_path_reproduces_opencv_cuda(dfx, algo):
    stats = []
    for name, f0, f1, seed, flow in _cases(algo):
        h, w = f0.shape
        with dfx.FlowEngine(w, h, ENGINE[algo]) as eng:
            stats.append((name, FS.pair_stat(eng.calc(f0, f1, init=seed), flow)))
    print(FS.table(stats), FS.gate(stats, f"HIP {algo} with an initial flow vs cv::cuda"))
