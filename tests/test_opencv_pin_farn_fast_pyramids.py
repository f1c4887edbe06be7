"""Pinning fast pyramids of -a=farn (dfx_params.farn_fast_pyramids = 1) against real OpenCV — active only when
tests/golden/opencv_farn_fast_pyramids.npz exists (scripts/pin_against_opencv.py on a machine with cv2.cuda:
cv::cuda::FarnebackOpticalFlow::create(3, 0.5, true, 13, 10, 5, 1.1, 0) on the committed seeds whose sizes the level rule
accepts).  The file is absent here, so every test SKIPS: the fast path is restated from memory of opencv_contrib 4.5.x
(cudaoptflow/src/farneback.cpp, cudawarping's pyr_down.cu / pyr_up.cu), rated MED (the pyrUp border rule LOW), parity
unpinned.  With the file present the reference of the fast-pyramid tests (tests/farneback_fastpyr_ref.py) and the HIP path
are held to OpenCV's flows by the graded statistic of tests/flow_stats.py, as tests/test_opencv_pin.py holds the default path."""
import os

import numpy as np
import pytest

from tests import farneback_fastpyr_ref as FR
from tests import flow_stats as FS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "opencv_farn_fast_pyramids.npz")
LEVELS = 3


def _cases():
    if not os.path.exists(GOLDEN):
        pytest.skip(f"{GOLDEN} absent: run scripts/pin_against_opencv.py where cv2.cuda exists (parity unpinned until then)")
    g = np.load(GOLDEN)
    return [(k[:-5], g[k[:-5] + "_f0"], g[k[:-5] + "_f1"], g[k]) for k in g.files if k.endswith("_flow")]


def test_fast_pyramid_reference_reproduces_opencv_cuda(oracle):
    p = oracle.farneback_default_params()
    p.num_levels = LEVELS
    stats = [(name, FS.pair_stat(FR.farneback_flow(oracle, f0, f1, p, fast=True), flow)) for name, f0, f1, flow in _cases()]
    print(FS.table(stats), FS.gate(stats, "fast-pyramid reference vs cv::cuda"))


@pytest.mark.gpu
def test_hip_path_reproduces_opencv_cuda(dfx):
    stats = []
    for name, f0, f1, flow in _cases():
        h, w = f0.shape
        with dfx.FlowEngine(w, h, "farn", farn_num_levels=LEVELS, farn_fast_pyramids=1) as eng:
            stats.append((name, FS.pair_stat(eng.calc(f0, f1), flow)))
    print(FS.table(stats), FS.gate(stats, "HIP farn, fast pyramids, vs cv::cuda"))
