"""Pinning the Gaussian update window of -a=farn (dfx_params.farn_window = DFX_FARN_WINDOW_GAUSSIAN) against real OpenCV —
active only when tests/golden/opencv_farn_gaussian.npz exists (scripts/pin_against_opencv.py on a machine with cv2.cuda:
cv::cuda::FarnebackOpticalFlow::create(5, 0.5, false, 15, 10, 5, 1.1, OPTFLOW_FARNEBACK_GAUSSIAN) on the committed seeds).
The file is absent here, so every test SKIPS: the Gaussian path is restated from memory of opencv_contrib 4.5.2
(cudaoptflow/src/farneback.cpp, cuda/farneback.cu: gaussianBlur5), rated MED, parity unpinned.  With the file present the
reference of the window tests (tests/farneback_window_ref.py) and the HIP path are held to OpenCV's flows by the graded
statistic of tests/flow_stats.py, as tests/test_opencv_pin.py holds the box path."""
import os

import numpy as np
import pytest

from tests import farneback_window_ref as WR
from tests import flow_stats as FS

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "opencv_farn_gaussian.npz")
WIN = 15


def _cases():
    if not os.path.exists(GOLDEN):
        pytest.skip(f"{GOLDEN} absent: run scripts/pin_against_opencv.py where cv2.cuda exists (parity unpinned until then)")
    g = np.load(GOLDEN)
    return [(k[:-5], g[k[:-5] + "_f0"], g[k[:-5] + "_f1"], g[k]) for k in g.files if k.endswith("_flow")]


def test_window_reference_reproduces_opencv_cuda(oracle):
    p = oracle.farneback_default_params()
    p.win_size = WIN
    stats = [(name, FS.pair_stat(WR.farneback_flow(oracle, f0, f1, p, "gaussian"), flow)) for name, f0, f1, flow in _cases()]
    print(FS.table(stats), FS.gate(stats, "Gaussian-window reference vs cv::cuda"))


@pytest.mark.gpu
def test_hip_path_reproduces_opencv_cuda(dfx):
    stats = []
    for name, f0, f1, flow in _cases():
        h, w = f0.shape
        with dfx.FlowEngine(w, h, "farn", farn_win_size=WIN, farn_window=1) as eng:
            stats.append((name, FS.pair_stat(eng.calc(f0, f1), flow)))
    print(FS.table(stats), FS.gate(stats, "HIP farn, Gaussian window, vs cv::cuda"))
