"""Pinning the illumination channel of -a=tvl1 (dfx_params.tvl1_gamma != 0) against real OpenCV — active only when
tests/golden/opencv_tvl1_gamma.npz exists (scripts/pin_against_opencv.py on a machine with cv2.cuda:
cv::cuda::OpticalFlowDual_TVL1::create(..., gamma = 0.4 / 2.0, useInitialFlow = false) on the two smallest of the
committed seeds, 64 x 48 and 224 x 224: with more of them the fixture would pass the 1 MiB a committed file may have).
The file is absent here, so every test SKIPS: the gamma path is restated from memory of opencv_contrib 4.5.x
(cudaoptflow/src/tvl1flow.cpp, cuda/tvl1flow.cu), rated MED, parity unpinned.  With the file present the reference of the
gamma tests (tests/tvl1_gamma_ref.py) and the HIP path are held to OpenCV's flows by the graded statistic of
tests/flow_stats.py, as tests/test_opencv_pin.py holds the gamma = 0 path."""
import os
import re

import numpy as np
import pytest

from tests import flow_stats as FS
from tests import tvl1_gamma_ref as GR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "opencv_tvl1_gamma.npz")


def _cases():
    if not os.path.exists(GOLDEN):
        pytest.skip(f"{GOLDEN} absent: run scripts/pin_against_opencv.py where cv2.cuda exists (parity unpinned until then)")
    g = np.load(GOLDEN)
    out = []
    for k in g.files:
        m = re.match(r"(.*)_gamma([0-9.]+)_flow$", k)
        if m:
            out.append((f"{m.group(1)} gamma {m.group(2)}", float(m.group(2)), g[m.group(1) + "_f0"], g[m.group(1) + "_f1"], g[k]))
    return out


def test_gamma_reference_reproduces_opencv_cuda():
    stats = [(name, FS.pair_stat(GR.tvl1_gamma_calc(f0, f1, gamma)[0], flow)) for name, gamma, f0, f1, flow in _cases()]
    print(FS.table(stats), FS.gate(stats, "TVL1 gamma reference vs cv::cuda"))


@pytest.mark.gpu
def test_hip_path_reproduces_opencv_cuda(dfx):
    stats = []
    for name, gamma, f0, f1, flow in _cases():
        h, w = f0.shape
        with dfx.FlowEngine(w, h, "tvl1", tvl1_gamma=gamma) as eng:
            stats.append((name, FS.pair_stat(eng.calc(f0, f1), flow)))
    print(FS.table(stats), FS.gate(stats, "HIP tvl1 with gamma vs cv::cuda"))
