#!/usr/bin/env python3
"""Pin the oracle to real OpenCV output — to be run on ANY machine that has an OpenCV build with the CUDA modules
(`cv2.cuda`, opencv_contrib cudaoptflow; the reference pins 4.5.2, /root/reference/docker/Dockerfile:6).

This environment has no OpenCV, so the flow oracles are "parity unpinned".  This script is the kit that
closes the gap the moment such a machine is reachable: it evaluates the very calls the reference makes
(/root/reference/src/denseflow_gpu.cpp:299-303, :327-334) on the committed synthetic seeds and writes

    tests/golden/opencv_tvl1.npz   opencv_farn.npz   opencv_farn_gaussian.npz   opencv_brox.npz   [opencv_cpu_tvl1.npz]

each holding, per case, the two uint8 frames and the CV_32FC2 flow OpenCV returned, plus cv2.getBuildInformation().
tests/test_opencv_pin.py picks the files up when present: the CPU oracle (-m "not gpu") and the HIP path (-m gpu)
must then agree with OpenCV within BASELINE.json's 1e-3 max-abs (TVL1, Farneback) — and the Brox oracle, which today
DEFINES its algorithm, gets its first external check.  opencv_farn_gaussian.npz is the Gaussian update window
(dfx_params.farn_window, restated from memory and rated MED): winSize 15 with OPTFLOW_FARNEBACK_GAUSSIAN, picked up by
tests/test_opencv_pin_farn_gaussian.py.  opencv_tvl1_gamma.npz is the illumination channel of TVL1 (dfx_params.tvl1_gamma,
restated from memory and rated MED): cuda.OpticalFlowDual_TVL1_create(gamma=0.4) and gamma=2.0 on the two smallest seeds
(the file stays below the 1 MiB a committed fixture may have), picked up by tests/test_opencv_pin_tvl1_gamma.py.
opencv_tvl1_init.npz / opencv_farn_init.npz are the caller-supplied initial flows (dfx_calc_batch_init*, restated from memory
and rated MED): OpticalFlowDual_TVL1 with useInitialFlow = true and FarnebackOpticalFlow with OPTFLOW_USE_INITIAL_FLOW on
the two smallest seeds, each seeded with that case's own unseeded OpenCV flow scaled by 0.5 (stored beside the result),
picked up by tests/test_opencv_pin_initial_flow.py.  opencv_farn_fast_pyramids.npz is fastPyramids
(dfx_params.farn_fast_pyramids, restated from memory and rated MED): create(3, 0.5, True, 13, 10, 5, 1.1, 0) on the two smallest
seeds — sizes whose levels below the coarsest are even, the only ones upstream defines a result for — picked up by
tests/test_opencv_pin_farn_fast_pyramids.py.  Nothing here imports the product or the oracle.

    python scripts/pin_against_opencv.py [--out tests/golden] [--testdata $OPENCV_TEST_DATA_PATH]
With --testdata the upstream fixtures SURVEY.md §4 names are added as cases: cv/optflow/RubberWhale1.png / 2.png
(opencv_extra) and gpu/opticalflow/{frame0,frame1}.png with the stored Brox golden opticalflow/brox_optical_flow.bin."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from denseflow_amd.synth import SynthClip  # noqa: E402  (numpy only)

# (width, height, seed, t0, t1): the seeds of tests/golden/make_golden.py and SURVEY.md §8d
CASES = [(64, 48, 3, 0, 1), (224, 224, 1, 0, 1), (224, 224, 1, 3, 1), (320, 200, 6, 0, 2), (1920, 1080, 2, 0, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--testdata", default=os.environ.get("OPENCV_TEST_DATA_PATH"))
    args = ap.parse_args()
    try:
        import cv2
    except ImportError:
        sys.exit("cv2 is not importable here: run this on a machine with OpenCV + opencv_contrib built WITH_CUDA")
    if not hasattr(cv2, "cuda") or cv2.cuda.getCudaEnabledDeviceCount() < 1:
        sys.exit("this OpenCV has no usable CUDA device: the reference's cv::cuda path cannot be evaluated")
    info = cv2.getBuildInformation()
    pairs = []
    for (w, h, seed, t0, t1) in CASES:
        clip = SynthClip(w, h, seed)
        pairs.append((f"synth_{w}x{h}_s{seed}_t{t0}_{t1}", clip.frame(t0), clip.frame(t1)))
    if args.testdata:
        for name, a, b in (("rubberwhale", "cv/optflow/RubberWhale1.png", "cv/optflow/RubberWhale2.png"),
                           ("gpu_frames", "gpu/opticalflow/frame0.png", "gpu/opticalflow/frame1.png")):
            fa, fb = (cv2.imread(os.path.join(args.testdata, p), cv2.IMREAD_GRAYSCALE) for p in (a, b))
            if fa is not None and fb is not None:
                pairs.append((name, fa, fb))

    def up(a):
        g = cv2.cuda_GpuMat()
        g.upload(a)
        return g

    algos = {
        "tvl1": lambda a, b: cv2.cuda_OpticalFlowDual_TVL1.create().calc(up(a), up(b), None).download(),
        "farn": lambda a, b: cv2.cuda_FarnebackOpticalFlow.create().calc(up(a), up(b), None).download(),
        # the Gaussian update window at a larger winSize, as OpenCV's documentation recommends it:
        # create(numLevels, pyrScale, fastPyramids, winSize, numIters, polyN, polySigma, flags)
        "farn_gaussian": lambda a, b: cv2.cuda_FarnebackOpticalFlow.create(
            5, 0.5, False, 15, 10, 5, 1.1, cv2.OPTFLOW_FARNEBACK_GAUSSIAN).calc(up(a), up(b), None).download(),
        # src/denseflow_gpu.cpp:303, :332-334: create(0.197f, 50.0f, 0.8f, 10, 77, 10) on frames scaled by 1/255
        "brox": lambda a, b: cv2.cuda_BroxOpticalFlow.create(0.197, 50.0, 0.8, 10, 77, 10).calc(
            up(a.astype(np.float32) * np.float32(1.0 / 255.0)), up(b.astype(np.float32) * np.float32(1.0 / 255.0)),
            None).download(),
    }
    os.makedirs(args.out, exist_ok=True)
    for algo, fn in algos.items():
        blob = {"build_information": np.array(info), "opencv_version": np.array(cv2.__version__)}
        for name, a, b in pairs:
            flow = fn(a, b)
            blob[name + "_f0"], blob[name + "_f1"], blob[name + "_flow"] = a, b, flow.astype(np.float32)
            print(algo, name, flow.shape, float(np.abs(flow).max()))
        np.savez_compressed(os.path.join(args.out, f"opencv_{algo}.npz"), **blob)
    # the illumination channel: create(tau, lambda, theta, nscales, warps, epsilon, iterations, scaleStep, gamma, useInitialFlow)
    blob = {"build_information": np.array(info), "opencv_version": np.array(cv2.__version__)}
    for name, a, b in pairs[:2]:
        blob[name + "_f0"], blob[name + "_f1"] = a, b
        for gamma in (0.4, 2.0):
            alg = cv2.cuda_OpticalFlowDual_TVL1.create(0.25, 0.15, 0.3, 5, 5, 0.01, 300, 0.8, gamma, False)
            flow = alg.calc(up(a), up(b), None).download()
            blob[f"{name}_gamma{gamma}_flow"] = flow.astype(np.float32)
            print("tvl1_gamma", gamma, name, flow.shape, float(np.abs(flow).max()))
    np.savez_compressed(os.path.join(args.out, "opencv_tvl1_gamma.npz"), **blob)
    # caller-supplied initial flows: the flow argument of calc is read as the seed (and overwritten with the result)
    seeded = {
        "tvl1": lambda: cv2.cuda_OpticalFlowDual_TVL1.create(0.25, 0.15, 0.3, 5, 5, 0.01, 300, 0.8, 0.0, True),
        "farn": lambda: cv2.cuda_FarnebackOpticalFlow.create(5, 0.5, False, 13, 10, 5, 1.1, cv2.OPTFLOW_USE_INITIAL_FLOW),
    }
    for algo, make in seeded.items():
        blob = {"build_information": np.array(info), "opencv_version": np.array(cv2.__version__)}
        for name, a, b in pairs[:2]:
            seed = (algos[algo](a, b).astype(np.float32) * np.float32(0.5)).astype(np.float32)
            flow = make().calc(up(a), up(b), up(seed.copy())).download()
            blob[name + "_f0"], blob[name + "_f1"] = a, b
            blob[name + "_seed"], blob[name + "_flow"] = seed, flow.astype(np.float32)
            print(algo + "_init", name, flow.shape, float(np.abs(flow).max()))
        np.savez_compressed(os.path.join(args.out, f"opencv_{algo}_init.npz"), **blob)
    # fastPyramids: pyrDown frame pyramids, pyrUp flows; only sizes whose levels below the coarsest are even both ways
    def fast_ok(w, h, levels):
        k, scale = 0, 1.0
        while k < levels and w * scale * 0.5 >= 32 and h * scale * 0.5 >= 32:  # numLevelsCropped
            scale *= 0.5
            k += 1
        for _ in range(k):
            if w & 1 or h & 1:
                return False
            w, h = (w + 1) // 2, (h + 1) // 2
        return True

    blob = {"build_information": np.array(info), "opencv_version": np.array(cv2.__version__)}
    for name, a, b in pairs[:2]:
        if not fast_ok(a.shape[1], a.shape[0], 3):
            continue
        flow = cv2.cuda_FarnebackOpticalFlow.create(3, 0.5, True, 13, 10, 5, 1.1, 0).calc(up(a), up(b), None).download()
        blob[name + "_f0"], blob[name + "_f1"], blob[name + "_flow"] = a, b, flow.astype(np.float32)
        print("farn_fast_pyramids", name, flow.shape, float(np.abs(flow).max()))
    np.savez_compressed(os.path.join(args.out, "opencv_farn_fast_pyramids.npz"), **blob)
    if hasattr(cv2, "optflow") and hasattr(cv2.optflow, "DualTVL1OpticalFlow_create"):  # the CPU comparator
        blob = {"build_information": np.array(info), "opencv_version": np.array(cv2.__version__)}
        for name, a, b in pairs[:3]:
            blob[name + "_f0"], blob[name + "_f1"] = a, b
            blob[name + "_flow"] = cv2.optflow.DualTVL1OpticalFlow_create().calc(a, b, None).astype(np.float32)
        np.savez_compressed(os.path.join(args.out, "opencv_cpu_tvl1.npz"), **blob)
    if args.testdata:
        p = os.path.join(args.testdata, "gpu/opticalflow/brox_optical_flow.bin")
        if os.path.exists(p):
            print("upstream Brox golden present:", p, "(compare with opencv_brox.npz['gpu_frames_flow'])")


if __name__ == "__main__":
    main()
