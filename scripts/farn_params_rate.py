#!/usr/bin/env python3
"""Pairs per second of -a=farn at 1080p for parameter sets beyond the defaults: frames resident in HBM, flows written to
HBM (FlowEngine.calc_optflows_device, synchronous), one process, one GPU.  Every case keeps one engine; after a warm-up
call per case the cases are timed in turn, ROUNDS times over, so that a drift of the machine hits all of them alike.

    python scripts/farn_params_rate.py --cases defaults,win15,win15_hbm,win21,win21_hbm,poly7 --out rates.json
    DFX_LIBRARY=/path/to/another/libdfx.so python scripts/farn_params_rate.py --cases defaults   # A/B of two builds
    python scripts/farn_params_rate.py --cases win15,gauss15,gauss15_hbm        # the Gaussian update window (farn_window)

Prints one line per case and round and a JSON summary (min / median / max pairs/s per case)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import denseflow_amd as dfx  # noqa: E402
from denseflow_amd import engine as E  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402

CASES = {
    "defaults": dict(),
    "defaults_hbm": dict(variant=E.VAR_FARN_M_IN_HBM),
    "poly7": dict(farn_poly_n=7, farn_poly_sigma=1.5),
    "win15": dict(farn_win_size=15),
    "win15_hbm": dict(farn_win_size=15, variant=E.VAR_FARN_M_IN_HBM),
    "win21": dict(farn_win_size=21),
    "win21_hbm": dict(farn_win_size=21, variant=E.VAR_FARN_M_IN_HBM),
    "win7": dict(farn_win_size=7),
    "win7_hbm": dict(farn_win_size=7, variant=E.VAR_FARN_M_IN_HBM),
    "win31": dict(farn_win_size=31),
}
# the Gaussian update window (dfx_params.farn_window), on chip and with M in HBM: gauss7, gauss7_hbm, gauss13, ...
G = getattr(E, "FARN_WINDOW_GAUSSIAN", 1)
for _w in (7, 13, 15, 21, 31):
    CASES[f"gauss{_w}"] = dict(farn_win_size=_w, farn_window=G)
    CASES[f"gauss{_w}_hbm"] = dict(farn_win_size=_w, farn_window=G, variant=E.VAR_FARN_M_IN_HBM)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="defaults,win15,win15_hbm,win21,win21_hbm,poly7")
    ap.add_argument("--frames", type=int, default=130)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=1.5, help="least timed window per case and round")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it does not fall back")
    w, h, n = a.width, a.height, a.frames
    names = a.cases.split(",")
    clip = SynthClip(w, h, 2)
    d_frames = torch.from_numpy(np.stack(clip.frames(n))).cuda()
    d_flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engines = {name: dfx.FlowEngine(w, h, "farn", **CASES[name]) for name in names}

    def call(eng):
        eng.calc_optflows_device(d_frames.data_ptr(), w, w * h, n, 1, d_flows.data_ptr(), w * h * 2)

    sums = {}
    for name in names:  # warm-up: code objects, allocations, clocks; and a checksum that shows the cases computed something
        call(engines[name])
        call(engines[name])
        sums[name] = float(d_flows[0].abs().sum().item())
    rates = {name: [] for name in names}
    for r in range(a.rounds):
        for name in names:
            calls, t0 = 0, time.perf_counter()
            while calls < 3 or time.perf_counter() - t0 < a.seconds:
                call(engines[name])  # returns when the flows are in HBM
                calls += 1
            dt = time.perf_counter() - t0
            rates[name].append(calls * (n - 1) / dt)
            print(f"round {r} {name}: {rates[name][-1]:.1f} pairs/s ({calls} calls of {n - 1} pairs in {dt:.2f} s)", flush=True)
    summary = {
        "size": [w, h], "frames": n, "library": os.environ.get("DFX_LIBRARY", dfx.library_path()),
        "device": torch.cuda.get_device_name(0),
        "cases": {name: {"pairs_per_s": [round(x, 1) for x in rates[name]], "min": round(min(rates[name]), 1),
                         "median": round(statistics.median(rates[name]), 1), "max": round(max(rates[name]), 1),
                         "batch": engines[name].stats().batch, "device_bytes": engines[name].device_bytes(),
                         "abs_sum_flow0": sums[name]} for name in names},
    }
    for eng in engines.values():
        eng.close()
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
