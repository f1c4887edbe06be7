#!/usr/bin/env python3
"""Pairs per second of -a=farn at 1080p with dfx_params.farn_fast_pyramids 0 and 1: a 300-frame SynthClip resident in HBM,
flows written to HBM (FlowEngine.calc_optflows_device, synchronous), farn_num_levels 3 (the most 1920 x 1080 accepts with
fast pyramids), one process, one GPU.  One engine per flag; after two warm-up calls each the flags are timed in turn,
ROUNDS times over, so that a drift of the machine hits both alike.

    python scripts/farn_fast_pyramids_rate.py --out rates.json
    DFX_LIBRARY=/path/to/the/parent/libdfx.so python scripts/farn_fast_pyramids_rate.py --flags 0    # the parent commit's rate
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python scripts/farn_fast_pyramids_rate.py --flags 1 --calls 3

--calls N: no timing, N calls per flag after one warm-up call (the profiler's run).  The JSON line also holds the compulsory
traffic of the two fast-pyramid kernels per call (bytes every launch of them must move: each source and each destination
element once), to set against their kernel times."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denseflow_amd as dfx  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402


def compulsory_bytes(w, h, levels, n_frames, n_pairs, frames_per_call):
    """Per calc_optflows_device call: pyrDown reads a level once (1 B per pixel from the 8-bit frame for level 1, 4 B after
    that) and writes the next one, for every frame built; pyrUp reads two planes of a level and writes two of the next."""
    sizes = [(w, h)]
    for _ in range(levels):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    down_u8 = frames_per_call * (sizes[0][0] * sizes[0][1] + 4 * sizes[1][0] * sizes[1][1]) if levels >= 1 else 0
    down_f32 = frames_per_call * sum(4 * (sizes[k - 1][0] * sizes[k - 1][1] + sizes[k][0] * sizes[k][1]) for k in range(2, levels + 1))
    up = n_pairs * sum(8 * (sizes[k + 1][0] * sizes[k + 1][1] + sizes[k][0] * sizes[k][1]) for k in range(levels))
    return {"k_farn_pyrdown<u8>": down_u8, "k_farn_pyrdown<f32>": down_f32, "k_farn_pyrup_flow": up}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", default="0,1")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=2.0, help="least timed window per flag and round")
    ap.add_argument("--calls", type=int, default=0, help="profiler mode: this many untimed calls per flag")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures, it does not fall back")
    w, h, n = a.width, a.height, a.frames
    flags = [int(f) for f in a.flags.split(",")]
    d_frames = SynthClip(w, h, 9).frames_torch(n, "cuda").contiguous()
    d_flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    engines = {}
    for f in flags:
        kw = dict(farn_num_levels=a.levels)
        if f:  # a library built before the field (DFX_LIBRARY A/B) is only ever asked for flag 0
            kw["farn_fast_pyramids"] = f
        engines[f] = dfx.FlowEngine(w, h, "farn", **kw)

    def call(eng):
        eng.calc_optflows_device(d_frames.data_ptr(), w, w * h, n, 1, d_flows.data_ptr(), w * h * 2)

    sums, launches = {}, {}
    for f in flags:  # warm-up: code objects, allocations, clocks; and a checksum that shows the flags computed something
        call(engines[f])
        engines[f].reset_stats()
        call(engines[f])
        st = engines[f].stats()
        launches[f] = st.kernel_launches
        sums[f] = float(d_flows[0].abs().sum().item())
    rates = {f: [] for f in flags}
    if a.calls:
        for f in flags:
            for _ in range(a.calls):
                call(engines[f])
    else:
        for r in range(a.rounds):
            for f in flags:
                calls, t0 = 0, time.perf_counter()
                while calls < 2 or time.perf_counter() - t0 < a.seconds:
                    call(engines[f])  # returns when the flows are in HBM
                    calls += 1
                dt = time.perf_counter() - t0
                rates[f].append(calls * (n - 1) / dt)
                print(f"round {r} fast_pyramids={f}: {rates[f][-1]:.1f} pairs/s ({calls} calls of {n - 1} pairs in {dt:.2f} s)", flush=True)
    batch = engines[flags[0]].stats().batch
    summary = {
        "size": [w, h], "frames": n, "levels": a.levels, "library": os.environ.get("DFX_LIBRARY", dfx.library_path()),
        "device": torch.cuda.get_device_name(0), "batch": batch,
        "compulsory_bytes_per_call": compulsory_bytes(w, h, a.levels, n, n - 1, n + (n - 2) // max(batch, 1)),
        "flags": {str(f): {"pairs_per_s": [round(x, 1) for x in rates[f]],
                           "min": round(min(rates[f]), 1) if rates[f] else None,
                           "median": round(statistics.median(rates[f]), 1) if rates[f] else None,
                           "max": round(max(rates[f]), 1) if rates[f] else None,
                           "kernel_launches_per_call": launches[f], "device_bytes": engines[f].device_bytes(),
                           "abs_sum_flow0": sums[f]} for f in flags},
    }
    for eng in engines.values():
        eng.close()
    line = json.dumps(summary)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
