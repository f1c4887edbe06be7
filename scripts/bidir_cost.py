#!/usr/bin/env python3
"""What the bidirectional call costs at 1080p (profiles/bidir/README.md, raw lines profiles/bidir/cost_1080p.jsonl): the bench clip (SynthClip(1920, 1080, seed=2), 300
frames resident = 299 pairs of adjacent frames) for TVL1 and Farneback through

  (a) two planar device calls, step = 1 then step = -1 (what a caller did before: every frame built twice);
  (b) one dfx_calc_batch_bidir_device call without the check;
  (c) the same with both masks;

alternating a, b, c for --rounds rounds behind one warm round, a fresh handle per algorithm.  Per call form: the host time
around the call(s) (they return with the device idle) and dfx_stats.device_ms (HIP events around every device batch on the
compute stream), median and spread (max - min) over the rounds.

The check kernel's time comes from those HIP events: per round, device_ms of (c) minus device_ms of (b) is the time of the
k_fb_check launches — one per device batch, both directions, 2 x 299 flows — and nothing else; it is set against the byte
model, per pixel and direction 8 B of F, 8 .. 32 B of B taps, 1 B of mask.  dfx_fb_check_device alone (299 flows, with and
without err planes) is timed with the host clock around the synchronous call: that figure INCLUDES the launch and the stream
synchronisation, and is labelled so.  Also printed: TVL1's inner iterations of (a) and (b), which must be equal (the
bidirectional call hands the engine the same two batches).  One JSON line per row on stdout."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denseflow_amd as dfx  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402

W, H = 1920, 1080


def timed(eng, fn):
    eng.reset_stats()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    dt = time.perf_counter() - t
    st = eng.stats()
    return dict(host_ms=dt * 1e3, device_ms=st.device_ms, pairs=int(st.pairs), iters=int(st.tvl1_total_iters),
                launches=int(st.kernel_launches))


def summary(rows, key):
    v = sorted(r[key] for r in rows)
    return dict(median=v[len(v) // 2], spread=v[-1] - v[0], runs=[round(x, 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--algos", default="tvl1,farn")
    args = ap.parse_args()
    n, m = args.frames, args.frames - 1
    frames = SynthClip(W, H, 2).frames_torch(n, "cuda")
    fwd = torch.empty((m, 2, H, W), dtype=torch.float32, device="cuda")
    bwd = torch.empty_like(fwd)
    occ_f = torch.empty((m, H, W), dtype=torch.uint8, device="cuda")
    occ_b = torch.empty_like(occ_f)
    hw = H * W
    for algo in args.algos.split(","):
        with dfx.FlowEngine(W, H, algo) as eng:
            def two_calls():
                eng.calc_optflows_planar_device(frames.data_ptr(), W, hw, n, 1, None, fwd.data_ptr(), W, hw, 2 * hw)
                eng.calc_optflows_planar_device(frames.data_ptr(), W, hw, n, -1, None, bwd.data_ptr(), W, hw, 2 * hw)

            def bidir(check):
                eng.calc_optflows_bidir_device(frames.data_ptr(), W, hw, n, 1, fwd.data_ptr(), bwd.data_ptr(), W, hw, 2 * hw,
                                               0.01, 0.5, occ_f.data_ptr() if check else None,
                                               occ_b.data_ptr() if check else None, W, hw)

            forms = [("two_planar_calls", two_calls), ("bidir_no_check", lambda: bidir(False)),
                     ("bidir_with_masks", lambda: bidir(True))]
            rows = {name: [] for name, _ in forms}
            for r in range(args.rounds + 1):
                for name, fn in forms:
                    res = timed(eng, fn)
                    if r:  # round 0 warms every form
                        rows[name].append(res)
            for name, _ in forms:
                last = rows[name][-1]
                print(json.dumps(dict(algo=algo, form=name, flows=2 * m, batch=int(eng.stats().batch),
                                      host_ms=summary(rows[name], "host_ms"), device_ms=summary(rows[name], "device_ms"),
                                      flows_per_s=2 * m / (summary(rows[name], "host_ms")["median"] * 1e-3),
                                      pairs_counted=last["pairs"], tvl1_total_iters=last["iters"],
                                      kernel_launches=last["launches"])), flush=True)
            # k_fb_check by HIP events: the same call with and without the masks, round by round
            diff = sorted(c["device_ms"] - b["device_ms"] for b, c in zip(rows["bidir_no_check"], rows["bidir_with_masks"]))
            med = diff[len(diff) // 2]
            lo, hi = 2 * m * hw * (8 + 8 + 1), 2 * m * hw * (8 + 32 + 1)
            print(json.dumps(dict(algo=algo, form="k_fb_check_by_events", flows=2 * m, launches=-(-m // int(eng.stats().batch)),
                                  ms=dict(median=med, spread=diff[-1] - diff[0], runs=[round(x, 3) for x in diff]),
                                  us_per_pair_both_directions=med * 1e3 / m, model_bytes=[lo, hi],
                                  model_tb_per_s=[lo / (med * 1e-3) / 1e12, hi / (med * 1e-3) / 1e12])), flush=True)
            # the check alone, on the flows the last round left in fwd / bwd: host clock, launch and synchronisation included
            err = torch.empty((m, H, W), dtype=torch.float32, device="cuda")
            for want_err in (False, True):
                ts = []
                for r in range(args.rounds + 1):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    eng.fb_check_device(fwd.data_ptr(), bwd.data_ptr(), W, hw, 2 * hw, m, 0.01, 0.5, occ_f.data_ptr(), W, hw,
                                        err.data_ptr() if want_err else None, W, hw)
                    if r:
                        ts.append((time.perf_counter() - t) * 1e3)
                ts.sort()
                med = ts[len(ts) // 2]
                out_b = 5 if want_err else 1
                lo, hi = m * hw * (8 + 8 + out_b), m * hw * (8 + 32 + out_b)
                print(json.dumps(dict(algo=algo, form="fb_check_device" + ("_err" if want_err else "") + "_host_clock_incl_launch_and_sync", flows=m,
                                      ms=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                                      us_per_flow=med * 1e3 / m, model_bytes=[lo, hi],
                                      model_tb_per_s=[lo / (med * 1e-3) / 1e12, hi / (med * 1e-3) / 1e12],
                                      occluded_share=float(occ_f.sum(dtype=torch.int64)) / occ_f.numel())), flush=True)
            del err


if __name__ == "__main__":
    main()
