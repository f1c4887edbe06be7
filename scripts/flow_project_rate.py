#!/usr/bin/env python3
"""What projecting flows forward costs at 1080p (profiles/flow_project/README.md, raw lines profiles/flow_project/*.jsonl):
64 flows resident in device memory — the library's own Farneback flows of adjacent frames 0 .. 64 of the bench clip
SynthClip(1920, 1080, seed=2), forward, with the forward occlusion masks of the bidirectional call for the masked form — and
smooth random flows of up to a quarter of the frame, through dfx_flow_project_device as the inverse (t = 1, scale = -1) with
no optional input, with an importance plane, with the masks, and with the coverage plane; out and hole always written; the
workspace holds --work-flows flows (all 64 by default: one wave of launches per call).  Per form: --calls synchronous calls
back to back inside one host-clock window (each call returns with the device idle, so the figure INCLUDES three launches and
one stream synchronisation per call), --rounds windows behind one warm window, the forms alternating round by round; median
and spread (max - min) over the windows, microseconds per flow; the adds of the straightforward scatter (12 of 8 bytes per
source pixel that lands in the frame) as bytes per second of the whole call; and the chip's copy rate measured in the same run
in the same way (a device-to-device copy of the 64 flows: 16 B per pixel).  Then the same projection through torch alone
(float index_add_ of the four taps, then a divide; 8 flows at a time) against the device's result, in pixels.  One JSON line
per row on stdout.  --label says which build of the library ran (DFX_LIBRARY chooses it)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denseflow_amd as dfx  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402

W, H = 1920, 1080
CHUNK = 8


def torch_project(flows, min_weight=0.25):
    """(out, hole) of the inverse by float sums: the bilinear footprint of every source added with index_add_, then a divide."""
    n = flows.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=flows.device, dtype=torch.float32),
                            torch.arange(W, device=flows.device, dtype=torch.float32), indexing="ij")
    out = torch.empty_like(flows)
    hole = torch.empty((n, H, W), dtype=torch.bool, device=flows.device)
    for i0 in range(0, n, CHUNK):
        f = flows[i0:i0 + CHUNK]
        m = f.shape[0]
        px, py = xs + f[:, 0], ys + f[:, 1]
        x0, y0 = px.floor(), py.floor()
        ax, ay = px - x0, py - y0
        acc = torch.zeros((3, m * H * W), device=flows.device)
        base = (torch.arange(m, device=flows.device) * (H * W)).view(m, 1, 1)
        for dy in (0, 1):
            for dx in (0, 1):
                tx, ty = x0 + dx, y0 + dy
                wgt = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
                ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                at = (base + ty.clamp(0, H - 1).long() * W + tx.clamp(0, W - 1).long())[ok]
                wv = wgt[ok]
                acc[0].index_add_(0, at, wv)
                acc[1].index_add_(0, at, wv * f[:, 0][ok])
                acc[2].index_add_(0, at, wv * f[:, 1][ok])
        acc = acc.view(3, m, H, W)
        hl = acc[0] < min_weight
        hole[i0:i0 + m] = hl
        den = torch.where(hl, torch.ones_like(acc[0]), acc[0])
        out[i0:i0 + m, 0] = torch.where(hl, torch.zeros_like(den), -acc[1] / den)
        out[i0:i0 + m, 1] = torch.where(hl, torch.zeros_like(den), -acc[2] / den)
    return out, hole


def smooth_random_flows(n, mag_x, mag_y):
    g = torch.Generator(device="cuda").manual_seed(490)
    coarse = torch.rand((n, 2, H // 120 + 1, W // 120 + 1), device="cuda", generator=g) * 2 - 1
    f = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    f[:, 0] *= mag_x
    f[:, 1] *= mag_y
    return f.contiguous()


def window(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / calls


def landing_share(f):
    ys, xs = torch.meshgrid(torch.arange(H, device=f.device, dtype=torch.float32),
                            torch.arange(W, device=f.device, dtype=torch.float32), indexing="ij")
    px, py = xs + f[:, 0], ys + f[:, 1]
    return float(((px > -1) & (px < W) & (py > -1) & (py < H)).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--work-flows", type=int, default=0, help="flows the workspace holds (0: all)")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="", help="copied into every row (which build of the library this is)")
    ap.add_argument("--no-torch", action="store_true", help="skip the comparison with torch alone")
    args = ap.parse_args()
    n, hw = args.flows, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flows, _, occ, _ = eng.flow_tensor_bidir(frames, 1)
        del frames
        wild = smooth_random_flows(n, W / 4, H / 4)
        g = torch.Generator(device="cuda").manual_seed(491)
        imp = torch.exp(torch.rand((n, H, W), device="cuda", generator=g) * 3 - 2)
        out = torch.empty((n, 2, H, W), device="cuda")
        hole = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        cov = torch.empty((n, H, W), device="cuda")
        copy = torch.empty_like(flows)
        wf = args.work_flows or n
        per = eng.flow_project_work_bytes()
        work = torch.empty((per * wf // 8,), dtype=torch.int64, device="cuda")
        forms = [(src, opt) for src in ("farneback", "smooth_random_quarter_frame") for opt in ("plain", "importance", "occ", "coverage")]

        def call(src, opt):
            eng.flow_project_device((flows if src == "farneback" else wild).data_ptr(), W, hw, 2 * hw, n, work.data_ptr(),
                                    per * wf, 1.0, -1.0, 0.25, out.data_ptr(), W, hw, 2 * hw, hole.data_ptr(), W, hw,
                                    cov.data_ptr() if opt == "coverage" else None, W, hw,
                                    imp.data_ptr() if opt == "importance" else None, W, hw,
                                    occ.data_ptr() if opt == "occ" else None, W, hw)

        times = {f: [] for f in forms}
        copies = []
        for r in range(args.rounds + 1):
            for f in forms:
                dt_ms = window(lambda: call(*f), args.calls)
                if r:  # round 0 warms every form
                    times[f].append(dt_ms)
            dt_ms = window(lambda: (copy.copy_(flows), torch.cuda.synchronize()), args.calls)
            if r:
                copies.append(dt_ms)
        copies.sort()
        copy_ms = copies[len(copies) // 2]
        copy_tb = n * hw * 16 / (copy_ms * 1e-3) / 1e12
        print(json.dumps(dict(label=args.label, form="device_to_device_copy_of_the_flows", flows=n, calls_per_window=args.calls,
                              ms_per_call=dict(median=copy_ms, spread=copies[-1] - copies[0], runs=[round(x, 4) for x in copies]),
                              us_per_flow=copy_ms * 1e3 / n, model_bytes=n * hw * 16, model_tb_per_s=copy_tb)), flush=True)
        share = {"farneback": landing_share(flows), "smooth_random_quarter_frame": landing_share(wild)}
        for f in forms:
            src, opt = f
            ts = sorted(times[f])
            med = ts[len(ts) // 2]
            call(*f)
            atomic_bytes = 96.0 * share[src] * n * hw
            print(json.dumps(dict(label=args.label, flows_from=src, optional=opt, flows=n, work_flows=wf, calls_per_window=args.calls,
                                  ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_flow=med * 1e3 / n, share_of_sources_landing_in_the_frame=share[src],
                                  plain_form_atomic_bytes=atomic_bytes, plain_form_atomic_tb_per_s_of_the_call=atomic_bytes / (med * 1e-3) / 1e12,
                                  us_per_flow_of_the_copy=copy_ms * 1e3 / n, hole_share=float(hole.float().mean()))), flush=True)
        if args.no_torch:
            return
        for src in ("farneback", "smooth_random_quarter_frame"):
            src_flows = flows if src == "farneback" else wild
            ts = []
            for r in range(min(args.rounds, 3) + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res, rhole = torch_project(src_flows)
                torch.cuda.synchronize()
                if r:
                    ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            call(src, "plain")
            both = ~rhole & (hole == 0)
            diff = (res - out).abs().amax(1)
            print(json.dumps(dict(label=args.label, form="torch_index_add_projection", flows_from=src, flows=n,
                                  ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                                  us_per_flow=ts[len(ts) // 2] * 1e3 / n,
                                  max_abs_difference_where_neither_is_a_hole_px=float(diff[both].max()),
                                  median_abs_difference_px=float(diff[both][::97].median()),
                                  hole_planes_agree_share=float((rhole == (hole != 0)).float().mean()),
                                  largest_flow_px=float(src_flows.abs().max()))), flush=True)
            del res, rhole, diff, both


if __name__ == "__main__":
    main()
