#!/usr/bin/env python3
"""What the backward warp costs at 1080p (profiles/warp/README.md, raw lines profiles/warp/rate_1080p.jsonl): 64 images resident
in device memory — frames 1 .. 64 of the bench clip SynthClip(1920, 1080, seed=2), the references frames 0 .. 63 — warped by

  flows "farn": the library's own Farneback flows of those 64 pairs (small real motion: neighbouring pixels share taps);
  flows "wide": smooth random flows of up to a quarter of the frame (the taps of a wave spread over many rows),

through dfx_warp_device in each image kind (gray, interleaved BGR, planar BGR), output type and combination of outputs named
below.  Per form: --calls synchronous calls back to back inside one host-clock window (each call returns with the device idle,
so the figure INCLUDES one launch and one stream synchronisation per call), --rounds windows behind one warm window, the forms
alternating round by round; median and spread (max - min) over the rounds, microseconds per image, and the byte model — per
pixel 8 B of flow, C .. 4 C B of taps (perfectly cached .. every tap its own access), C x elem B of output, + C B of reference
with the statistics, + 1 B of occlusion mask, + 1 B of valid mask — as a pair of rates.  The last rows are the same quantity
(the masked mean absolute error of the gray images) through torch alone: float conversion, a sampling grid, grid_sample, an
absolute difference, a mask and a reduction.  One JSON line per row on stdout."""
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
ELEM = {torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4}


def wide_flows(n, seed=7):
    g = torch.Generator(device="cpu").manual_seed(seed)
    grid = torch.rand((n, 2, H // 64 + 2, W // 64 + 2), generator=g) * 2 - 1
    f = torch.nn.functional.interpolate(grid, size=(H, W), mode="bilinear", align_corners=True)
    f[:, 0] *= 0.25 * W
    f[:, 1] *= 0.25 * H
    return f.contiguous().cuda()


def torch_masked_error(src, ref, flows, occ):
    """mean |ref - warp(src, flows)| over the pixels whose target stays inside and that occ does not mask: torch alone."""
    n = src.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    px, py = xs + flows[:, 0], ys + flows[:, 1]
    inside = (px >= 0) & (py >= 0) & (px <= W - 1) & (py <= H - 1) & (occ == 0)
    grid = torch.stack([px * (2.0 / (W - 1)) - 1, py * (2.0 / (H - 1)) - 1], -1)
    warped = torch.nn.functional.grid_sample(src.float().unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    diff = (ref.float() - warped.squeeze(1).round()).abs() * inside
    return diff.reshape(n, -1).sum(1) / inside.reshape(n, -1).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, hw = args.images, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flow_sets = {"farn": eng.flow_tensor(frames, 1), "wide": wide_flows(n)}
        gray_src, gray_ref = frames[1:], frames[:-1]
        bgr = torch.stack([frames, frames.flip(1), frames.flip(2)], -1)  # (n + 1, H, W, 3): three unlike channels
        images = {"gray": (gray_src, gray_ref), "bgr": (bgr[1:], bgr[:-1]),
                  "planar": (bgr[1:].permute(0, 3, 1, 2).contiguous(), bgr[:-1].permute(0, 3, 1, 2).contiguous())}
        occ = (torch.rand((n, H, W), device="cuda") < 0.1).to(torch.uint8)
        # (image kind, output type or None for no warped image, occ, valid, stats)
        forms = [("gray", torch.uint8, False, False, False), ("gray", torch.uint8, True, True, True),
                 ("gray", None, True, False, True), ("gray", torch.float32, False, False, False),
                 ("bgr", torch.uint8, False, False, False), ("bgr", torch.float16, False, False, False),
                 ("bgr", torch.float32, False, False, False), ("bgr", torch.uint8, True, True, True),
                 ("bgr", None, True, False, True),
                 ("planar", torch.uint8, False, False, False), ("planar", torch.float16, False, False, False),
                 ("planar", torch.uint8, True, True, True), ("planar", None, True, False, True)]
        outs = {}
        for kind, dt, *_ in forms:
            if dt is not None and (kind, dt) not in outs:
                outs[kind, dt] = torch.empty(images[kind][0].shape, dtype=dt, device="cuda")
        valid = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        stats = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        codes = {torch.uint8: 3, torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

        def call(kind, dt, with_occ, want_valid, want_stats, flows):
            src, ref = images[kind]
            ch = 1 if kind == "gray" else 3
            pitch, plane = (3 * W, 0) if kind == "bgr" else (W, hw)
            out = outs[kind, dt] if dt is not None else None
            eng.warp_device(src.data_ptr(), ch, 1 if kind == "planar" else 0, pitch, plane, ch * hw, flows.data_ptr(), W, hw,
                            2 * hw, n, 0, codes[dt] if dt is not None else 3, out.data_ptr() if dt is not None else None,
                            pitch, plane, ch * hw, ref.data_ptr(), occ.data_ptr() if with_occ else None, W, hw,
                            valid.data_ptr() if want_valid else None, W, hw, stats.data_ptr() if want_stats else None)

        for fname, flows in flow_sets.items():
            times = {f: [] for f in forms}
            for r in range(args.rounds + 1):
                for f in forms:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.calls):
                        call(*f, flows)
                    dt_ms = (time.perf_counter() - t) * 1e3 / args.calls
                    if r:  # round 0 warms every form
                        times[f].append(dt_ms)
            inside = None
            for f in forms:
                kind, dt, with_occ, want_valid, want_stats = f
                ch = 1 if kind == "gray" else 3
                fixed = 8 + (ch * ELEM[dt] if dt is not None else 0) + (ch if want_stats else 0) + int(with_occ) + int(want_valid)
                ts = sorted(times[f])
                med = ts[len(ts) // 2]
                lo, hi = n * hw * (fixed + ch), n * hw * (fixed + 4 * ch)
                row = dict(flows=fname, kind=kind, out=str(dt).replace("torch.", "") if dt is not None else None, occ=with_occ,
                           valid=want_valid, stats=want_stats, images=n, calls_per_window=args.calls,
                           ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                           us_per_image=med * 1e3 / n, model_bytes=[lo, hi],
                           model_tb_per_s=[lo / (med * 1e-3) / 1e12, hi / (med * 1e-3) / 1e12])
                if want_stats:
                    call(*f, flows)
                    st = stats.cpu().numpy().astype("float64")
                    row["valid_share"] = float(st[:, 0].sum() / (n * hw))
                    row["mean_abs_error"] = float(st[:, 1].sum() / (st[:, 0].sum() * ch))
                print(json.dumps(row), flush=True)
            # the same figure through torch alone (gray, masked): every pass a kernel of its own
            ts = []
            for r in range(args.rounds + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                err = torch_masked_error(gray_src, gray_ref, flows, occ)
                torch.cuda.synchronize()
                if r:
                    ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            call("gray", None, True, False, True, flows)
            st = stats.cpu().numpy().astype("float64")
            print(json.dumps(dict(flows=fname, kind="gray", form="torch_grid_sample_masked_error", images=n,
                                  ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_image=ts[len(ts) // 2] * 1e3 / n,
                                  mean_abs_error_torch=float(err.double().mean()),
                                  mean_abs_error_device_per_image_mean=float((st[:, 1] / st[:, 0]).mean()))), flush=True)
            del err


if __name__ == "__main__":
    main()
