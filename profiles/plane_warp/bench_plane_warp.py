#!/usr/bin/env python3
"""What the backward warp of typed planes costs at 1080p (profiles/plane_warp/README.md, raw lines rate_1080p.jsonl), with the
method of scripts/warp_rate.py: sources resident in device memory, warped by

  flows "farn": the library's own Farneback flows of adjacent frames of the bench clip SynthClip(1920, 1080, seed=2);
  flows "wide": smooth random flows of up to a quarter of the frame (the taps of a wave spread over many rows),

through dfx_warp_planes_device in the forms named below, next to dfx_warp_device (float32 out) on the same pictures, the same
result through torch alone (a normalised grid from the planar flows, grid_sample(align_corners=True), NCHW and channels_last)
and a plain device copy of the same buffer.  Per form: --calls synchronous calls back to back inside one host-clock window
(each call returns with the device idle, so the figure INCLUDES one launch and one stream synchronisation per call), --rounds
windows behind one warm window, the forms alternating round by round; median and spread (max - min) over the rounds,
microseconds per image, and the byte model — per pixel 8 B of flow, C x elem x (1 .. 4) B of taps (perfectly cached .. every
tap its own access), C x elem B of out, + 1 B of occlusion mask, + 1 B of valid mask — as a pair of rates.  The image count
shrinks with the channel count (64 images up to C = 3, 16 at C = 16, 4 at C = 64) so that every form moves a few GB per call
and the largest holds 4.2 GB.  One JSON line per row on stdout."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import denseflow_amd as dfx  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402

W, H = 1920, 1080
HW = W * H
ELEM = {torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4}
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2, torch.uint8: 3}


def wide_flows(n, seed=7):
    g = torch.Generator(device="cpu").manual_seed(seed)
    grid = torch.rand((n, 2, H // 64 + 2, W // 64 + 2), generator=g) * 2 - 1
    f = torch.nn.functional.interpolate(grid, size=(H, W), mode="bilinear", align_corners=True)
    f[:, 0] *= 0.25 * W
    f[:, 1] *= 0.25 * H
    return f.contiguous().cuda()


def torch_warp(src, flows):
    """The same sampling through torch alone: src (n, C, H, W) in either memory format, flows (n, 2, H, W)."""
    ys, xs = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    grid = torch.stack([(xs + flows[:, 0]) * (2.0 / (W - 1)) - 1, (ys + flows[:, 1]) * (2.0 / (H - 1)) - 1], -1)
    return torch.nn.functional.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    images_of = {1: 64, 3: 64, 16: 16, 64: 4}
    frames = SynthClip(W, H, 2).frames_torch(65, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flow_sets = {"farn": eng.flow_tensor(frames, 1), "wide": wide_flows(64)}
        bgr = torch.stack([frames, frames.flip(1), frames.flip(2)], 1)[1:].contiguous()  # (64, 3, H, W) uint8: three unlike channels
        gray = frames[1:].contiguous()
        gen = torch.Generator(device="cuda").manual_seed(3)
        src = {}  # (C, dtype) -> channels-first planes; the channels-last copy is made per form
        src[1, torch.float32], src[3, torch.float32] = gray.float()[:, None].contiguous(), bgr.float()
        for c in (16, 64):
            src[c, torch.float32] = torch.randn((images_of[c], c, H, W), generator=gen, device="cuda")
            src[c, torch.float16] = src[c, torch.float32].half()
        src[1, torch.uint8] = gray[:, None].contiguous()
        occ = (torch.rand((64, H, W), device="cuda") < 0.1).to(torch.uint8)
        valid = torch.empty((64, H, W), dtype=torch.uint8, device="cuda")
        # (name, C, channels-last, source dtype, out dtype, nearest, keep, occ, valid); "warp" rows are dfx_warp_device
        forms = [("warp_device", 1, False, torch.uint8, torch.float32, False, False, False, False),
                 ("warp_device", 3, False, torch.uint8, torch.float32, False, False, False, False),
                 ("planes", 1, False, torch.float32, torch.float32, False, False, False, False),
                 ("planes", 3, False, torch.float32, torch.float32, False, False, False, False),
                 ("planes", 3, True, torch.float32, torch.float32, False, False, False, False)]
        for c in (16, 64):
            for dt in (torch.float32, torch.float16):
                forms += [("planes", c, il, dt, dt, False, False, False, False) for il in (False, True)]
        forms += [("planes", 1, False, torch.uint8, torch.uint8, True, False, False, False),
                  ("planes", 16, False, torch.float32, torch.float32, False, False, True, True),
                  ("planes", 16, False, torch.float32, torch.float32, False, True, True, True),
                  ("planes", 16, True, torch.float32, torch.float32, False, False, True, True),
                  ("planes", 16, True, torch.float32, torch.float32, False, True, True, True),
                  ("planes", 16, False, torch.float32, torch.bfloat16, False, False, False, False),
                  ("torch_grid_sample", 16, False, torch.float32, torch.float32, False, False, False, False),
                  ("torch_grid_sample", 16, True, torch.float32, torch.float32, False, False, False, False),
                  ("copy", 16, False, torch.float32, torch.float32, False, False, False, False)]
        last, outs = {}, {}

        def buffers(f):
            name, c, il, sdt, odt = f[:5]
            key = (name == "warp_device", c, il, sdt)
            if key not in last:
                s = (gray if c == 1 else bgr) if name == "warp_device" else src[c, sdt]
                last[key] = s.contiguous(memory_format=torch.channels_last) if il else s
            s = last[key]
            if (key, odt) not in outs:
                outs[key, odt] = torch.zeros_like(s, dtype=odt)
            return s, outs[key, odt]

        def call(f, flows):
            name, c, il, sdt, odt, near, keep, with_occ, want_valid = f
            s, out = buffers(f)
            n = s.shape[0]
            fl = flows[:n]
            if name == "copy":
                out.copy_(s)
                torch.cuda.synchronize()
            elif name == "torch_grid_sample":
                outs["torch", il] = torch_warp(s, fl)
                torch.cuda.synchronize()
            elif name == "warp_device":
                eng.warp_device(s.data_ptr(), c, 1 if c == 3 else 0, W, HW, c * HW, fl.data_ptr(), W, HW, 2 * HW, n, 0, 0,
                                out.data_ptr(), W, HW, c * HW)
            else:
                pitch, plane = (c * W, 0) if il else (W, HW if c > 1 else 0)
                eng.warp_planes_device(s.data_ptr(), CODE[sdt], c, 0 if il else 1, pitch, plane, c * HW, fl.data_ptr(), W, HW, 2 * HW,
                                       n, 0, int(near), int(keep), CODE[odt], out.data_ptr(), pitch, plane, c * HW,
                                       occ.data_ptr() if with_occ else None, W, HW, valid.data_ptr() if want_valid else None, W, HW)

        for fname, flows in flow_sets.items():
            times = {f: [] for f in forms}
            for r in range(args.rounds + 1):
                for f in forms:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(args.calls):
                        call(f, flows)
                    dt_ms = (time.perf_counter() - t) * 1e3 / args.calls
                    if r:  # round 0 warms every form
                        times[f].append(dt_ms)
            for f in forms:
                name, c, il, sdt, odt, near, keep, with_occ, want_valid = f
                n = buffers(f)[0].shape[0]
                ts = sorted(times[f])
                med = ts[len(ts) // 2]
                taps = c * ELEM[sdt]
                fixed = 8 + c * ELEM[odt] + int(with_occ) + int(want_valid)
                lo, hi = n * HW * (fixed + taps), n * HW * (fixed + (1 if near else 4) * taps)
                if name == "copy":
                    lo = hi = 2 * n * HW * c * 4
                row = dict(flows=fname, form=name, channels=c, layout="hwc" if il else "chw", src=str(sdt).replace("torch.", ""),
                           out=str(odt).replace("torch.", ""), sample="nearest" if near else "bilinear", invalid="keep" if keep else "zero",
                           occ=with_occ, valid=want_valid, images=n, calls_per_window=args.calls,
                           ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                           us_per_image=med * 1e3 / n, model_bytes=[lo, hi],
                           model_tb_per_s=[lo / (med * 1e-3) / 1e12, hi / (med * 1e-3) / 1e12])
                if name == "torch_grid_sample":  # its largest difference from the library's result on the same data
                    mine = ("planes", c, il, sdt, odt, False, False, False, False)
                    call(mine, flows)
                    call(f, flows)
                    diff = (outs["torch", il] - buffers(mine)[1]).abs()
                    row["max_abs_diff_from_library"] = float(diff.max())
                    # ... and over the pixels whose four taps all lie in the frame: in the band of one pixel round it
                    # grid_sample blends with its zero padding where the library's `inside` rule gives 0
                    fl = flows[:n]
                    px = torch.arange(W, device="cuda", dtype=torch.float32) + fl[:, 0]
                    py = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] + fl[:, 1]
                    inner = ((px >= 0) & (py >= 0) & (px <= W - 1) & (py <= H - 1))[:, None].expand_as(diff)
                    row["max_abs_diff_inside"] = float(diff[inner].max())
                    row["inside_share"] = float(inner.float().mean())
                    row["max_abs_source"] = float(buffers(f)[0].abs().max())
                print(json.dumps(row), flush=True)
            outs.pop(("torch", False), None), outs.pop(("torch", True), None)


if __name__ == "__main__":
    main()
