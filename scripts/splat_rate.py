#!/usr/bin/env python3
"""What carrying images forward along flows costs at 1080p (profiles/splat/README.md, raw lines profiles/splat/*.jsonl): 64
images resident in device memory — frames 0 .. 63 of the bench clip SynthClip(1920, 1080, seed=2) as gray bytes, as BGR bytes
interleaved and planar (the gray frame and two shifted copies), and as float32 payload planes — with the library's own forward
Farneback flows of adjacent frames (and the forward occlusion masks of the bidirectional call for the masked form), and with
smooth random flows of up to a quarter of the frame, through dfx_splat_device at t = 1; the workspace holds all 64 images (one
wave of launches per call).  Per form: --calls synchronous calls back to back inside one host-clock window (each call returns
with the device idle, so the figure INCLUDES three launches and one stream synchronisation per call), --rounds windows behind
one warm window, the forms alternating round by round — dfx_flow_project_device on the same flows among them, the yardstick;
median and spread (max - min) over the windows, microseconds per image and per 64-bit word of the workspace's pixel (the
projection has 3, the splat 1 + C).  Then the same splat through torch alone (float index_add_ of the four taps per channel, then
a divide; 8 images at a time) against the device's float32 result.  One JSON line per row on stdout.  --label says which build
of the library ran (DFX_LIBRARY chooses it)."""
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
U8, F32 = 3, 0  # DFX_WARP_U8, DFX_PLANAR_F32


def torch_splat(images, flows, min_weight=0.25):
    """(out, hole) of the mean splat by float sums: the bilinear footprint of every source added with index_add_ per channel,
    then a divide.  images (n, C, H, W) float32."""
    n, c = images.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, device=flows.device, dtype=torch.float32),
                            torch.arange(W, device=flows.device, dtype=torch.float32), indexing="ij")
    out = torch.empty_like(images)
    hole = torch.empty((n, H, W), dtype=torch.bool, device=flows.device)
    for i0 in range(0, n, CHUNK):
        f, img = flows[i0:i0 + CHUNK], images[i0:i0 + CHUNK]
        m = f.shape[0]
        px, py = xs + f[:, 0], ys + f[:, 1]
        x0, y0 = px.floor(), py.floor()
        ax, ay = px - x0, py - y0
        acc = torch.zeros((1 + c, m * H * W), device=flows.device)
        base = (torch.arange(m, device=flows.device) * (H * W)).view(m, 1, 1)
        for dy in (0, 1):
            for dx in (0, 1):
                tx, ty = x0 + dx, y0 + dy
                wgt = (ax if dx else 1 - ax) * (ay if dy else 1 - ay)
                ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                at = (base + ty.clamp(0, H - 1).long() * W + tx.clamp(0, W - 1).long())[ok]
                wv = wgt[ok]
                acc[0].index_add_(0, at, wv)
                for k in range(c):
                    acc[1 + k].index_add_(0, at, wv * img[:, k][ok])
        acc = acc.view(1 + c, m, H, W)
        hl = acc[0] < min_weight
        hole[i0:i0 + m] = hl
        den = torch.where(hl, torch.ones_like(acc[0]), acc[0])
        for k in range(c):
            out[i0:i0 + m, k] = torch.where(hl, torch.zeros_like(den), acc[1 + k] / den)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every row (which build of the library this is)")
    ap.add_argument("--no-torch", action="store_true", help="skip the comparison with torch alone")
    ap.add_argument("--plain-only", action="store_true", help="the five source forms and the projection only (for a kernel trace)")
    args = ap.parse_args()
    n, hw = args.images, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flows, _, occ, _ = eng.flow_tensor_bidir(frames, 1)
        gray = frames[:n].contiguous()
        del frames
        chw = torch.stack([gray, gray.roll(5, 2), gray.roll(3, 1)], 1).contiguous()
        hwc = chw.permute(0, 2, 3, 1).contiguous()
        pay = torch.stack([gray.float() / 16, flows[:, 0], flows[:, 1], gray.roll(7, 2).float() / 255], 1).contiguous()
        wild = smooth_random_flows(n, W / 4, H / 4)
        g = torch.Generator(device="cuda").manual_seed(491)
        imp = torch.exp(torch.rand((n, H, W), device="cuda", generator=g) * 3 - 2)
        srcs = {"gray": (gray, U8, 1, 0, W, 0, hw), "hwc": (hwc, U8, 3, 0, 3 * W, 0, 3 * hw), "chw": (chw, U8, 3, 1, W, hw, 3 * hw),
                "f1": (pay, F32, 1, 0, W, 0, 4 * hw), "f4": (pay, F32, 4, 1, W, hw, 4 * hw)}
        out8 = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")
        out32 = torch.empty((n, 4, H, W), device="cuda")
        hole = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        cov = torch.empty((n, H, W), device="cuda")
        pout = torch.empty((n, 2, H, W), device="cuda")
        work = torch.empty((5 * hw * n,), dtype=torch.int64, device="cuda")
        wb = work.numel() * 8

        def splat(src, flow="farneback", opt="plain", f32_out=False, keep=False, mode=0):
            t, dt, c, layout, pitch, plane, image = srcs[src]
            u8_out = dt == U8 and not f32_out and mode == 0
            o = out8 if u8_out else out32
            eng.splat_device(t.data_ptr(), dt, c, layout, pitch, plane, image, (flows if flow == "farneback" else wild).data_ptr(),
                             W, hw, 2 * hw, n, work.data_ptr(), wb, 1.0, 0.25, mode, int(keep), U8 if u8_out else F32,
                             o.data_ptr(), pitch, plane, c * hw, hole.data_ptr(), W, hw,
                             cov.data_ptr() if opt == "coverage" else None, W, hw,
                             imp.data_ptr() if opt == "importance" else None, W, hw,
                             occ.data_ptr() if opt == "occ" else None, W, hw)

        def project(flow="farneback"):
            eng.flow_project_device((flows if flow == "farneback" else wild).data_ptr(), W, hw, 2 * hw, n, work.data_ptr(), wb, 1.0,
                                    -1.0, 0.25, pout.data_ptr(), W, hw, 2 * hw, hole.data_ptr(), W, hw)

        forms = [("project", dict())] + [("splat", dict(src=s)) for s in srcs]
        if not args.plain_only:
            forms += [("project", dict(flow="random"))]
            forms += [("splat", dict(src=s, opt=o)) for s in ("gray", "f4") for o in ("importance", "occ", "coverage")]
            forms += [("splat", dict(src=s, keep=True)) for s in ("gray", "f4")]
            forms += [("splat", dict(src="gray", f32_out=True)), ("splat", dict(src="gray", mode=1)), ("splat", dict(src="f4", mode=1))]
            forms += [("splat", dict(src=s, flow="random")) for s in ("gray", "hwc", "f4")]
        times = [[] for _ in forms]
        for r in range(args.rounds + 1):
            for k, (what, kw) in enumerate(forms):
                fn = (lambda: splat(**kw)) if what == "splat" else (lambda: project(**kw))
                dt_ms = window(fn, args.calls)
                if r:  # round 0 warms every form
                    times[k].append(dt_ms)
        for (what, kw), ts in zip(forms, times):
            ts.sort()
            med = ts[len(ts) // 2]
            words = 3 if what == "project" else 1 + srcs[kw["src"]][2]
            (splat if what == "splat" else project)(**kw)
            print(json.dumps(dict(label=args.label, call=what, **kw, images=n, calls_per_window=args.calls,
                                  ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_image=med * 1e3 / n, words_per_pixel=words, us_per_image_per_word=med * 1e3 / n / words,
                                  hole_share=float(hole.float().mean()))), flush=True)
        if args.no_torch or args.plain_only:
            return
        for src, flow in (("gray", "farneback"), ("f4", "farneback"), ("gray", "random")):
            c = srcs[src][2]
            images = gray[:, None].float() if src == "gray" else pay
            src_flows = flows if flow == "farneback" else wild
            ts = []
            for r in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res, rhole = torch_splat(images, src_flows)
                torch.cuda.synchronize()
                if r:
                    ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            splat(src, flow, f32_out=True)
            both = ~rhole & (hole == 0)
            diff = (res - out32.view(-1)[:n * c * hw].view(n, c, H, W)).abs().amax(1)
            print(json.dumps(dict(label=args.label, call="torch_index_add_splat", src=src, flow=flow, images=n,
                                  ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                                  us_per_image=ts[len(ts) // 2] * 1e3 / n,
                                  max_abs_difference_where_neither_is_a_hole=float(diff[both].max()),
                                  median_abs_difference=float(diff[both][::97].median()),
                                  largest_payload=float(images.abs().max()),
                                  hole_planes_agree_share=float((rhole == (hole != 0)).float().mean()))), flush=True)
            del res, rhole, diff, both


if __name__ == "__main__":
    main()
