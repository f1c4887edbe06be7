#!/usr/bin/env python3
"""What chaining flows costs at 1080p (profiles/flow_chain/README.md, raw lines profiles/flow_chain/rate_1080p.jsonl):
64 flows resident in device memory — the library's own Farneback flows of adjacent frames 0 .. 64 of the bench clip
SynthClip(1920, 1080, seed=2), forward, with the forward occlusion masks of the bidirectional call for the masked forms —
through dfx_flow_chain_device with L in {2, 6, 15} links, emit last and all, with and without the masks, every anchor that
fits (65 - L chains per call, anchor_step 1), valid planes written; and one case (L = 6, last, no masks) on smooth random
flows of up to a quarter of the frame, where neighbouring lanes still land on neighbouring taps but far from home.  Per
form: --calls synchronous calls back to back inside one host-clock window (each call returns with the device idle, so the
figure INCLUDES the launch and one stream synchronisation per call), --rounds windows behind one warm window, the forms
alternating round by round; median and spread (max - min) over the windows, microseconds per link (one flow sampled at every
pixel) and per emitted flow, and the bytes that must move — per pixel and link 8 B gathered and 1 B of mask where masks are
read (up to 4 where the taps' bytes share no sector), per pixel and emitted flow 9 B written (8 of flow, 1 of valid) — as a
rate and as a share of the chip's copy rate, measured in the same run in the same way (a device-to-device copy of the 64
flows: 16 B per pixel).  Then the same chain through torch alone (a grid build, F.grid_sample with align_corners and the
border padding, and an add per link; 8 anchors at a time) against the device's clamp-border result.  One JSON line per row
on stdout."""
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


def torch_chain(flows, length, anchors):
    """A_L of `anchors` chains of hop 1, anchor_step 1, clamp border: (anchors, 2, H, W)."""
    ys, xs = torch.meshgrid(torch.arange(H, device=flows.device, dtype=torch.float32),
                            torch.arange(W, device=flows.device, dtype=torch.float32), indexing="ij")
    out = torch.empty((anchors, 2, H, W), device=flows.device)
    for j0 in range(0, anchors, CHUNK):
        m = min(CHUNK, anchors - j0)
        a = torch.zeros((m, 2, H, W), device=flows.device)
        for k in range(length):
            gx = (xs + a[:, 0]) * (2.0 / (W - 1)) - 1.0
            gy = (ys + a[:, 1]) * (2.0 / (H - 1)) - 1.0
            a = a + F.grid_sample(flows[j0 + k:j0 + k + m], torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border",
                                  align_corners=True)
        out[j0:j0 + m] = a
    return out


def smooth_random_flows(n, mag_x, mag_y):
    g = torch.Generator(device="cuda").manual_seed(480)
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
    ap.add_argument("--flows", type=int, default=64)
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
        lmax = 15
        room = max((n - L + 1) * L for L in (2, 6, lmax))  # output flows of the largest form
        out = torch.empty((room, 2, H, W), device="cuda")
        valid = torch.empty((room, H, W), dtype=torch.uint8, device="cuda")
        copy = torch.empty_like(flows)
        forms = [("farneback", L, emit, masked) for L in (2, 6, lmax) for emit in ("last", "all") for masked in (False, True)]
        forms.append(("smooth_random_quarter_frame", 6, "last", False))

        def call(src, L, emit, masked, border="zero"):
            eng.flow_chain_device((flows if src == "farneback" else wild).data_ptr(), W, hw, 2 * hw, n, out.data_ptr(), W, hw,
                                  2 * hw, L, 0, 1, n - L + 1, 1, dfx.engine.CHAIN_EMITS[emit], dfx.engine.WARP_BORDERS[border],
                                  occ.data_ptr() if masked else None, W, hw, valid.data_ptr(), W, hw)

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
        for f in forms:
            src, L, emit, masked = f
            m = n - L + 1
            links, emitted = m * L, m * (L if emit == "all" else 1)
            ts = sorted(times[f])
            med = ts[len(ts) // 2]
            nbytes = hw * (links * (9 if masked else 8) + emitted * 9)
            tb = nbytes / (med * 1e-3) / 1e12
            call(*f)
            print(json.dumps(dict(label=args.label, flows_from=src, length=L, emit=emit, masked=masked, anchors=m, links=links,
                                  emitted_flows=emitted, calls_per_window=args.calls,
                                  ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_link=med * 1e3 / links, us_per_emitted_flow=med * 1e3 / emitted, model_bytes=nbytes,
                                  model_tb_per_s=tb, share_of_the_copy_rate=tb / copy_tb,
                                  valid_share_after_the_last_link=float(valid[emitted - 1].float().mean()))), flush=True)
        if args.no_torch:
            return
        # the same chain through torch alone, against the device's clamp-border result
        for src, L in (("farneback", 2), ("farneback", 6), ("farneback", lmax), ("smooth_random_quarter_frame", 6)):
            m = n - L + 1
            src_flows = flows if src == "farneback" else wild
            ts = []
            for r in range(min(args.rounds, 3) + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = torch_chain(src_flows, L, m)
                torch.cuda.synchronize()
                if r:
                    ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            call(src, L, "last", False, "clamp")
            diff = (res - out[:m]).abs().amax(1)
            largest = float(out[:m].abs().max())
            torch.cuda.synchronize()  # torch has read `out` before the library writes it again
            call(src, L, "last", False, "zero")
            ok = valid[:m] != 0
            print(json.dumps(dict(label=args.label, form="torch_grid_sample_chain", flows_from=src, length=L, anchors=m, links=m * L,
                                  ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                                  us_per_link=ts[len(ts) // 2] * 1e3 / (m * L),
                                  max_abs_difference_from_the_device_px=float(diff.max()),
                                  max_abs_difference_over_valid_pixels_px=float(diff[ok].max()),
                                  median_abs_difference_px=float(diff.flatten()[::97].median()),
                                  largest_flow_px=largest)), flush=True)
            del res, diff


if __name__ == "__main__":
    main()
