#!/usr/bin/env python3
"""What the flow median costs at 1080p (profiles/flow_median/README.md, raw lines profiles/flow_median/rate_1080p.jsonl):
64 flows resident in device memory — the library's own Farneback flows of frames 0 .. 64 of the bench clip
SynthClip(1920, 1080, seed=2), forward, with the forward occlusion masks of the bidirectional call for the masked forms —
through dfx_flow_median_device in each of its six instantiations (ksize 3 / 5; no mask, mask with mode all, mask with mode
fill; the masked forms write mask_out), and the two fill forms again with synthetic masks that mark 30 % of the pixels in
blobs (a thresholded 31 x 31 box average of noise), because a fill costs what its mask marks.  Per form: --calls
synchronous calls back to back inside one host-clock window (each call returns with the device idle, so the figure
INCLUDES the launch and one stream synchronisation per call), --rounds
windows behind one warm window, the forms alternating round by round; median and spread (max - min) over the windows,
microseconds per flow, and the bytes that must move — 16 B per pixel unmasked (8 read, 8 written), 18 B with a mask read
and mask_out written — as a rate and as a share of the chip's copy rate, measured in the same run in the same way (a
device-to-device copy of the 64 flows: the same 16 B per pixel).  Then the same filter through torch alone (F.pad
replicate, unfold, median along the window; for the masked fill: sort with the excluded samples at +inf and a gather of
rank (m - 1) >> 1), 8 flows at a time because the unfolded windows are 25 times the flows.  One JSON line per row on stdout."""
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


def torch_windows(x, ksize):
    """(n, c, H, W) -> (n, c, H, W, ksize * ksize), replicated border."""
    r = ksize // 2
    p = F.pad(x, (r, r, r, r), mode="replicate")
    return p.unfold(2, ksize, 1).unfold(3, ksize, 1).reshape(x.shape[0], x.shape[1], H, W, ksize * ksize)


def torch_median(flows, ksize):
    out = torch.empty_like(flows)
    for i in range(0, flows.shape[0], CHUNK):
        out[i:i + CHUNK] = torch_windows(flows[i:i + CHUNK], ksize).median(dim=-1).values
    return out


def torch_fill(flows, masks, ksize):
    out = torch.empty_like(flows)
    left = torch.empty_like(masks)
    for i in range(0, flows.shape[0], CHUNK):
        fl, mk = flows[i:i + CHUNK], masks[i:i + CHUNK]
        excl = torch_windows((mk != 0).float()[:, None], ksize) != 0                 # (n, 1, H, W, k²)
        m = ksize * ksize - excl.sum(-1)                                             # (n, 1, H, W)
        keys = torch.where(excl, float("inf"), torch_windows(fl, ksize)).sort(dim=-1).values
        rank = ((m - 1).clamp(min=0) >> 1)[..., None].expand(-1, 2, -1, -1, -1)
        med = keys.gather(-1, rank)[..., 0]
        keep = (m == 0) | (mk[:, None] == 0)
        out[i:i + CHUNK] = torch.where(keep, fl, med)
        left[i:i + CHUNK] = (m[:, 0] == 0).to(torch.uint8)
    return out, left


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
    args = ap.parse_args()
    n, hw = args.flows, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flows, _, occ, _ = eng.flow_tensor_bidir(frames, 1)
        out = torch.empty_like(flows)
        copy = torch.empty_like(flows)
        mask_out = torch.empty_like(occ)
        g = F.avg_pool2d(torch.randn((n, 1, H, W), device="cuda"), 31, stride=1, padding=15)[:, 0]
        blobs = (g > g.flatten()[::257].quantile(0.7)).to(torch.uint8)
        del g
        forms = [(k, m) for k in (3, 5) for m in ("none", "all", "fill")] + [(3, "fill_blobs"), (5, "fill_blobs")]

        def call(ksize, form):
            masked = form != "none"
            masks = blobs if form == "fill_blobs" else occ
            eng.flow_median_device(flows.data_ptr(), W, hw, 2 * hw, n, out.data_ptr(), W, hw, 2 * hw, ksize,
                                   dfx.engine.MEDIAN_MODES["all" if form in ("none", "all") else "fill"],
                                   masks.data_ptr() if masked else None, W, hw, mask_out.data_ptr() if masked else None, W, hw)

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
        print(json.dumps(dict(form="device_to_device_copy_of_the_flows", flows=n, calls_per_window=args.calls,
                              ms_per_call=dict(median=copy_ms, spread=copies[-1] - copies[0], runs=[round(x, 4) for x in copies]),
                              us_per_flow=copy_ms * 1e3 / n, model_bytes=n * hw * 16, model_tb_per_s=copy_tb)), flush=True)
        shares = {"all": float((occ != 0).float().mean()), "fill_blobs": float((blobs != 0).float().mean())}
        shares["fill"] = shares["all"]
        for f in forms:
            ksize, form = f
            ts = sorted(times[f])
            med = ts[len(ts) // 2]
            nbytes = n * hw * (16 if form == "none" else 18)
            tb = nbytes / (med * 1e-3) / 1e12
            call(*f)
            print(json.dumps(dict(ksize=ksize, form=form, flows=n, calls_per_window=args.calls,
                                  ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_flow=med * 1e3 / n, model_bytes=nbytes, model_tb_per_s=tb,
                                  share_of_the_copy_rate=tb / copy_tb, masked_share=shares.get(form),
                                  pixels_left_masked=int(mask_out.sum()) if form != "none" else None)), flush=True)
        # the same filter through torch alone
        for ksize, form in ((3, "none"), (5, "none"), (5, "fill")):
            ts = []
            for r in range(min(args.rounds, 3) + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                res = torch_median(flows, ksize) if form == "none" else torch_fill(flows, occ, ksize)
                torch.cuda.synchronize()
                if r:
                    ts.append((time.perf_counter() - t) * 1e3)
            ts.sort()
            call(ksize, form)
            if form == "none":
                differing = int((res.view(torch.int32) != out.view(torch.int32)).sum())
            else:
                differing = int((res[0].view(torch.int32) != out.view(torch.int32)).sum()) + int((res[1] != mask_out).sum())
            print(json.dumps(dict(form="torch_" + ("median" if form == "none" else "fill"), ksize=ksize, flows=n,
                                  ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                                  us_per_flow=ts[len(ts) // 2] * 1e3 / n, elements_differing_from_the_device=differing)),
                  flush=True)


if __name__ == "__main__":
    main()
