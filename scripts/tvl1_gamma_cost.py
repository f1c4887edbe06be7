#!/usr/bin/env python3
"""python scripts/tvl1_gamma_cost.py — step-kernel time per pixel-iteration of the 1080p bench clip (SynthClip seed 2, 130 frames = one device batch) through
calc_optflows_device at tvl1_gamma 0 and 0.4: step_ms / tvl1_px_iters of dfx_stats, one warm pass and two timed ones."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import denseflow_amd
from denseflow_amd.synth import SynthClip

W, H, N = 1920, 1080, 130
dev = torch.device("cuda:0")
d_frames = SynthClip(W, H, seed=2).frames_torch(N, dev)
out = torch.empty((N - 1, H, W, 2), dtype=torch.float32, device=dev)
res = {}
for gamma in (0.0, 0.4, 0.0, 0.4):
    with denseflow_amd.FlowEngine(W, H, "tvl1", tvl1_gamma=gamma) as eng:
        for p in range(3):
            eng.reset_stats()
            eng.calc_optflows_device(d_frames.data_ptr(), W, W * H, N, 1, out.data_ptr(), W * H * 2)
            st = eng.stats()
            if p:
                r = dict(gamma=gamma, step_ms=st.step_ms, px_iters=st.tvl1_px_iters, ns_per_px_iter=st.step_ms * 1e6 / st.tvl1_px_iters,
                         mean_iters=st.tvl1_total_iters / st.pairs, device_ms=st.device_ms, batch=st.batch, finite=bool(torch.isfinite(out).all()))
                print(json.dumps(r), flush=True)
                res.setdefault(gamma, []).append(r["ns_per_px_iter"])
a, b = min(res[0.0]), min(res[0.4])
print(json.dumps(dict(ns_per_px_iter_gamma0=a, ns_per_px_iter_gamma04=b, ratio=b / a)))
