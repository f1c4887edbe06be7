#!/usr/bin/env python3
"""What a caller-supplied initial flow costs and buys at 1080p (profiles/initial_flow/README.md): the bench clip
(SynthClip(1920, 1080, seed=2), 130 frames = one device batch of 129 pairs) through calc_optflows_device, for TVL1 and
Farneback in three configurations:

  (a) defaults, unseeded;
  (b) one level (tvl1_nscales = 1 / farn_num_levels = 0), pair i seeded with pass (a)'s flow of pair i - 1 (pair 0: zeros);
  (c) defaults, seeded the same way.

Per configuration: pairs/s (one warm pass, then the median of three timed ones), tvl1_total_iters per pair, the mean
end-point error against SynthClip.true_flow on every 16th pair, device_ms per pass.  For TVL1 the seed launches' share of
device_ms is measured by difference: the same calls with tvl1_warps = 0 run level control, the seed chain, the upsamples
and the merge only, so seeded minus unseeded there is the chain's time.  One JSON line per configuration on stdout."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import denseflow_amd as dfx  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402

W, H, N = 1920, 1080, 130


def run(eng, frames, out, init=None, passes=3):
    def once():
        eng.reset_stats()
        torch.cuda.synchronize()
        t = time.perf_counter()
        eng.calc_optflows_device(frames.data_ptr(), W, W * H, N, 1, out.data_ptr(), W * H * 2,
                                 init=None if init is None else init.data_ptr())
        dt = time.perf_counter() - t
        st = eng.stats()
        return dt, st.device_ms, st.tvl1_total_iters / max(st.pairs, 1)

    once()
    res = sorted(once() for _ in range(passes))
    return res[len(res) // 2]


def epe(out, clip):
    idx = list(range(0, N - 1, 16))
    e = []
    for i in idx:
        t = clip.true_flow(i, i + 1).astype(np.float32)
        f = out[i].cpu().numpy()
        e.append(float(np.mean(np.hypot(f[..., 0] - t[..., 0], f[..., 1] - t[..., 1]))))
    return float(np.mean(e))


def main():
    clip = SynthClip(W, H, 2)
    frames = clip.frames_torch(N, "cuda")
    one_level = {"tvl1": dict(tvl1_nscales=1), "farn": dict(farn_num_levels=0)}
    for algo in ("tvl1", "farn"):
        flows_a = torch.empty((N - 1, H, W, 2), dtype=torch.float32, device="cuda")
        out = torch.empty_like(flows_a)
        with dfx.FlowEngine(W, H, algo) as eng:
            dt, ms, it = run(eng, frames, flows_a)
            print(json.dumps(dict(algo=algo, config="a_unseeded_defaults", pairs_per_s=(N - 1) / dt, device_ms=ms,
                                  iters_per_pair=it, epe_px=epe(flows_a, clip))), flush=True)
        seed = torch.zeros_like(flows_a)
        seed[1:] = flows_a[:-1]
        for name, kw in (("b_seeded_one_level", one_level[algo]), ("c_seeded_defaults", dict())):
            with dfx.FlowEngine(W, H, algo, **kw) as eng:
                dt, ms, it = run(eng, frames, out, seed)
            rec = dict(algo=algo, config=name, pairs_per_s=(N - 1) / dt, device_ms=ms, iters_per_pair=it, epe_px=epe(out, clip))
            if algo == "tvl1":
                with dfx.FlowEngine(W, H, algo, tvl1_warps=0, **kw) as eng:
                    ms1 = run(eng, frames, out, seed)[1]
                    ms0 = run(eng, frames, out)[1]
                rec.update(seed_chain_ms=ms1 - ms0, seed_share_of_device_ms=(ms1 - ms0) / ms)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
