#!/usr/bin/env python3
"""What the global-motion fit costs at 1080p (profiles/global_motion/README.md, raw lines
profiles/global_motion/rate_1080p.jsonl): 64 flows resident in device memory — the library's own Farneback flows of frames
0 .. 64 of the bench clip SynthClip(1920, 1080, seed=2) — through dfx_global_motion_device with the affine and the translation
model, rounds 1 / 3 / 5, with the apply pass (compensated flows and moving masks written) and without it (the fit alone).
Per form: --calls synchronous calls back to back inside one host-clock window (each call returns with the device idle, so
the figure INCLUDES the zeroing of the records, rounds (+ 1) launches and one stream synchronisation per call), --rounds
windows behind one warm window, the forms alternating round by round; median and spread (max - min) over the windows,
microseconds per flow, and the byte model — 8 B per pixel and round read, + 8 B read, 8 B and 1 B written by the apply pass —
as a rate.  Then the same five-round affine fit and subtraction through torch alone (masked moment sums accumulated in
float64, a batched 3 x 3 solve, every pass a kernel of its own), and the Farneback call that produced the flows, timed in
the same run: the fit's share of one pair's time.  One JSON line per row on stdout."""
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


def torch_global_motion(flows, rounds=5, thr=0.5, growth=2.0):
    """The robust affine fit and the subtraction in torch alone: (params (n, 6) float64 in centred doubled coordinates,
    compensated flows, moving masks).  Per round a residual, a mask, twelve masked sums accumulated in float64 and a batched
    3 x 3 solve; every pass a kernel of its own."""
    n = flows.shape[0]
    xc = (2 * torch.arange(W, device="cuda", dtype=torch.float32) - (W - 1))[None, None, :]
    yc = (2 * torch.arange(H, device="cuda", dtype=torch.float32) - (H - 1))[None, :, None]
    u, v = flows[:, 0], flows[:, 1]
    ok = (u.abs() < 4096) & (v.abs() < 4096)

    def total(t):
        return t.sum(dim=(1, 2), dtype=torch.float64)

    def residual(p):
        pf = p.float()[:, :, None, None]
        return u - (pf[:, 0] + pf[:, 1] * xc + pf[:, 2] * yc), v - (pf[:, 3] + pf[:, 4] * xc + pf[:, 5] * yc)

    p = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    inl = ok
    for k in range(rounds):
        if k:
            ru, rv = residual(p)
            inl = ok & (ru * ru + rv * rv <= (thr * growth ** (rounds - 1 - k)) ** 2)
        m = inl.float()
        mx, my, mu, mv = m * xc, m * yc, torch.where(inl, u, 0.0), torch.where(inl, v, 0.0)
        S1, Sx, Sy, Sxx, Sxy, Syy = total(m), total(mx), total(my), total(mx * xc), total(mx * yc), total(my * yc)
        N = torch.stack([torch.stack([S1, Sx, Sy], -1), torch.stack([Sx, Sxx, Sxy], -1), torch.stack([Sy, Sxy, Syy], -1)], 1)
        rhs = torch.stack([torch.stack([total(mu), total(mu * xc), total(mu * yc)], -1),
                           torch.stack([total(mv), total(mv * xc), total(mv * yc)], -1)], -1)
        p = torch.linalg.solve(N, rhs).transpose(1, 2).reshape(n, 6)
    ru, rv = residual(p)
    moving = ~(ok & (ru * ru + rv * rv <= thr * thr))
    return p, torch.stack([ru, rv], 1), moving.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    n, hw = args.flows, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    with dfx.FlowEngine(W, H, "farn") as eng:
        flows = eng.flow_tensor(frames, 1)
        out = torch.empty_like(flows)
        moving = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        rec = torch.zeros((n, 352 // 8), dtype=torch.int64, device="cuda")
        # (model, rounds, with the apply pass)
        forms = [(m, r, a) for m in ("affine", "translation") for r in (1, 3, 5) for a in (False, True)]

        def call(model, rounds, apply):
            eng.global_motion_device(flows.data_ptr(), W, hw, 2 * hw, n, rec.data_ptr(), dfx.engine.GM_MODELS[model], rounds, 0.5,
                                     2.0, None, 0, 0, out.data_ptr() if apply else None, W, hw, 2 * hw,
                                     moving.data_ptr() if apply else None, W, hw)

        times = {f: [] for f in forms}
        farn = []
        for r in range(args.rounds + 1):
            for f in forms:
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(args.calls):
                    call(*f)
                dt_ms = (time.perf_counter() - t) * 1e3 / args.calls
                if r:  # round 0 warms every form
                    times[f].append(dt_ms)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.flow_tensor(frames, 1, out=flows)
            if r:
                farn.append((time.perf_counter() - t) * 1e3)
        farn.sort()
        farn_us = farn[len(farn) // 2] * 1e3 / n
        print(json.dumps(dict(form="farneback_flow_tensor", pairs=n, ms_per_call=dict(median=farn[len(farn) // 2],
                                                                                      spread=farn[-1] - farn[0],
                                                                                      runs=[round(x, 3) for x in farn]),
                              us_per_pair=farn_us)), flush=True)
        for f in forms:
            model, rounds, apply = f
            ts = sorted(times[f])
            med = ts[len(ts) // 2]
            nbytes = n * hw * (8 * rounds + (17 if apply else 0))
            call(*f)
            host = rec.cpu().numpy().view("uint8").reshape(n, -1).copy().view(dfx.engine.GM_RESULT_DTYPE).reshape(n)
            print(json.dumps(dict(model=model, rounds=rounds, apply=apply, flows=n, calls_per_window=args.calls,
                                  ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                  us_per_flow=med * 1e3 / n, us_per_flow_and_pass=med * 1e3 / n / (rounds + int(apply)),
                                  model_bytes=nbytes, model_tb_per_s=nbytes / (med * 1e-3) / 1e12,
                                  share_of_a_farneback_pair=med * 1e3 / n / farn_us,
                                  last_round_inlier_share=float(host["inliers"][:, rounds - 1].mean() / hw),
                                  status_nonzero=int((host["status"] != 0).sum()), a_of_flow_0=[float(x) for x in host["a"][0]])),
                  flush=True)
        # the same fit and subtraction through torch alone
        ts = []
        for r in range(args.rounds + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            p, comp, mv = torch_global_motion(flows)
            torch.cuda.synchronize()
            if r:
                ts.append((time.perf_counter() - t) * 1e3)
        ts.sort()
        call("affine", 5, True)
        host = rec.cpu().numpy().view("uint8").reshape(n, -1).copy().view(dfx.engine.GM_RESULT_DTYPE).reshape(n)
        dev_p = torch.from_numpy(host["p"].astype("float64")).cuda()
        print(json.dumps(dict(form="torch_affine_5_rounds_and_subtraction", flows=n,
                              ms_per_call=dict(median=ts[len(ts) // 2], spread=ts[-1] - ts[0], runs=[round(x, 3) for x in ts]),
                              us_per_flow=ts[len(ts) // 2] * 1e3 / n, share_of_a_farneback_pair=ts[len(ts) // 2] * 1e3 / n / farn_us,
                              max_abs_param_difference_to_device=float((p - dev_p).abs().max()),
                              max_abs_compensated_difference_to_device=float((comp - out).abs().max()),
                              moving_pixels_differing=int((mv != moving).sum()))), flush=True)


if __name__ == "__main__":
    main()
