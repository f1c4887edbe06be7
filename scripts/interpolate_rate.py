#!/usr/bin/env python3
"""What interpolating frames costs at 1080p (profiles/interpolate/README.md, raw lines profiles/interpolate/*.jsonl): 64 pairs
resident in device memory — adjacent frames 0 .. 64 of the bench clip SynthClip(1920, 1080, seed=2), gray and as interleaved
BGR, with the library's own Farneback flows in both directions and their forward-backward masks — through
dfx_interpolate_device at t = 0.5 into uint8 images, with 0 and 3 fill passes, with the forward flow alone and with both; the
workspace holds all 64 pairs (one wave of launches per call).  In the same run, alternating round by round, the composed path
the calls of the previous version allow: dfx_flow_project_device twice, the fill passes of dfx_flow_median_device on either
side, dfx_warp_device twice to float32 with its valid plane, and the tiers, the blend, the clamp and the rounding in torch, every
buffer allocated beforehand; its images are compared with the single call's.  Per form: --calls synchronous calls back to back
inside one host-clock window, --rounds windows behind one warm window; median and spread (max - min) over the windows,
microseconds per pair; and the chip's copy rate measured in the same run in the same way (a device-to-device copy of the 64
forward flows: 16 B per pixel).  One JSON line per row on stdout.

--trace FORM runs that one form --calls times and nothing else (no composed path, no copy): the run to put under
`rocprofv3 --kernel-trace`, on its own.  --parse-trace DIR reads the kernel trace such a run left and prints, per pass of the
call, the device time per pair (the median launch of the pass times its launches per call), the synthesis pass's share of the
call and its bytes per second under the byte model of DESIGN.md: per pixel 16 B of flow planes, 2 B of hole planes, 2 B of
filled-hole planes with fill passes, C B of output and 2 C B of taps (each frame read once)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

W, H = 1920, 1080
FORMS = [(img, passes, bidir) for img in ("gray", "bgr") for passes in (0, 3) for bidir in (False, True)]


def form_name(img, passes, bidir):
    return f"{img}_passes{passes}_{'bidir' if bidir else 'fwd'}"


def synth_model_bytes(channels, passes):
    return 16 + 2 + (2 if passes > 0 else 0) + channels + 2 * channels  # per pixel


def parse_trace(directory, form, calls, pairs):
    img, passes, bidir = next(f for f in FORMS if form_name(*f) == form)
    channels = 1 if img == "gray" else 3
    files = glob.glob(os.path.join(directory, "**", "*_kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *_kernel_trace.csv under {directory}")
    fam = {"k_fs_zero": [], "k_fp_scatter": [], "k_fp_normalise": [], "k_flow_median": [], "k_interp_synth": []}
    for r in csv.DictReader(open(files[0])):
        for k in fam:
            if k in r["Kernel_Name"]:
                fam[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    per_pair = {}
    for k, ds in fam.items():
        if ds:
            ds.sort()
            per_pair[k] = ds[len(ds) // 2] * (len(ds) / calls) / pairs
    total = sum(per_pair.values())
    synth = per_pair.get("k_interp_synth", float("nan"))
    model = synth_model_bytes(channels, passes) * W * H
    print(json.dumps(dict(form=form, pairs=pairs, calls=calls, launches_per_call={k: len(v) / calls for k, v in fam.items() if v},
                          device_us_per_pair=per_pair, device_us_per_pair_total=total, synthesis_share_of_the_call=synth / total,
                          synthesis_model_bytes_per_pair=model, synthesis_model_tb_per_s=model / (synth * 1e-6) / 1e12)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every row (which build of the library this is)")
    ap.add_argument("--trace", default="", help="run this one form only (for a kernel trace)")
    ap.add_argument("--parse-trace", default="", help="directory of a kernel trace of --trace FORM (needs --trace FORM too)")
    args = ap.parse_args()
    if args.parse_trace:
        return parse_trace(args.parse_trace, args.trace, args.calls, args.pairs)

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import denseflow_amd as dfx
    from denseflow_amd.synth import SynthClip

    def window(fn, calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / calls

    n, hw, t = args.pairs, H * W, 0.5
    t1 = 1.0 - t
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    bgr = torch.stack([frames, 255 - frames, frames // 2 + 64], dim=-1).contiguous()
    clips = {"gray": (frames, 1, W, hw), "bgr": (bgr, 3, 3 * W, 3 * hw)}  # (clip, channels, pitch, image stride)
    with dfx.FlowEngine(W, H, "farn") as eng:
        fwd, bwd, occ_f, occ_b = eng.flow_tensor_bidir(frames, 1)
        per = {p: eng.interpolate_work_bytes(p) for p in (0, 3)}
        work = torch.empty((per[3] * n // 8 + 1,), dtype=torch.int64, device="cuda")
        outs = {"gray": torch.empty((n, H, W), dtype=torch.uint8, device="cuda"),
                "bgr": torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")}

        def single(img, passes, bidir):
            clip, ch, pitch, image = clips[img]
            eng.interpolate_device(clip.data_ptr(), clip.data_ptr() + image, ch, 0, pitch, 0, image, fwd.data_ptr(),
                                   bwd.data_ptr() if bidir else None, W, hw, 2 * hw, n, work.data_ptr(), per[passes] * n, t, 0.25,
                                   passes, 3, occ_f.data_ptr(), occ_b.data_ptr() if bidir else None, W, hw, 3,
                                   outs[img].data_ptr(), pitch, 0, image)

        if args.trace:
            form = next(f for f in FORMS if form_name(*f) == args.trace)
            for _ in range(args.calls):
                single(*form)
            return

        # the composed path: every intermediate a float32 plane in device memory
        G = [torch.empty((n, 2, H, W), device="cuda") for _ in range(4)]  # side 0, side 1 and their ping-pong twins
        M = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(6)]  # H0, H1 and two masks per side
        S = {img: [torch.empty(outs[img].shape, device="cuda") for _ in range(2)] for img in clips}
        V = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
        pwork = torch.empty((eng.flow_project_work_bytes() * n // 8,), dtype=torch.int64, device="cuda")
        composed_out = {}

        def composed(img, passes, bidir):
            clip, ch, pitch, image = clips[img]
            pw = (pwork.data_ptr(), pwork.numel() * 8)
            eng.flow_project_device(fwd.data_ptr(), W, hw, 2 * hw, n, *pw, t, -t, 0.25, G[0].data_ptr(), W, hw, 2 * hw,
                                    M[0].data_ptr(), W, hw, d_occ_ptr=occ_f.data_ptr(), occ_pitch=W, occ_stride=hw)
            if bidir:
                eng.flow_project_device(bwd.data_ptr(), W, hw, 2 * hw, n, *pw, t1, -t1, 0.25, G[1].data_ptr(), W, hw, 2 * hw,
                                        M[1].data_ptr(), W, hw, d_occ_ptr=occ_b.data_ptr(), occ_pitch=W, occ_stride=hw)
            else:
                eng.flow_project_device(fwd.data_ptr(), W, hw, 2 * hw, n, *pw, t, t1, 0.25, G[1].data_ptr(), W, hw, 2 * hw,
                                        M[1].data_ptr(), W, hw, d_occ_ptr=occ_f.data_ptr(), occ_pitch=W, occ_stride=hw)
            gf, hf = [], []
            for side in (0, 1):
                src, dst, msrc = G[side], G[2 + side], M[side]
                mdst = [M[2 + 2 * side], M[3 + 2 * side]]
                for k in range(passes):
                    eng.flow_median_device(src.data_ptr(), W, hw, 2 * hw, n, dst.data_ptr(), W, hw, 2 * hw, 3, 1, msrc.data_ptr(),
                                           W, hw, mdst[k % 2].data_ptr(), W, hw)
                    src, dst, msrc = dst, src, mdst[k % 2]
                gf.append(src)
                hf.append(msrc)
                eng.warp_device(clip.data_ptr() + side * image, ch, 0, pitch, 0, image, src.data_ptr(), W, hw, 2 * hw, n, 0, 0,
                                S[img][side].data_ptr(), pitch, 0, image, d_valid_ptr=V[side].data_ptr(), valid_pitch=W, valid_stride=hw)
            ins = [v != 0 for v in V]
            prim = [(M[k] == 0) & ins[k] for k in (0, 1)]
            cand = [(hf[k] == 0) & ins[k] for k in (0, 1)]
            first = prim[0] | prim[1]
            w0, w1 = torch.where(first, prim[0], cand[0]), torch.where(first, prim[1], cand[1])
            if ch == 3:
                w0, w1 = w0[..., None], w1[..., None]
            s0, s1 = S[img]
            p0, p1 = clip[:n].float(), clip[1:].float()
            o = torch.where(w0 & w1, s0 + t * (s1 - s0), torch.where(w0, s0, torch.where(w1, s1, p0 + t * (p1 - p0))))
            composed_out[img] = o.clamp_(0, 255).round_().to(torch.uint8)

        copy = torch.empty_like(fwd)
        times = {(path, f): [] for f in FORMS for path in ("single", "composed")}
        copies = []
        for r in range(args.rounds + 1):
            for f in FORMS:
                for path, fn in (("single", single), ("composed", composed)):
                    dt_ms = window(lambda: fn(*f), args.calls)
                    if r:  # round 0 warms every form
                        times[(path, f)].append(dt_ms)
            dt_ms = window(lambda: (copy.copy_(fwd), torch.cuda.synchronize()), args.calls)
            if r:
                copies.append(dt_ms)
        copies.sort()
        copy_ms = copies[len(copies) // 2]
        print(json.dumps(dict(label=args.label, form="device_to_device_copy_of_the_forward_flows", pairs=n, calls_per_window=args.calls,
                              ms_per_call=dict(median=copy_ms, spread=copies[-1] - copies[0], runs=[round(x, 4) for x in copies]),
                              us_per_pair=copy_ms * 1e3 / n, model_bytes=n * hw * 16,
                              model_tb_per_s=n * hw * 16 / (copy_ms * 1e-3) / 1e12)), flush=True)
        for f in FORMS:
            img, passes, bidir = f
            single(*f)
            composed(*f)
            torch.cuda.synchronize()
            diff = (outs[img].int() - composed_out[img].int()).abs()
            row = dict(label=args.label, form=form_name(*f), image=img, fill_passes=passes, backward_flow=bidir, pairs=n,
                       calls_per_window=args.calls, workspace_bytes_per_pair=per[passes],
                       composed_differs_in_pixels=int((diff != 0).sum()), composed_max_abs_difference=int(diff.max()))
            for path in ("single", "composed"):
                ts = sorted(times[(path, f)])
                med = ts[len(ts) // 2]
                row[path] = dict(ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                 us_per_pair=med * 1e3 / n)
            row["composed_over_single"] = row["composed"]["us_per_pair"] / row["single"]["us_per_pair"]
            row["us_per_pair_of_the_copy"] = copy_ms * 1e3 / n
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
