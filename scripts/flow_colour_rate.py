#!/usr/bin/env python3
"""What colouring flows costs at 1080p (profiles/flow_colour/README.md, raw lines profiles/flow_colour/*.jsonl): 64 flows
resident in device memory — the library's own Farneback flows of adjacent frames 0 .. 64 of the bench clip
SynthClip(1920, 1080, seed=2), with the forward-backward masks of the same bidirectional call — through
dfx_flow_colour_device into interleaved RGB images: FIXED mode without d_max2 (one pass), FLOW and BATCH (the measuring pass
and the colour pass), FLOW with a mask, FLOW blended over a BGR frame.  In the same run, alternating round by round with
every form: a device-to-device copy that moves the form's byte model (half of it read, half of it written), and the same
formulas composed from torch ops with torch.atan2, whose images are compared with the library's (the polynomial angle and
torch's differ in a few bytes by one level).  Per form: --calls synchronous calls back to back inside one host-clock window,
--rounds windows behind one warm window; median and spread (max - min) over the windows.  One JSON line per row on stdout.
--trace FORM runs that one form --calls times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`, on
its own, for the device time of each pass.

Byte model per pixel: 8 B of flow read per pass, 1 B of mask per pass, 3 B of frame, 3 B written."""
import argparse
import json
import os
import sys
import time

W, H = 1920, 1080
#        name            norm     masked blended  passes
FORMS = [("fixed", "fixed", False, False, 1), ("flow", "flow", False, False, 2), ("batch", "batch", False, False, 2),
         ("flow_masked", "flow", True, False, 2), ("flow_blended", "flow", False, True, 2)]
MAX_RAD = 8.0


def model_bytes(masked, blended, passes):
    return passes * (8 + (1 if masked else 0)) + (3 if blended else 0) + 3  # per pixel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every row (which build of the library this is)")
    ap.add_argument("--no-torch-path", action="store_true", help="time the library and the copy only")
    ap.add_argument("--trace", default="", help="run this one form --calls times and nothing else (for a kernel trace)")
    args = ap.parse_args()

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

    n, hw = args.flows, H * W
    frames = SynthClip(W, H, 2).frames_torch(n + 1, "cuda")
    bgr = torch.stack([frames[:n], 255 - frames[:n], frames[:n] // 2 + 64], dim=-1).contiguous()
    wheel = torch.from_numpy(dfx.colour_wheel()).to("cuda").float() / 255.0
    with dfx.FlowEngine(W, H, "farn") as eng:
        fwd, _, occ, _ = eng.flow_tensor_bidir(frames, 1)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        max2 = torch.empty(n + 1, device="cuda")

        def single(name, norm, masked, blended, passes):
            eng.flow_colour_device(fwd.data_ptr(), W, hw, 2 * hw, n, out.data_ptr(), 3 * W, 0, 3 * hw, dfx.engine.COLOUR_NORMS[norm],
                                   MAX_RAD if norm == "fixed" else 0.0, max2.data_ptr() if passes == 2 else None, 1, 0, (0, 0, 0),
                                   occ.data_ptr() if masked else None, W, hw, bgr.data_ptr() if blended else None, 3, 0, 3 * W, 0,
                                   3 * hw, 128)

        if args.trace:
            form = next(f for f in FORMS if f[0] == args.trace)
            for _ in range(args.calls):
                single(*form)
            return

        composed_out = torch.empty_like(out)

        def composed(name, norm, masked, blended, passes, chunk=8):
            """The same formulas from torch ops, eight flows at a time (every intermediate is an (8, H, W[, 3]) tensor)."""
            u, v = fwd[:, 0], fwd[:, 1]
            known = (u.abs() <= 1e9) & (v.abs() <= 1e9)
            if masked:
                known &= occ == 0
            r2 = torch.where(known, u * u + v * v, torch.zeros((), device="cuda"))
            if norm == "fixed":
                R = torch.full((n,), MAX_RAD, device="cuda")
            else:
                m2 = r2.amax(dim=(1, 2))
                R = torch.sqrt(m2 if norm == "flow" else m2.amax().expand(n))
            D = (R + 2.0 ** -23).view(n, 1, 1)
            for i in range(0, n, chunk):
                s = slice(i, i + chunk)
                un, vn = u[s] / D[s], v[s] / D[s]
                rad = torch.sqrt(un * un + vn * vn)
                if norm != "fixed":
                    rad = rad.clamp(max=1.0)
                fk = ((torch.atan2(-vn, -un) / torch.pi + 1.0) * 27.0).clamp(0.0, 54.0).nan_to_num_(0.0)
                k0 = fk.floor()
                f = (fk - k0)[..., None]
                k0 = k0.long()
                k1 = torch.where(k0 == 54, 0, k0 + 1)
                col = (1.0 - f) * wheel[k0] + f * wheel[k1]
                rad = rad[..., None]
                col = torch.where(rad <= 1.0, 1.0 - rad * (1.0 - col), col * 0.75)
                img = (255.0 * col).floor().clamp(0.0, 255.0).nan_to_num_(0.0).to(torch.uint8)
                img = torch.where(known[s][..., None], img, torch.zeros((), dtype=torch.uint8, device="cuda"))
                if blended:
                    img = ((128 * img.int() + 128 * bgr[s].int() + 128) >> 8).to(torch.uint8)
                composed_out[s] = img

        copies = {}
        for f in FORMS:
            half = hw * n * model_bytes(*f[2:]) // 2
            copies[f[0]] = (torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda"))
        paths = [("single", single), ("copy", lambda name, *a: copies[name][1].copy_(copies[name][0]))]
        if not args.no_torch_path:
            paths.append(("composed", composed))
        times = {(path, f[0]): [] for f in FORMS for path, _ in paths}
        for r in range(args.rounds + 1):
            for f in FORMS:
                for path, fn in paths:
                    dt_ms = window(lambda: fn(*f), args.calls if path != "composed" else max(args.calls // 5, 1))
                    if r:  # round 0 warms every form
                        times[(path, f[0])].append(dt_ms)
        for f in FORMS:
            name, norm, masked, blended, passes = f
            model = model_bytes(masked, blended, passes) * hw * n
            row = dict(label=args.label, form=name, norm=norm, masked=masked, blended=blended, passes=passes, flows=n,
                       calls_per_window=args.calls, model_bytes_per_pixel=model_bytes(masked, blended, passes))
            for path, _ in paths:
                ts = sorted(times[(path, name)])
                med = ts[len(ts) // 2]
                row[path] = dict(ms_per_call=dict(median=med, spread=ts[-1] - ts[0], runs=[round(x, 4) for x in ts]),
                                 us_per_flow=med * 1e3 / n, model_tb_per_s=model / (med * 1e-3) / 1e12)
            row["fraction_of_the_copy_rate"] = row["copy"]["us_per_flow"] / row["single"]["us_per_flow"]
            if not args.no_torch_path:
                single(*f)
                composed(*f)
                torch.cuda.synchronize()
                diff = (out.int() - composed_out.int()).abs()
                row["composed_over_single"] = row["composed"]["us_per_flow"] / row["single"]["us_per_flow"]
                row["composed_differs_in_bytes"] = int((diff != 0).sum())
                row["composed_max_abs_difference"] = int(diff.max())
                row["bytes_compared"] = diff.numel()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
