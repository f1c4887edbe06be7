#!/usr/bin/env python3
"""What the motion descriptors of flows cost at 1080p (profiles/flow_hist/README.md, raw lines profiles/flow_hist/*.jsonl): 64
flows resident in device memory — the library's own Farneback flows of adjacent frames 0 .. 64 of the bench clip
SynthClip(1920, 1080, seed=2), with the forward-backward masks of the same bidirectional call — through dfx_flow_hist_device
into the integer sums and the (n, D, CH, CW) float values, 8 bins, no normalisation: HOF alone, MBH alone (MBHx + MBHy) and
all three kinds, at cell 8 and 16, without and with the mask.  Three more inputs of the same size tell what binds the kernel,
all three kinds at cell 8: every pixel (3, 0), so that every pixel of a cell adds to one slot (the contention worst case); a
random axis direction per pixel, so that no run of a lane's four pixels merges (the most atomics); and the zero flow with the
still slot off, which loads and computes the same and issues no atomic at all.  In the same run, alternating round by round
with every form: a device-to-device copy that moves the form's byte model (half of it read, half of it written), and the same
definition composed from torch ops (gradients by slicing, torch.atan2, integer scatter_add_), whose sums are compared with the
library's (the polynomial angle and torch's move a weight of 1 / 256 between neighbouring slots here and there).  Per form:
--calls synchronous calls back to back inside one host-clock window, --rounds windows behind one warm window; median and spread
(max - min) over the windows.  One JSON line per row on stdout.

Byte model per pixel: 8 B of flow read, 1 B of mask; the outputs are D * 12 / cell^2 B per pixel and left out."""
import argparse
import json
import os
import sys
import time

W, H = 1920, 1080
BINS, THR = 8, 0.4
KINDS = {"hof": 1, "mbh": 6, "all": 7}
#        name, kinds, cell, masked, input
FORMS = [(f"{k}_c{c}{'_masked' if m else ''}", k, c, m, "farn") for k in KINDS for c in (8, 16) for m in (False, True)]
FORMS += [("all_c8_one_direction", "all", 8, False, "one"), ("all_c8_random_axes", "all", 8, False, "axes"),
          ("all_c8_zero_no_atomics", "all", 8, False, "zero"), ("all_c4", "all", 4, False, "farn"), ("all_c32", "all", 32, False, "farn")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into every row (which build of the library this is)")
    ap.add_argument("--no-torch-path", action="store_true", help="time the library and the copy only")
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
    with dfx.FlowEngine(W, H, "farn") as eng:
        fwd, _, occ, _ = eng.flow_tensor_bidir(frames, 1)
        one = torch.zeros_like(fwd)
        one[:, 0] = 3.0
        d = torch.randint(0, 4, (n, H, W), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        axes = torch.stack([torch.tensor([2.0, 0.0, -2.0, 0.0], device="cuda")[d],
                            torch.tensor([0.0, 2.0, 0.0, -2.0], device="cuda")[d]], 1).contiguous()
        inputs = {"farn": fwd, "one": one, "axes": axes, "zero": torch.zeros_like(fwd)}

        def geometry(kinds, cell):
            D = (BINS + 1 if kinds & 1 else 0) + (BINS if kinds & 2 else 0) + (BINS if kinds & 4 else 0)
            return D, -(-H // cell), -(-W // cell)

        outs = {}
        for _, k, c, _, _ in FORMS:
            D, CH, CW = geometry(KINDS[k], c)
            outs[(k, c)] = (torch.empty((n, D, CH, CW), device="cuda"), torch.empty((n, CH, CW, D), dtype=torch.int64, device="cuda"))

        def single(name, k, cell, masked, inp):
            D, CH, CW = geometry(KINDS[k], cell)
            out, sums = outs[(k, cell)]
            eng.flow_hist_device(inputs[inp].data_ptr(), W, hw, 2 * hw, n, KINDS[k], cell, BINS, -1.0 if inp == "zero" else THR, 0,
                                 sums.data_ptr(), CH * CW * D, out.data_ptr(), CH * CW, 1, CW, D * CH * CW,
                                 occ.data_ptr() if masked else None, W, hw)

        composed_sums = {}

        def composed(name, k, cell, masked, inp, chunk=8):
            """The same definition from torch ops, eight flows at a time."""
            kinds = KINDS[k]
            D, CH, CW = geometry(kinds, cell)
            flows = inputs[inp]
            thr = -1.0 if inp == "zero" else THR
            res = torch.zeros((n, CH * CW * D), dtype=torch.int64, device="cuda")
            cy = (torch.arange(H, device="cuda") // cell).view(1, H, 1)
            cx = (torch.arange(W, device="cuda") // cell).view(1, 1, W)
            cellbase = (cy * CW + cx) * D
            for i in range(0, n, chunk):
                s = slice(i, i + chunk)
                u, v = flows[s, 0], flows[s, 1]
                known = (u.abs() <= 1e9) & (v.abs() <= 1e9)
                if masked:
                    known &= occ[s] == 0
                u, v = torch.where(known, u, 0.0), torch.where(known, v, 0.0)
                base = 0
                for bit in (1, 2, 4):
                    if not kinds & bit:
                        continue
                    if bit == 1:
                        gx, gy, part = u, v, known
                    else:
                        p = u if bit == 2 else v
                        gx = torch.cat([p[:, :, 1:], p[:, :, -1:]], 2) - torch.cat([p[:, :, :1], p[:, :, :-1]], 2)
                        gy = torch.cat([p[:, 1:], p[:, -1:]], 1) - torch.cat([p[:, :1], p[:, :-1]], 1)
                        part = known & torch.cat([known[:, :, 1:], known[:, :, -1:]], 2) & torch.cat([known[:, :, :1], known[:, :, :-1]], 2) \
                            & torch.cat([known[:, 1:], known[:, -1:]], 1) & torch.cat([known[:, :1], known[:, :-1]], 1)
                    m = torch.sqrt(gx * gx + gy * gy)
                    Q = torch.round(m * 256.0).long()
                    fk = torch.atan2(gy, gx) / torch.pi * (0.5 * BINS)
                    fk = torch.where(fk < 0, fk + BINS, fk)
                    k0 = fk.floor()
                    f = fk - k0
                    k0 = k0.long()
                    wrap = k0 >= BINS
                    k0 = torch.where(wrap, 0, k0)
                    f = torch.where(wrap, 0.0, f)
                    k1 = torch.where(k0 + 1 == BINS, 0, k0 + 1)
                    w1 = (Q * torch.round(f * 256.0).long() + 128) >> 8
                    w0 = Q - w1
                    if bit == 1:
                        still = part & (m <= thr)
                        k0 = torch.where(still, BINS, k0)
                        w0 = torch.where(still, 256, w0)
                        w1 = torch.where(still, 0, w1)
                    w0, w1 = torch.where(part, w0, 0), torch.where(part, w1, 0)
                    r = res[s]
                    r.scatter_add_(1, (cellbase + base + k0).reshape(r.shape[0], -1), w0.reshape(r.shape[0], -1))
                    r.scatter_add_(1, (cellbase + base + k1).reshape(r.shape[0], -1), w1.reshape(r.shape[0], -1))
                    base += BINS + 1 if bit == 1 else BINS
            composed_sums[name] = res.view(n, CH, CW, D)

        def model_bytes(masked):
            return 8 + (1 if masked else 0)

        copies = {}
        for masked in (False, True):
            half = hw * n * model_bytes(masked) // 2
            copies[masked] = (torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda"))
        paths = [("single", single), ("copy", lambda name, k, c, masked, inp: copies[masked][1].copy_(copies[masked][0]))]
        if not args.no_torch_path:
            paths.append(("composed", composed))
        times = {(path, f[0]): [] for f in FORMS for path, _ in paths}
        for r in range(args.rounds + 1):
            for f in FORMS:
                for path, fn in paths:
                    if path == "composed" and r > 2:  # the composed path is slow and steady: two timed windows of one call
                        continue
                    dt_ms = window(lambda: fn(*f), args.calls if path != "composed" else 1)
                    if r:  # round 0 warms every form
                        times[(path, f[0])].append(dt_ms)
        for f in FORMS:
            name, k, cell, masked, inp = f
            D, CH, CW = geometry(KINDS[k], cell)
            model = model_bytes(masked) * hw * n
            row = dict(label=args.label, form=name, kinds=k, cell=cell, bins=BINS, masked=masked, input=inp, flows=n, slots=D,
                       calls_per_window=args.calls, model_bytes_per_pixel=model_bytes(masked),
                       output_bytes_per_pixel=round(D * 12 / (cell * cell), 3))
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
                sums = outs[(k, cell)][1]
                diff = (sums - composed_sums.pop(name)).abs()
                row["composed_over_single"] = row["composed"]["us_per_flow"] / row["single"]["us_per_flow"]
                row["composed_differs_in_sums"] = int((diff != 0).sum())
                row["composed_max_abs_difference"] = int(diff.max())
                row["composed_total_abs_difference_over_total"] = float(diff.sum().double() / sums.sum().double().clamp(min=1))
                row["sums_compared"] = diff.numel()
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
