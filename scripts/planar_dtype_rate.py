#!/usr/bin/env python3
"""Rates of the typed planar output and cost of the source layouts (profiles/planar_dtype/README.md).

    python scripts/planar_dtype_rate.py [--parent PATH/libdfx.so] [--reps 5] [--frames 300] [--out FILE.json]

One process, one device.  Per algorithm (farn, tvl1) and form (host: pinned host frames in, pinned host planes out,
PCIe-inclusive; resident: frames and planes in HBM) the variants are alternated `reps` times after one warm-up of each:

    parent_a / parent_b  the PARENT commit's dfx_calc_batch_planar(_device), from the library given with --parent, twice per
                         round: their difference is the run-to-run spread the float32 typed entry must sit inside
    f32                  dfx_calc_batch_planar_as(_device) with DFX_PLANAR_F32
    f16 / bf16           the same with DFX_PLANAR_F16 / DFX_PLANAR_BF16

and the preparation launch is timed for BGR interleaved (this tree's kernel and the parent's), RGB channels-first, and RGB channels-first flipped and permuted
to BGR interleaved in torch first, at 1080p -> 1080p and 2160p -> 1080p.  A rate is pairs / wall time of the call, the
device synchronised at both ends.  Prints one JSON document; every variant's output is compared with the float32 one
on a sample (bit-equal for f32, the restatement of tests/reduced_ref.py for the half types)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import denseflow_amd  # noqa: E402
from denseflow_amd import engine as E  # noqa: E402
from denseflow_amd.synth import SynthClip  # noqa: E402
from tests import reduced_ref as R  # noqa: E402

W, H = 1920, 1080


def engine_on(lib_path, algo):
    """A FlowEngine bound to the library at lib_path (None: this tree's)."""
    if lib_path is None:
        return denseflow_amd.FlowEngine(W, H, algo)
    mine, env = E._lib, os.environ.get("DFX_LIBRARY")
    E._lib, os.environ["DFX_LIBRARY"] = None, lib_path
    try:
        return denseflow_amd.FlowEngine(W, H, algo)  # binds E.load_library()'s CDLL of lib_path
    finally:
        E._lib = mine
        if env is None:
            del os.environ["DFX_LIBRARY"]
        else:
            os.environ["DFX_LIBRARY"] = env


def summary(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1), "n": len(xs)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def flow_rates(algo, n_frames, reps, parent):
    m = n_frames - 1
    clip = SynthClip(W, H, seed=2)
    d_frames = clip.frames_torch(n_frames, torch.device("cuda:0"))
    h_frames = torch.empty((n_frames, H, W), dtype=torch.uint8, pin_memory=True)
    h_frames.copy_(d_frames)
    h_out = torch.empty((m, 2, H, W), dtype=torch.float32, pin_memory=True)
    d_out = torch.empty((m, 2, H, W), dtype=torch.float32, device="cuda")
    fp = (C.c_void_p * n_frames)(*[h_frames[i].data_ptr() for i in range(n_frames)])
    plane = W * H

    def host_ptrs(elem):
        base = h_out.data_ptr()
        up = (C.c_void_p * m)(*[base + (2 * k) * plane * elem for k in range(m)])
        vp = (C.c_void_p * m)(*[base + (2 * k + 1) * plane * elem for k in range(m)])
        return up, vp

    engines = {"this": engine_on(None, algo)}
    if parent:
        engines["parent"] = engine_on(parent, algo)
    out = {}
    try:
        def ok(rc, eng):
            if rc != 0:
                raise RuntimeError(eng._L.dfx_last_error(eng._h).decode())

        def variant(name, form):
            eng = engines["parent" if name.startswith("parent") else "this"]
            L, h = eng._L, eng._h
            code = {"f32": 0, "f16": 1, "bf16": 2}.get(name)
            elem = 2 if code in (1, 2) else 4
            if form == "host":
                up, vp = host_ptrs(elem)
                if code is None:
                    return lambda: ok(L.dfx_calc_batch_planar(h, fp, W, n_frames, 1, 0.0, up, vp, W * 4), eng)
                return lambda: ok(L.dfx_calc_batch_planar_as(h, fp, W, n_frames, 1, 0.0, code, up, vp, W * elem), eng)
            if code is None:
                return lambda: ok(L.dfx_calc_batch_planar_device(h, d_frames.data_ptr(), W, plane, n_frames, 1, 0.0,
                                                                 d_out.data_ptr(), W, plane, 2 * plane), eng)
            return lambda: ok(L.dfx_calc_batch_planar_as_device(h, d_frames.data_ptr(), W, plane, n_frames, 1, 0.0, code,
                                                                d_out.data_ptr(), W, plane, 2 * plane), eng)

        names = (["parent_a"] if parent else []) + ["f32", "f16", "bf16"] + (["parent_b"] if parent else [])
        for form in ("host", "resident"):
            calls = {n: variant(n, form) for n in names}
            ref = None
            checks = {}
            for n in names:  # warm-up of every variant, and what it computes
                calls[n]()
                torch.cuda.synchronize()
                src = h_out if form == "host" else d_out
                if n in ("f16", "bf16"):  # the typed planes are dense in the first half of the buffer
                    bits = src.view(torch.int16).reshape(-1)[:2 * m * plane].reshape(m, 2, H, W)[::37, :, ::9].cpu().numpy()
                    want = R.reduce_bits(ref, "float16" if n == "f16" else "bfloat16")
                    checks[n] = bool(np.array_equal(bits.view(np.uint16), want))
                else:  # (a sample: every 37th flow, every 9th row)
                    got = src[::37, :, ::9].cpu().numpy().copy()
                    if ref is None:
                        ref = got
                    checks[n] = bool(np.array_equal(got.view(np.uint32), ref.view(np.uint32)))
            rates = {n: [] for n in names}
            for _ in range(reps):
                for n in names:
                    rates[n].append(m / timed(calls[n]))
            out[form] = {"rates_pairs_per_s": {n: summary(v) for n, v in rates.items()}, "same_values": checks}
    finally:
        for e in engines.values():
            e.close()
    return out


def prepare_costs(reps, parent):
    out = {}
    old = engine_on(parent, "farn") if parent else None  # (the parent's preparation kernel: BGR interleaved only)
    with denseflow_amd.FlowEngine(W, H, "farn", max_batch=1) as eng:
        for ws, hs, n in ((1920, 1080, 32), (3840, 2160, 16)):
            rng = torch.Generator(device="cuda").manual_seed(3)
            rgb_chw = torch.randint(0, 256, (n, 3, hs, ws), dtype=torch.uint8, device="cuda", generator=rng)
            bgr_hwc = rgb_chw.flip(1).permute(0, 2, 3, 1).contiguous()
            gray = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(4)]

            def bgr():
                eng.prepare_frames_device(bgr_hwc.data_ptr(), 3 * ws, 3 * ws * hs, ws, hs, 3, n, gray[0].data_ptr(), W, W * H)

            def chw():
                eng.prepare_frames_layout_device(rgb_chw.data_ptr(), ws, 3 * ws * hs, 0, ws, hs, 3, "rgb", "chw", n,
                                                 gray[1].data_ptr(), W, W * H)

            def torch_first():
                t = rgb_chw.flip(1).permute(0, 2, 3, 1).contiguous()
                torch.cuda.synchronize()
                eng.prepare_frames_device(t.data_ptr(), 3 * ws, 3 * ws * hs, ws, hs, 3, n, gray[2].data_ptr(), W, W * H)

            def bgr_parent():
                old.prepare_frames_device(bgr_hwc.data_ptr(), 3 * ws, 3 * ws * hs, ws, hs, 3, n, gray[3].data_ptr(), W, W * H)

            calls = {"bgr_interleaved": bgr, "rgb_channels_first": chw, "torch_flip_permute_then_bgr": torch_first}
            if old is not None:
                calls = {"bgr_interleaved_parent": bgr_parent, **calls}
            for f in calls.values():
                f()
            us = {k: [] for k in calls}
            for _ in range(reps):
                for k, f in calls.items():
                    us[k].append(timed(f) * 1e6 / n)
            same = bool(torch.equal(gray[0], gray[1]) and torch.equal(gray[0], gray[2]) and
                        (old is None or torch.equal(gray[0], gray[3])))
            out[f"{ws}x{hs}"] = {"us_per_frame": {k: summary(v) for k, v in us.items()}, "same_gray": same, "frames": n}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libdfx.so (the float32 comparator)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--algos", default="farn,tvl1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {"size": [W, H], "frames": a.frames, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "parent": bool(a.parent)}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)

    doc["prepare"] = prepare_costs(max(a.reps, 5), a.parent)
    dump()
    for algo in [x for x in a.algos.split(",") if x]:
        doc[algo] = flow_rates(algo, a.frames, a.reps, a.parent)
        dump()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
