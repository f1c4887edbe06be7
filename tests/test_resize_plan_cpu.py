"""CPU test of the engines' plans (denseflow_amd/csrc/engine_plan.h, the header every *_engine.cpp compiles): the geometry an
engine derives from (W, H, params) is host arithmetic, and dfx_set_size re-plans an engine object that already holds the
plan of another size.  A plan after another plan must equal the plan from scratch, field by field — the level count
changes with the size (TVL1 2..5, Brox 2..24 levels; Farneback's taps table has one run per level), so anything left
over from the previous size would show.  The TVL1 and Brox level tables are held against the CPU oracle's pyramids."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_py

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = [(96, 64), (65, 33), (224, 224), (64, 64), (20, 20), (130, 70), (1920, 1080), (3840, 2160)]
CAP = 4096


@pytest.fixture(scope="module")
def rp():
    out_dir = os.path.join(HERE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libresize_plan_harness.%d.so" % os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "resize_plan_harness.cpp")],
                   check=True, capture_output=True)
    L = C.CDLL(so)
    os.unlink(so)
    L.rp_fit_batch.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
    return L


def _plan(L, name, w0, h0, w, h, max_batch=0):
    out = (C.c_longlong * CAP)()
    n = getattr(L, "rp_" + name)(w0, h0, w, h, max_batch, out, CAP)
    assert 0 < n <= CAP
    return list(out[:n])


@pytest.mark.parametrize("name", ["tvl1", "farn", "brox"])
def test_plan_after_another_plan_is_the_plan_from_scratch(rp, name):
    scratch = {s: _plan(rp, name, 0, 0, *s) for s in SIZES}
    assert len({tuple(v) for v in scratch.values()}) == len(SIZES)  # the fields do depend on the size
    for prev in SIZES:
        for s in SIZES:
            assert _plan(rp, name, *prev, *s) == scratch[s], (name, prev, s)
    assert _plan(rp, name, 3840, 2160, 20, 20, max_batch=7) == _plan(rp, name, 0, 0, 20, 20, max_batch=7)


def _tvl1_levels(plan):
    n = plan[2]
    return [(plan[3 + 4 * s], plan[4 + 4 * s]) for s in range(n)], [plan[5 + 4 * s] for s in range(n)]


@pytest.mark.parametrize("size", SIZES)
def test_tvl1_levels_are_the_oracles_pyramid(rp, size):
    w, h = size
    p = oracle_py.tvl1_default_params()
    p.warps, p.iterations = 1, 1  # the pyramid does not depend on them; the oracle run stays short
    z = np.zeros((h, w), np.uint8)
    _, tr = oracle_py.tvl1_calc(z, z, p, want_trace=True)
    levels, pitches = _tvl1_levels(_plan(rp, "tvl1", 0, 0, w, h))
    assert levels == [(tr.w[s], tr.h[s]) for s in range(tr.nscales)]
    assert all(pt % 64 == 0 and 0 <= pt - lw < 64 for pt, (lw, _) in zip(pitches, levels))


def test_level_counts_cross_the_boundaries_the_gpu_tests_aim_at(rp):
    n = {s: _plan(rp, "tvl1", 0, 0, *s)[2] for s in SIZES}
    assert n[(20, 20)] == 2 and n[(65, 33)] == 4 and n[(96, 64)] == 5 and n[(3840, 2160)] == 5
    assert _plan(rp, "farn", 0, 0, 20, 20)[2] == 1 and _plan(rp, "farn", 0, 0, 1920, 1080)[2] == 6


@pytest.mark.parametrize("size", SIZES)
def test_brox_levels_are_the_oracles_pyramid(rp, size):
    plan = _plan(rp, "brox", 0, 0, *size)
    n = plan[2]
    assert [(plan[3 + 4 * l], plan[4 + 4 * l]) for l in range(n)] == oracle_py.brox_pyramid_sizes(*size)


def test_batch_rules(rp):
    # the automatic batch: 256 Mpx of frames, at most 2048 pairs; max_batch wins; the free-memory rule halves
    assert _plan(rp, "tvl1", 0, 0, 1920, 1080)[-3] == 129
    assert _plan(rp, "tvl1", 0, 0, 224, 224)[-3] == 2048
    assert _plan(rp, "tvl1", 0, 0, 224, 224, max_batch=5)[-3] == 5
    assert rp.rp_fit_batch(129, 1 << 20, 1 << 40) == 129
    assert rp.rp_fit_batch(129, 1 << 30, 40 << 30) == 16  # 18 pairs x 1 GiB fit half of 40 GiB, 34 do not
    assert rp.rp_fit_batch(129, 1 << 30, 1 << 20) == 1
    assert rp.rp_frames_batch(1920, 1080, 0) == 16 and rp.rp_frames_batch(48, 32, 0) == 256 and rp.rp_frames_batch(48, 32, 3) == 3
    # TVL1's 4 GiB pair-slot rule is part of the plan: refused before anything is allocated
    assert _plan(rp, "tvl1", 0, 0, 8192, 8192)[-1] == 1 and _plan(rp, "tvl1", 0, 0, 8192, 8191)[-1] == 0
    assert _plan(rp, "tvl1", 0, 0, 8129, 8192)[-1] == 1 and _plan(rp, "tvl1", 0, 0, 8128, 8192)[-1] == 0


@pytest.mark.parametrize("step", [1, -1, 2, -3])
def test_pairs_stay_inside_clips_whatever_their_sizes(rp, step):
    """Clips of different frame sizes joined into one FlowBuffer: the pair rule knows clip lengths only, and no pair may
    take its two frames from two clips."""
    seg = [4, 3, 1, 0, 6]
    start = np.concatenate([[0], np.cumsum(seg)])
    clip_of = np.repeat(np.arange(len(seg)), seg)
    cap = sum(seg) + 1
    lo, hi = (C.c_int * cap)(), (C.c_int * cap)()
    m = rp.rp_pairs((C.c_int * len(seg))(*seg), len(seg), step, lo, hi, cap)
    assert m == sum(max(n - abs(step), 0) for n in seg)
    want = [(int(start[s]) + i, int(start[s]) + i + abs(step)) for s, n in enumerate(seg) for i in range(max(n - abs(step), 0))]
    assert [(lo[i], hi[i]) for i in range(m)] == want
    assert all(clip_of[lo[i]] == clip_of[hi[i]] for i in range(m))


@pytest.mark.parametrize("step", [1, -2, 3])
@pytest.mark.parametrize("batch", [1, 3, 64])
def test_format_runs_keep_every_frame_in_its_clips_format(rp, step, batch):
    """dfx_next_segments_src: the frames a batch brings in are prepared in runs of one source size.  No run may hold
    frames of two sizes (a frame resized with another clip's geometry is wrong bits), every frame some pair needs is in
    exactly one run, in order, and neighbouring clips of one size share a launch."""
    seg = [4, 3, 1, 0, 5, 2, 6]
    sizes = [(32, 24), (64, 48), (33, 47), (9, 9), (33, 47), (33, 47), (32, 24)]
    clip_of = np.repeat(np.arange(len(seg)), seg)
    wh = [v for s in sizes for v in s]
    cap = 4 * (sum(seg) + 8)
    out = (C.c_longlong * cap)()
    rows = rp.rp_format_runs((C.c_int * len(seg))(*seg), (C.c_int * len(wh))(*wh), len(seg), step, batch, out, cap // 4)
    runs = [tuple(out[4 * k:4 * k + 4]) for k in range(rows)]
    seen = []
    for b, first, n, clip in runs:
        assert n > 0
        ids = list(range(first, first + n))
        assert all(sizes[clip_of[f]] == sizes[clip] for f in ids), (b, first, n, clip)
        seen += ids
    assert seen == sorted(set(seen))  # once each, in order
    a = abs(step)
    needed = sorted({f for s, n in enumerate(seg) for i in range(max(n - a, 0))
                     for f in (int(np.sum(seg[:s])) + i, int(np.sum(seg[:s])) + i + a)})
    assert set(needed) <= set(seen)
    # consecutive runs of one batch differ in size: clips 4 and 5 (both 33 x 47) are never split inside a batch
    for (b0, f0, n0, c0), (b1, f1, n1, c1) in zip(runs, runs[1:]):
        if b0 == b1 and f0 + n0 == f1:
            assert sizes[c0] != sizes[c1]
