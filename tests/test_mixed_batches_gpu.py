"""TVL1 parity for device batches that mix stragglers with easy pairs.

The TVL1 engine runs a device batch in lockstep, one pyramid level at a time: every pair has its own state machine on the
device (tvl1_ctrl.h), finish_level (tvl1_device_common.h) counts the pairs out of a level, and the host keeps enqueueing
step launches until the last one has left (tvl1_engine.cpp: run_pairs).  How long a pair iterates depends on its content:
at 224 x 224 a flat pair leaves every warp after the warp-and-head kernel (50 inner iterations), a plain SynthClip pair
after ~550, a hard cut runs to the iteration bound (7500).  Real video mixes these inside one batch, so pairs sit in
LEVEL_DONE for hundreds of speculative steps while one pair is still iterating and others are back in their warp phase.

Every test here builds such batches and holds them against the CPU oracle (the default reading, tvl1_math 0): the flows
bit for bit, and — through the dfxi_tvl1_batch_tables test hook — the executed iteration table and the per-level count
of convergence checks of EVERY pair, not only of the last one (dfx_stats).  Nothing here assumes that the batch runs in
lockstep, and nothing asserts launch counts, no-op steps or timings: those change with how the engine dispatches."""
import collections
import os
import threading

import numpy as np
import pytest

from denseflow_amd.synth import ContentClip, HardClip, SynthClip

pytestmark = pytest.mark.gpu

W, H = 224, 224
NF = 7  # frames per clip of the joined mixed FlowBuffer
STRAGGLER = 7000  # inner iterations (all levels, all warps) of a pair that counts as a straggler here
# Clip order of the joined mixed FlowBuffer: a straggler is its first, a middle and its last pair for every step below.
#   fade        pairs (0,1) .. (3,4) run 6300-7400 iterations; (2,3) / (3,4) evaluate a check on almost every odd one
#   cut         pair (0,1) is a hard cut (7100), (1,0) runs every warp of every level to the bound (7500)
#   cut_rev     the cut clip played backwards: its last pair is the reversed cut
CLIPS = ["fade", "synth", "constant", "hard", "static_noise", "cut", "cartoon", "saturated", "letterbox", "cut_rev"]
SEED = 7
ORACLE_THREADS_1080P = min(16, os.cpu_count() or 1)


def _clip_frames(name, n):
    if name == "synth":
        return SynthClip(W, H, SEED).frames(n)
    if name == "hard":
        return HardClip(W, H, SEED).frames(n)
    if name == "cut_rev":
        return ContentClip(W, H, SEED, "cut").frames(n)[::-1]
    return ContentClip(W, H, SEED, name).frames(n)


def _pairs(n, step):
    """Frame indices (a, b) of the pairs of one clip of n frames, in output order (src/denseflow_gpu.cpp:315-316)."""
    return [(i, i + step) if step > 0 else (i - step, i) for i in range(max(n - abs(step), 0))]


def _table(rows, levels):
    """An iteration table as `levels` rows of DFX_MAX_WARPS entries, zero-padded."""
    rows = [list(r) for r in rows[:levels]]
    return rows + [[0] * len(rows[0])] * (levels - len(rows))


class _Ref:
    """What the oracle says about one pair: flow, iteration table, checks per level, the pyramid's level sizes."""

    def __init__(self, flow, tr):
        self.flow = flow
        self.levels = tr.nscales
        self.table = tr.iters_table()
        by_level = collections.Counter(c[0] for c in tr.checks())
        assert tr.n_checks == sum(by_level.values()), "the oracle's check trace overflowed"
        self.checks = [by_level.get(s, 0) for s in range(tr.nscales)]
        self.total = sum(sum(r) for r in self.table)
        self.px_iters = sum(float(tr.w[s] * tr.h[s]) * sum(self.table[s]) for s in range(tr.nscales))


@pytest.fixture(scope="module")
def ref_of(oracle):
    """Oracle results keyed by the pair's bytes and the reading: each pair is computed once for the whole module."""
    cache = {}
    readings = {0: 0, 2: oracle.VAR_TVL1_SQRT_HYPOT, 3: oracle.VAR_TVL1_LIBM_HYPOT}

    def get(f0, f1, math=0, threads=None):
        key = (f0.tobytes(), f1.tobytes(), math)
        if key not in cache:
            with oracle.variant(readings[math]):
                cache[key] = _Ref(*oracle.tvl1_calc(f0, f1, want_trace=True, threads=threads))
        return cache[key]

    return get


class Mixed:
    """A joined FlowBuffer of clips and, per pair in output order, its frames."""

    def __init__(self, clips, step):
        self.lengths = [len(c) for c in clips]
        self.frames = [f for c in clips for f in c]
        self.pair_frames = [(c[a], c[b]) for c in clips for a, b in _pairs(len(c), step)]
        self.step = step
        self.m = len(self.pair_frames)


@pytest.fixture(scope="module")
def mixed(ref_of):
    """step -> (Mixed, [_Ref per pair]) for the joined mixed clips of NF frames."""
    clips = [_clip_frames(name, NF) for name in CLIPS]
    out = {}
    for step in (1, -1, 2):
        mx = Mixed(clips, step)
        out[step] = (mx, [ref_of(a, b) for a, b in mx.pair_frames])
    return out


def _check_flow(got, want, what):
    assert np.array_equal(got, want), (f"{what}: max-abs {np.max(np.abs(got - want))}, "
                                       f"{np.count_nonzero(got != want)} values differ")


def _check_tables(tables, checks, refs, what, first=0):
    """Per-pair readout of a batch against the oracle (pairs first .. first + len(tables) - 1 of `refs`)."""
    for j, (t, c) in enumerate(zip(tables, checks)):
        r = refs[first + j]
        levels = max(len(t), r.levels)
        assert _table(t, levels) == _table(r.table, levels), f"{what}: pair {first + j}: iteration tables differ"
        assert c + [0] * (levels - len(c)) == r.checks + [0] * (levels - r.levels), \
            f"{what}: pair {first + j}: checks per level {c} vs the oracle's {r.checks}"


def _run(dfx, mx, **knobs):
    with dfx.FlowEngine(W, H, "tvl1", **knobs) as eng:
        eng.next_segments(mx.lengths)
        flows = eng.calc_optflows(mx.frames, mx.step)
        st = eng.stats()
        tables, checks = eng.tvl1_batch_tables()
    return flows, st, tables, checks


# ------------------------------------------------------------------------------------------------------ A

@pytest.mark.parametrize("step", [1, -1, 2])
def test_A_joined_mixed_clips_in_one_device_batch(dfx, mixed, step):
    mx, refs = mixed[step]
    m = mx.m
    # the batch is what it is meant to be: stragglers first, in the middle, last
    assert refs[0].total >= STRAGGLER and refs[-1].total >= STRAGGLER
    assert any(r.total >= STRAGGLER for r in refs[m // 3: 2 * m // 3])
    assert min(r.total for r in refs) <= 100  # ... beside pairs that leave every level at once
    flows, st, tables, checks = _run(dfx, mx)
    assert st.batch >= m, "the joined clips are meant to fit one automatic batch"
    assert st.pairs == m and len(flows) == m and len(tables) == m and len(checks) == m
    for i in range(m):
        _check_flow(flows[i], refs[i].flow, f"step {step} pair {i}")
    _check_tables(tables, checks, refs, f"step {step}")
    assert st.tvl1_total_iters == sum(r.total for r in refs)
    assert st.tvl1_px_iters == sum(r.px_iters for r in refs)  # integers below 2^53: exact in any order
    assert st.tvl1_checks == sum(refs[-1].checks)


# ------------------------------------------------------------------------------------------------------ B

FORMS = ([("impl", {"impl": 1}), ("impl", {"impl": 2})]
         + [("variant", {"variant": v}) for v in ("VAR_TVL1_CLASSIC_GEOM", "VAR_TVL1_WARP_IN_STEP",
                                                  "VAR_TVL1_WARP_GATHER", "VAR_TVL1_NO_HEAD")]
         + [("fuse_k", {"tvl1_fuse_k": k}) for k in (1, 2, 3, 5, 8, 12)]
         + [("step_group", {"step_group": g}) for g in (1, 2, 64)]
         + [("blocking_sync", {"blocking_sync": 1})])


@pytest.mark.parametrize("knobs", [f[1] for f in FORMS], ids=[f"{f[0]}={list(f[1].values())[0]}" for f in FORMS])
def test_B_every_kernel_form_on_the_mixed_batch(dfx, mixed, knobs):
    """Every form is bit-identical to the default run, which test A pins to the oracle: compared with the oracle here."""
    mx, refs = mixed[1]
    knobs = {k: (getattr(dfx.engine, v) if isinstance(v, str) else v) for k, v in knobs.items()}
    flows, st, tables, checks = _run(dfx, mx, **knobs)
    assert st.pairs == mx.m and len(tables) == mx.m
    for i in range(mx.m):
        _check_flow(flows[i], refs[i].flow, f"{knobs} pair {i}")
    _check_tables(tables, checks, refs, f"{knobs}")


@pytest.mark.parametrize("math", [2, 3])
def test_B_hypot_readings_on_stragglers_and_flat_pairs(dfx, ref_of, math):
    """tvl1_math 2 / 3 against the oracle's matching reading: the reversed cut, fade (3,4) and a constant pair, joined."""
    cut = ContentClip(W, H, SEED, "cut").frames(2)
    fade = ContentClip(W, H, SEED, "fade").frames(5)
    const = ContentClip(W, H, SEED, "constant").frames(2)
    clips = [[cut[1], cut[0]], [fade[3], fade[4]], const]
    mx = Mixed(clips, 1)
    refs = [ref_of(a, b, math) for a, b in mx.pair_frames]
    assert refs[0].total >= STRAGGLER and refs[2].total <= 100
    flows, st, tables, checks = _run(dfx, mx, tvl1_math=math)
    assert len(tables) == 3
    for i in range(3):
        _check_flow(flows[i], refs[i].flow, f"math {math} pair {i}")
    _check_tables(tables, checks, refs, f"math {math}")


# ------------------------------------------------------------------------------------------------------ C

def _batches(m, mb):
    return [list(range(i, min(i + mb, m))) for i in range(0, m, mb)]


def test_C_straggler_positions_in_split_batches(dfx, mixed):
    mx, refs = mixed[1]
    m = mx.m
    slow = {i for i, r in enumerate(refs) if r.total >= STRAGGLER}
    sizes = (1, 2, 5, 16, m - 1)
    # the sizes put a straggler first in a batch, last in a full batch, and alone in a ragged final batch
    split = [_batches(m, mb) for mb in sizes]
    assert any(b[0] in slow and len(b) > 1 for bs in split for b in bs)
    assert any(b[-1] in slow and len(b) == mb > 1 for mb, bs in zip(sizes, split) for b in bs)
    assert any(len(bs[-1]) == 1 and len(bs[0]) > 1 and bs[-1][0] in slow for bs in split)
    for mb, bs in zip(sizes, split):
        flows, st, tables, checks = _run(dfx, mx, max_batch=mb)
        assert st.batch == mb and st.pairs == m
        for i in range(m):
            _check_flow(flows[i], refs[i].flow, f"max_batch {mb} pair {i}")
        last = bs[-1]
        assert len(tables) == len(last), f"max_batch {mb}: the readout holds the last batch"
        _check_tables(tables, checks, refs, f"max_batch {mb}", first=last[0])


# ------------------------------------------------------------------------------------------------------ D

def test_D_full_224_batch_of_2048_pairs_batch_mates_independent(dfx, ref_of):
    """64 clips x 33 frames through the device-resident path.  Replacing 4 clips by stragglers changes nothing for the
    60 others: their flows and tables are bit-identical to the all-plain run."""
    import torch

    dev = torch.device("cuda", 0)
    n_clips, nf = 64, 33
    m = n_clips * (nf - 1)
    plain = [SynthClip(W, H, 3000 + i) for i in range(n_clips)]
    alt = (SynthClip(W, H, 4001), SynthClip(W, H, 4002))  # unrelated: every pair of the alternating clip is a cut
    replaced = {
        5: ContentClip(W, H, SEED, "cut").frames(nf),
        23: ContentClip(W, H, SEED, "fade").frames(nf),
        41: [alt[t % 2].frame(t) for t in range(nf)],
        62: [alt[(t + 1) % 2].frame(t) for t in range(nf)],
    }

    def run(clips):
        d_frames = torch.cat(clips).contiguous()
        d_flows = torch.empty((m, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with dfx.FlowEngine(W, H, "tvl1") as eng:
            eng.next_segments([nf] * n_clips)
            eng.calc_optflows_device(d_frames.data_ptr(), W, W * H, n_clips * nf, 1, d_flows.data_ptr(), W * H * 2)
            st = eng.stats()
            tables, checks = eng.tvl1_batch_tables()
        assert st.batch == m and st.pairs == m and len(tables) == m
        return d_frames, d_flows, tables, checks

    base = [c.frames_torch(nf, dev) for c in plain]
    _, flows1, tables1, checks1 = run(base)
    mixed_clips = list(base)
    for ci, fr in replaced.items():
        mixed_clips[ci] = torch.from_numpy(np.stack(fr)).to(dev)
    d_frames2, flows2, tables2, checks2 = run(mixed_clips)

    same = (flows1.view(torch.int32) == flows2.view(torch.int32)).view(m, -1).all(dim=1).cpu().numpy()
    del flows1
    touched = {ci * (nf - 1) + j for ci in replaced for j in range(nf - 1)}
    for i in range(m):
        if i not in touched:
            assert same[i], f"pair {i} of an untouched clip changed when its batch mates did"
            assert tables1[i] == tables2[i] and checks1[i] == checks2[i], f"pair {i}: tables changed"
    # three stragglers, the first and the last pair of the batch, against the oracle
    picks = [0, 5 * (nf - 1), 23 * (nf - 1) + 3, 41 * (nf - 1) + 17, m - 1]
    for i in picks:
        ci, j = divmod(i, nf - 1)
        f0 = d_frames2[ci * nf + j].cpu().numpy()
        f1 = d_frames2[ci * nf + j + 1].cpu().numpy()
        r = ref_of(f0, f1)
        if i in touched and i != 23 * (nf - 1) + 3:
            assert r.total >= STRAGGLER, f"pair {i} was meant to be a straggler"
        _check_flow(flows2[i].cpu().numpy(), r.flow, f"2048-pair batch, pair {i}")
        _check_tables(tables2[i:i + 1], checks2[i:i + 1], [r], f"2048-pair batch, pair {i}")


# ------------------------------------------------------------------------------------------------------ E

def test_E_1080p_automatic_batch_with_one_replaced_frame(dfx, ref_of):
    """bench.py's headline clip (130 frames of SynthClip(1920, 1080, 2)) with frame 64 from an unrelated clip: pairs 63
    and 64 are hard cuts, the other 127 flows and tables are those of the unmodified run."""
    import torch

    w, h, n = 1920, 1080, 130
    dev = torch.device("cuda", 0)
    d_plain = SynthClip(w, h, 2).frames_torch(n, dev)
    d_cut = d_plain.clone()
    d_cut[64] = SynthClip(w, h, 77).frames_torch(1, dev, start=64)[0]

    def run(d_frames):
        d_flows = torch.empty((n - 1, h, w, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with dfx.FlowEngine(w, h, "tvl1") as eng:
            eng.calc_optflows_device(d_frames.data_ptr(), w, w * h, n, 1, d_flows.data_ptr(), w * h * 2)
            st = eng.stats()
            tables, checks = eng.tvl1_batch_tables()
        assert st.batch == n - 1 and len(tables) == n - 1
        return d_flows, tables, checks

    flows1, tables1, checks1 = run(d_plain)
    flows2, tables2, checks2 = run(d_cut)
    same = (flows1.view(torch.int32) == flows2.view(torch.int32)).view(n - 1, -1).all(dim=1).cpu().numpy()
    del flows1
    for i in range(n - 1):
        if i not in (63, 64):
            assert same[i], f"flow {i} changed when frame 64 was replaced"
            assert tables1[i] == tables2[i] and checks1[i] == checks2[i], f"pair {i}: tables changed"
    for i in (63, 64):
        f0, f1 = d_cut[i].cpu().numpy(), d_cut[i + 1].cpu().numpy()
        r = ref_of(f0, f1, threads=ORACLE_THREADS_1080P)
        assert r.total > 3 * sum(map(sum, tables2[0])), f"pair {i} was meant to be a straggler"
        _check_flow(flows2[i].cpu().numpy(), r.flow, f"1080p pair {i}")
        _check_tables(tables2[i:i + 1], checks2[i:i + 1], [r], f"1080p pair {i}")


# ------------------------------------------------------------------------------------------------------ F

def test_F_submit_two_flowbuffers_the_first_ending_on_a_straggler(dfx, mixed):
    mx, refs = mixed[1]
    assert refs[-1].total >= STRAGGLER
    plain = SynthClip(W, H, 21).frames(9)
    with dfx.FlowEngine(W, H, "tvl1", max_batch=16) as eng:
        want = eng.calc_optflows(plain, 1)
        eng.next_segments(mx.lengths)
        t1, got1 = eng.submit_optflows(mx.frames, 1)
        t2, got2 = eng.submit_optflows(plain, 1)
        eng.wait(t1)
        eng.wait(t2)
    for i in range(mx.m):
        _check_flow(got1[i], refs[i].flow, f"submitted mixed FlowBuffer pair {i}")
    for i in range(len(want)):
        _check_flow(got2[i], want[i], f"submitted plain FlowBuffer pair {i}")


def test_F_two_handles_in_two_threads(dfx, mixed):
    """One handle iterates the stragglers while another finishes plain pairs: the level bookkeeping (d_level_done,
    h_done_flag, done_token) is per handle."""
    mx, refs = mixed[1]
    plain = [f for s in range(4) for f in SynthClip(W, H, 50 + s).frames(9)]
    with dfx.FlowEngine(W, H, "tvl1") as eng:
        eng.next_segments([9] * 4)
        want_plain = eng.calc_optflows(plain, 1)
        tables_plain, checks_plain = eng.tvl1_batch_tables()
    results, errors = {}, []

    def work(name):
        try:
            with dfx.FlowEngine(W, H, "tvl1") as eng:
                for _ in range(2):
                    if name == "mixed":
                        eng.next_segments(mx.lengths)
                        flows = eng.calc_optflows(mx.frames, 1)
                    else:
                        eng.next_segments([9] * 4)
                        flows = eng.calc_optflows(plain, 1)
                    results.setdefault(name, []).append((flows, eng.tvl1_batch_tables()))
        except Exception as e:  # reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(n,)) for n in ("mixed", "plain")]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for flows, (tables, checks) in results["mixed"]:
        for i in range(mx.m):
            _check_flow(flows[i], refs[i].flow, f"mixed handle pair {i}")
        _check_tables(tables, checks, refs, "mixed handle")
    for flows, (tables, checks) in results["plain"]:
        for i in range(len(want_plain)):
            _check_flow(flows[i], want_plain[i], f"plain handle pair {i}")
        assert tables == tables_plain and checks == checks_plain


# ------------------------------------------------------------------------------------------------------ G

@pytest.mark.parametrize("batch", [0, 3])
@pytest.mark.parametrize("algo", ["farn", "brox"])
def test_G_farneback_and_brox_on_the_joined_mixed_clips(dfx, oracle, algo, batch):
    """Farneback's row segments and Brox's persistent SOR workgroups across pairs of different classes in one launch;
    3 frames (2 pairs) per clip of the mixed FlowBuffer."""
    clips = [_clip_frames(name, 3) for name in CLIPS]
    mx = Mixed(clips, 1)
    calc = {"farn": oracle.farneback_calc, "brox": oracle.brox_calc}[algo]
    knobs = {"max_batch": batch} if batch else {}
    with dfx.FlowEngine(W, H, algo, **knobs) as eng:
        eng.next_segments(mx.lengths)
        flows = eng.calc_optflows(mx.frames, 1)
        st = eng.stats()
    assert st.pairs == mx.m and (batch or st.batch >= mx.m)
    for i, (a, b) in enumerate(mx.pair_frames):
        _check_flow(flows[i], calc(a, b), f"{algo} batch {batch} pair {i}")


# ------------------------------------------------------------------------------------------------------ the hook

def test_the_batch_tables_hook_agrees_with_the_stats_and_refuses_what_it_cannot_answer(dfx):
    import ctypes as C

    L = dfx.load_library()
    it = (C.c_int * (8 * dfx.engine.DFX_MAX_LEVELS * dfx.engine.DFX_MAX_WARPS))()
    ck = (C.c_int * (8 * dfx.engine.DFX_MAX_LEVELS))()
    frames = SynthClip(64, 48, 3).frames(6)
    with dfx.FlowEngine(64, 48, "farn") as eng:
        eng.calc_optflows(frames, 1)
        assert L.dfxi_tvl1_batch_tables(eng._h, 8, it, ck) == -dfx.engine.ERR_UNSUPPORTED
    with dfx.FlowEngine(64, 48, "tvl1", max_batch=4) as eng:
        assert L.dfxi_tvl1_batch_tables(eng._h, 8, it, ck) == -dfx.engine.ERR_INVALID  # before any batch
        eng.calc_optflows(frames, 1)  # 5 pairs: a batch of 4, then one of 1
        st = eng.stats()
        assert L.dfxi_tvl1_batch_tables(eng._h, 0, it, ck) == -dfx.engine.ERR_INVALID  # max_pairs too small
        tables, checks = eng.tvl1_batch_tables()
        assert len(tables) == 1 and tables[0] == st.iters_table() and sum(checks[0]) == st.tvl1_checks
        eng.calc_optflows(frames[:5], 1)  # 4 pairs: one full batch
        st = eng.stats()
        tables, checks = eng.tvl1_batch_tables()
        assert len(tables) == 4 and tables[-1] == st.iters_table() and sum(checks[-1]) == st.tvl1_checks
