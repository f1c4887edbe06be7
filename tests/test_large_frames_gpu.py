"""Frames above 4K, GPU vs oracle: where a pair's TVL1 work planes cross the 2^31 and 2^32 byte lines.

The TVL1 tile kernels address a pair slot through a buffer descriptor (tvl1_device_common.h): slot base in the descriptor,
plane offset in a 32-bit scalar offset, pixel offset in a 32-bit vector offset.  At 8192 x 8191, the largest 8192-wide frame
the engine accepts, the slot is 4 294 443 008 bytes: planes 8-15 start above 2^31 and the slot ends 512 KiB short of 2^32.
With max_batch = 2 the second pair's slot starts 4.29 GB into the plane allocation.  A signed offset or range check there
would not fault; it would read zeros or drop stores in the upper planes, so these tests compare every bit with the oracle.
DCI 8K (8192 x 4320) is a real frame size: plane 15 crosses 2^31 inside the slot, and Farneback and Brox (27 pyramid levels)
run there too.

Frames come from a separable generator (sums of products of 1-D sinusoids: one small matrix product per frame), moving by a
constant sub-pixel translation; SynthClip would take minutes per frame pair at these sizes.  The oracle runs on
OMP_NUM_THREADS threads, the 8192 x 8191 flows once per module (the whole file: about 80 s on a 16-thread allowance).
"""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS = int(os.environ.get("OMP_NUM_THREADS", 16))
W, H = 8192, 8191      # slot 16 x 4 x 8192 x 8191 B: 2^32 - 512 KiB
DCI_W, DCI_H = 8192, 4320
BOUND = 2.0            # tight enough that the bounded planes clamp to 0 and 255


def _frames(w, h, n, seed=8, velocity=(1.3, -0.6), terms=12):
    """n uint8 frames of sum_k a_k sin(2 pi (x - vx t) / lx_k + px_k) sin(2 pi (y - vy t) / ly_k + py_k), wavelengths
    log-uniform in [6, 160] px, mapped to [16, 240]."""
    rng = np.random.default_rng(seed)
    lx = np.exp(rng.uniform(math.log(6.0), math.log(160.0), terms))
    ly = np.exp(rng.uniform(math.log(6.0), math.log(160.0), terms))
    px, py = rng.uniform(0.0, 2.0 * math.pi, terms), rng.uniform(0.0, 2.0 * math.pi, terms)
    amp = (lx * ly) ** 0.25
    x, y = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    out = []
    for t in range(n):
        cx = np.sin(2.0 * math.pi * (x[None, :] - velocity[0] * t) / lx[:, None] + px[:, None])         # (terms, w)
        cy = np.sin(2.0 * math.pi * (y[:, None] - velocity[1] * t) / ly[None, :] + py[None, :]) * amp   # (h, terms)
        out.append(np.rint(128.0 + 112.0 * (cy @ cx) / amp.sum()).astype(np.uint8))
    return out


def _iters(stats):
    return [r[:5] for r in stats.iters_table()]


# ---------------------------------------------------------------------------------------------- the refusal boundary

@pytest.mark.parametrize("w,h", [(8192, 8192), (8129, 8192)])
def test_tvl1_refuses_a_pair_slot_of_4_gib(dfx, w, h):
    """round_up(w, 64) x h x 64 B reaches 2^32: exactly 4 GiB for both (8129 pads to a pitch of 8192)."""
    with pytest.raises(dfx.DfxError, match="too large"):
        dfx.FlowEngine(w, h, "tvl1", max_batch=1)


@pytest.mark.parametrize("w,h", [(8128, 8192), (8192, 8191)])
def test_tvl1_accepts_a_pair_slot_just_below_4_gib(dfx, w, h):
    dfx.FlowEngine(w, h, "tvl1", max_batch=1).close()


# ---------------------------------------------------------------------------------------------- TVL1 at 8192 x 8191

@pytest.fixture(scope="module")
def big_frames():
    return _frames(W, H, 3)


@pytest.fixture(scope="module")
def big_oracle(oracle, big_frames):
    return [oracle.tvl1_calc(big_frames[i], big_frames[i + 1], want_trace=True, threads=THREADS) for i in range(2)]


@pytest.fixture(scope="module")
def big_default(dfx, big_frames):
    """The default engine on both pairs in ONE batch: flows, the last pair's iteration table and check count, batch."""
    with dfx.FlowEngine(W, H, "tvl1", max_batch=2) as eng:
        flows = eng.calc_optflows(big_frames, 1)
        st = eng.stats()
        return flows, _iters(st), st.tvl1_checks, st.batch


def test_tvl1_8192x8191_two_pairs_in_one_batch_match_oracle(big_oracle, big_default):
    flows, iters, checks, batch = big_default
    assert batch == 2  # pair 1's slot starts 4.29 GB into the plane allocation
    for i, (out, (ref, _)) in enumerate(zip(flows, big_oracle)):
        assert np.array_equal(out, ref), f"pair {i}: max-abs {np.max(np.abs(out - ref))}, " \
                                         f"{np.count_nonzero(out != ref)} values differ"
    tr = big_oracle[1][1]  # the stats describe the last pair
    assert iters == [r[:5] for r in tr.iters_table()]
    assert checks == tr.n_checks
    assert iters[0][0] > 2  # level 0 ran well past the head kernel's iterations: the step kernel's planes were used


def test_tvl1_8192x8191_every_kernel_form_is_the_default(dfx, big_frames, big_default):
    """The kernel forms test_tvl1_gpu.py holds bit-identical at small sizes, at the largest accepted frame.  impl 1 and 2
    address the planes through 64-bit pointers, so they cross-check the buffer path independently; they go first."""
    from denseflow_amd import engine as E

    base, base_iters = big_default[0], big_default[1]
    forms = [dict(impl=1), dict(impl=2)]
    forms += [dict(variant=E.VAR_TVL1_CLASSIC_GEOM)]
    for variant, ks in ((0, (1, 2, 3, 4, 6)), (E.VAR_TVL1_WARP_GATHER, (4, 3)), (E.VAR_TVL1_WARP_IN_STEP, (2, 4)),
                        (E.VAR_TVL1_WARP_IN_STEP | E.VAR_TVL1_CLASSIC_GEOM, (4,)), (E.VAR_TVL1_CLASSIC_GEOM, (1, 3)),
                        (E.VAR_TVL1_NO_HEAD, (1, 2, 4))):
        forms += [dict(tvl1_fuse_k=k, variant=variant, step_group=3 + k) for k in ks]
    for form in forms:
        with dfx.FlowEngine(W, H, "tvl1", max_batch=2, **form) as eng:
            out = eng.calc_optflows(big_frames, 1)
            assert eng.stats().batch == 2, form
            assert _iters(eng.stats()) == base_iters, form
        for i, (a, b) in enumerate(zip(out, base)):
            assert np.array_equal(a, b), f"{form} pair {i}: {np.count_nonzero(a != b)} values differ"
        del out


def test_tvl1_8192x8191_bounded_output_matches_oracle(dfx, oracle, big_frames, big_oracle):
    """calc_optflows_u8 (flow, then encodeFlowMap's bounding, on the device) against the oracle's bounding of the
    oracle's flow, over 67 M pixels per plane."""
    with dfx.FlowEngine(W, H, "tvl1", max_batch=2) as eng:
        img_x, img_y = eng.calc_optflows_u8(big_frames, 1, BOUND)
    for i, (ref, _) in enumerate(big_oracle):
        ox, oy = oracle.flow_to_u8(ref, -BOUND, BOUND)
        assert np.array_equal(img_x[i], ox) and np.array_equal(img_y[i], oy), f"pair {i}"
    allv = np.concatenate([p.ravel() for p in img_x + img_y])
    assert (allv == 0).any() and (allv == 255).any()


# ---------------------------------------------------------------------------------------------- DCI 8K, 8192 x 4320

@pytest.fixture(scope="module")
def dci_frames():
    return _frames(DCI_W, DCI_H, 3, seed=9)


def test_tvl1_dci_8k_matches_oracle(dfx, oracle, dci_frames):
    f0, f1 = dci_frames[0], dci_frames[1]
    ref, tr = oracle.tvl1_calc(f0, f1, want_trace=True, threads=THREADS)
    with dfx.FlowEngine(DCI_W, DCI_H, "tvl1") as eng:
        out = eng.calc(f0, f1)
        st = eng.stats()
    assert np.array_equal(out, ref), f"max-abs {np.max(np.abs(out - ref))}, {np.count_nonzero(out != ref)} values differ"
    assert _iters(st) == [r[:5] for r in tr.iters_table()] and st.tvl1_checks == tr.n_checks


def test_farneback_dci_8k_matches_oracle(dfx, oracle, dci_frames):
    with dfx.FlowEngine(DCI_W, DCI_H, "farn") as eng:
        flows = eng.calc_optflows(dci_frames, 1)
    for i, out in enumerate(flows):
        ref = oracle.farneback_calc(dci_frames[i], dci_frames[i + 1], threads=THREADS)
        assert np.array_equal(out, ref), f"pair {i}: max-abs {np.max(np.abs(out - ref))}"


def test_brox_dci_8k_matches_oracle(dfx, oracle, dci_frames):
    """Beyond the 24 pyramid levels of every other Brox test (27 here, of DFX_MAX_LEVELS = 32)."""
    with dfx.FlowEngine(DCI_W, DCI_H, "brox") as eng:
        flows = eng.calc_optflows(dci_frames, 1)
        st = eng.stats()
    sizes = oracle.brox_pyramid_sizes(DCI_W, DCI_H)
    assert len(sizes) > 24 and st.levels == len(sizes)
    assert [(st.level_w[l], st.level_h[l]) for l in range(st.levels)] == [tuple(sz) for sz in sizes]
    for i, out in enumerate(flows):
        ref = oracle.brox_calc(dci_frames[i], dci_frames[i + 1], threads=THREADS)
        assert np.all(np.isfinite(out))
        assert np.array_equal(out, ref), f"pair {i}: max-abs {np.max(np.abs(out - ref))}"
