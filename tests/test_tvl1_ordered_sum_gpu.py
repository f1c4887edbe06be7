"""The second trip of the last arriver's ordered sum (end_segment_tile, denseflow_amd/csrc/tvl1_device_common.h).

The last workgroup of a pair to arrive sums the pair's partial error sums with `for (i = tid; i < nblk; i += blockDim.x)`:
with 256 threads the loop takes a second trip only above 256 workgroups per pair.  960 x 400 is a frame at which the simple
kernel (impl 1: 64 x 4 pixels per workgroup) and the fused tile kernels (fuse_k 4), with and without the illumination
channel, all launch more than that at level 0; the counts are asserted from the dimensions below.  Two pyramid levels and
two warps bound the work; iterations and epsilon are the defaults, so the convergence check decides where every warp ends.
Two pairs share one device batch.  Every comparison is np.array_equal or ==: there is no tolerance."""
import numpy as np
import pytest

from denseflow_amd.synth import SynthClip
from tests.test_mixed_batches_gpu import _Ref, _check_flow, _check_tables

pytestmark = pytest.mark.gpu

W, H, SEED = 960, 400, 11
NSCALES, WARPS = 2, 2
FUSE_K = 4  # include/dfx.h: tvl1_fuse_k 0 = auto = 4
KW = dict(max_batch=2, tvl1_nscales=NSCALES, tvl1_warps=WARPS)
THREADS = 256  # per workgroup, of every step kernel


@pytest.fixture(scope="module")
def frames():
    return SynthClip(W, H, SEED).frames(3)  # two pairs: one batch


def _run(dfx, frames, **kw):
    with dfx.FlowEngine(W, H, "tvl1", **KW, **kw) as eng:
        flows = eng.calc_optflows(frames, 1)
        assert eng.stats().batch == 2
        tables, checks = eng.tvl1_batch_tables()
    return flows, tables, checks


def test_every_form_launches_more_workgroups_per_pair_than_a_workgroup_has_threads(dfx):
    simple = -(-W // 64) * -(-H // 4)
    assert simple == 1500 and simple > THREADS
    # a fused tile is 64 x TH pixels, TH = 2 * (largest fuse_k + 4) (tvl1_fused_max_k); it owns 64 - 2K columns, a tile at
    # the left or right border up to K more (tvl1_step_geom), and TH - 2K rows
    th = 2 * (dfx.load_library().dfxi_tvl1_fused_max_k() + 4)
    own_w, own_h = 64 - 2 * FUSE_K, th - 2 * FUSE_K
    tiles_x, tiles_y = -(-(W - 2 * FUSE_K) // own_w), -(-H // own_h)
    print(f"simple {simple} workgroups; fused tile 64 x {th}, at least {tiles_x} x {tiles_y} tiles")
    assert tiles_x * tiles_y > THREADS


def test_without_gamma_default_form_and_simple_kernel_are_the_oracle(dfx, oracle, frames):
    refs = []
    for a, b in zip(frames[:-1], frames[1:]):
        p = oracle.tvl1_default_params()
        p.nscales, p.warps = NSCALES, WARPS
        refs.append(_Ref(*oracle.tvl1_calc(a, b, p, want_trace=True)))
    print("oracle: iteration tables", [r.table for r in refs], "checks per level", [r.checks for r in refs])
    assert all(r.levels == NSCALES and sum(r.checks) > 0 for r in refs)
    for what, kw in (("default form", dict()), ("impl 1", dict(impl=1))):
        flows, tables, checks = _run(dfx, frames, **kw)
        assert len(flows) == len(tables) == 2
        for i, (got, r) in enumerate(zip(flows, refs)):
            _check_flow(got, r.flow, f"{what}, pair {i}")
        _check_tables(tables, checks, refs, what)


def test_with_gamma_tuned_form_and_simple_kernel_agree(dfx, frames):
    tuned = _run(dfx, frames, tvl1_gamma=0.4)
    simple = _run(dfx, frames, tvl1_gamma=0.4, impl=1)
    print("tvl1_gamma 0.4: iteration tables", tuned[1], "checks per level", tuned[2])
    assert sum(map(sum, tuned[2])) > 0  # convergence sums were evaluated
    assert tuned[1] == simple[1], "iteration tables differ"
    assert tuned[2] == simple[2], "checks per level differ"
    assert len(tuned[0]) == len(simple[0]) == 2
    for i, (a, b) in enumerate(zip(tuned[0], simple[0])):
        assert np.isfinite(a).all()
        _check_flow(a, b, f"tvl1_gamma 0.4, pair {i}, tuned form against impl 1")
