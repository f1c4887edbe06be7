"""The TVL1 warp-and-head kernel's lean form (the default: the two iterations on the lean tile function, I0 loaded row by
row, the far gather one window row at a time, an 80 x 42 image tile — at most 128 VGPRs and 40 KB of LDS = 4 waves per SIMD)
against its register form of round 6 (DFX_VAR_TVL1_HEAD_NBR_LDS: 80 x 44 image tile, 3 waves per SIMD) and against the
two-launch form (DFX_VAR_TVL1_NO_HEAD).  The three must agree bit for bit, flows and tvl1_batch_tables() alike; at
tvl1_math 0, 2 and 3 the default is also held against the CPU oracle's matching reading.

Shapes: 96 x 40 (one tile column, two tile rows: every tile on the border, both own-edge flags set), 130 x 70 (the smallest
size with an interior tile), 256 x 128, 250 x 121 (ragged last row and column, w not a multiple of 4: the per-element
patch of the straddling float4 of the image-tile copy).
Settings: 2 levels, 3 warps (warp 0 with p = 0, the others with p loaded); 1, 2 and 6 iterations (the segment ends inside
the head / the head is the whole loop / the loop goes on into the step kernel, which reads the stored I1wx, I1wy,
rho_c); epsilon 0 and the default.
Content: plain pairs, a hard cut, hard content, and a pair whose halves move vertically by +4 and -6 pixels (the lean
image tile's vertical margin, 3, plus 1 and plus 3): that tile serves vertical flows in (-4, 4] (the round-6 one
(-5, 5]), so the first sits on the new `far` boundary and the second 2 pixels beyond it.  Those flows only develop over a full pyramid, so the content pairs also run with the
reference's parameters."""
import numpy as np
import pytest

from denseflow_amd.synth import HardClip, SynthClip
from tests.test_mixed_batches_gpu import _Ref, _check_flow, _check_tables

pytestmark = pytest.mark.gpu

SHAPES = [(96, 40, 4), (130, 70, 5), (256, 128, 1), (250, 121, 6)]
SETTINGS = [{"tvl1_iterations": it, **eps} for it in (1, 2, 6) for eps in ({}, {"tvl1_epsilon": 0.0})]
FAR_MARGIN = 3  # the lean image tile's vertical margin: HY = FAR_MARGIN + 2 rows above and below the 64 x 32 tile


def _frames(w, h, seed):
    """5 pairs: two plain ones, a hard cut, hard content, and the vertical motion across the far boundary."""
    hard = HardClip(w, h, seed)
    last = hard.frame(1)
    moved = last.copy()
    moved[:, : w // 2] = np.roll(last[:, : w // 2], FAR_MARGIN + 1, axis=0)
    moved[:, w // 2:] = np.roll(last[:, w // 2:], -(FAR_MARGIN + 3), axis=0)
    return SynthClip(w, h, seed).frames(3) + [hard.frame(0), last, moved]


def _run(dfx, w, h, frames, **kw):
    with dfx.FlowEngine(w, h, "tvl1", max_batch=3, **kw) as eng:  # 5 pairs: a batch of 3 and a ragged one of 2
        flows = eng.calc_optflows(frames, 1)
        tables, checks = eng.tvl1_batch_tables()
    return flows, tables, checks


def _three_forms_agree(dfx, w, h, frames, **kw):
    from denseflow_amd import engine as E

    flows, tables, checks = _run(dfx, w, h, frames, **kw)
    for name in ("VAR_TVL1_HEAD_NBR_LDS", "VAR_TVL1_NO_HEAD"):
        f2, t2, c2 = _run(dfx, w, h, frames, variant=getattr(E, name), **kw)
        assert (t2, c2) == (tables, checks), f"{kw}: tables of {name} differ"
        for i, (a, b) in enumerate(zip(flows, f2)):
            _check_flow(a, b, f"{kw}: pair {i} against {name}")
    return flows, tables, checks


@pytest.fixture(scope="module")
def ref_of(oracle):
    """Oracle results keyed by the pair, the reading and the parameters: computed once for the module."""
    cache = {}
    readings = {0: 0, 2: oracle.VAR_TVL1_SQRT_HYPOT, 3: oracle.VAR_TVL1_LIBM_HYPOT}

    def get(f0, f1, math, kw):
        key = (f0.tobytes(), f1.tobytes(), math, tuple(sorted(kw.items())))
        if key not in cache:
            p = oracle.tvl1_default_params()
            for k, v in kw.items():
                setattr(p, k[len("tvl1_"):], v)
            with oracle.variant(readings[math]):
                cache[key] = _Ref(*oracle.tvl1_calc(f0, f1, p, want_trace=True))
        return cache[key]

    return get


def _against_oracle(ref_of, frames, math, kw, flows, tables, checks):
    refs = [ref_of(frames[i], frames[i + 1], math, kw) for i in range(len(frames) - 1)]
    for i, r in enumerate(refs):
        _check_flow(flows[i], r.flow, f"{kw} math {math}: pair {i} against the oracle")
    _check_tables(tables, checks, refs, f"{kw} math {math}", first=len(refs) - len(tables))  # (the last batch's readout)


@pytest.mark.parametrize("math", [0, 1, 2, 3])
@pytest.mark.parametrize("w,h,seed", SHAPES)
def test_lean_head_kernel_is_the_register_form_and_the_two_launch_form(dfx, ref_of, w, h, seed, math):
    frames = _frames(w, h, seed)
    for setting in SETTINGS:
        kw = {"tvl1_nscales": 2, "tvl1_warps": 3, **setting}
        flows, tables, checks = _three_forms_agree(dfx, w, h, frames, tvl1_math=math, **kw)
        assert len(flows) == 5 and len(tables) == 2
        if math != 1:
            _against_oracle(ref_of, frames, math, kw, flows, tables, checks)


@pytest.mark.parametrize("math", [0, 1])
@pytest.mark.parametrize("w,h,seed", [(130, 70, 5), (250, 121, 6)])
def test_large_and_far_flows_over_the_full_pyramid(dfx, ref_of, w, h, seed, math):
    """The cut, the hard pair and the moved pair with the reference's parameters: the flows reach and pass the image
    tile's margin (asserted on the result), at every level on the way down."""
    frames = _frames(w, h, seed)[2:]
    flows, tables, checks = _three_forms_agree(dfx, w, h, frames, tvl1_math=math)
    v = np.abs(flows[-1][..., 1])
    assert (v > FAR_MARGIN + 1).any() and (v <= FAR_MARGIN + 1).any(), "the moved pair straddles the far boundary"
    assert np.abs(flows[0]).max() > FAR_MARGIN + 3, "the cut's flow is large"
    if math == 0:
        _against_oracle(ref_of, frames, 0, {}, flows, tables, checks)
