"""The TVL1 step kernel's lean form (the default: lane +-1 neighbours by DPP, rho_c / grad / 1/grad in LDS, 128 VGPRs =
4 waves per SIMD) against its register form of rounds 2-6 (DFX_VAR_TVL1_STEP_NBR_LDS: neighbour planes in LDS, the
loop constants in registers, 3 waves per SIMD).  Same tile, same arithmetic, same error-sum order: the flows and the
iteration tables must be the same bits — for every hypot reading and the fast mode, for every fuse_k, in both tile
geometries, for frames smaller than one tile, one tile wide and ragged at both borders, and for a ragged batch."""
import numpy as np
import pytest

from denseflow_amd.synth import HardClip, SynthClip


def _iters(stats):
    return [r[:5] for r in stats.iters_table()]


def _run(dfx, w, h, frames, **kw):
    with dfx.FlowEngine(w, h, "tvl1", max_batch=3, **kw) as eng:
        out = eng.calc_optflows(frames, 1)
        return out, _iters(eng.stats())


def _same(dfx, w, h, frames, **kw):
    from denseflow_amd import engine as E

    base, base_iters = _run(dfx, w, h, frames, variant=kw.pop("variant", 0) | E.VAR_TVL1_STEP_NBR_LDS, **kw)
    out, iters = _run(dfx, w, h, frames, **kw)
    assert iters == base_iters, kw
    for i, (a, b) in enumerate(zip(out, base)):
        assert np.array_equal(a, b), f"{kw}: pair {i} changed"


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", [(224, 224, 1), (97, 61, 9), (64, 32, 4), (16, 16, 2), (300, 200, 6), (786, 70, 5),
                                      (1229, 691, 2)])
@pytest.mark.parametrize("math", [0, 1, 2, 3])
def test_lean_step_kernel_is_the_register_form_bit_for_bit(dfx, w, h, seed, math):
    clip = SynthClip(w, h, seed)
    frames = clip.frames(3) + [HardClip(w, h, seed).frame(0), HardClip(w, h, seed).frame(1)]  # + a cut, + hard content
    _same(dfx, w, h, frames, tvl1_math=math)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", [(224, 224, 1), (120, 442, 3), (57, 40, 4)])
def test_lean_step_kernel_for_every_k_and_geometry(dfx, w, h, seed):
    from denseflow_amd import engine as E

    clip = SynthClip(w, h, seed)
    frames = clip.frames(4)
    for k in (1, 2, 3, 4, 6):
        _same(dfx, w, h, frames, tvl1_fuse_k=k, step_group=3 + k)
    for variant in (E.VAR_TVL1_CLASSIC_GEOM, E.VAR_TVL1_NO_HEAD, E.VAR_TVL1_WARP_IN_STEP):
        _same(dfx, w, h, frames, variant=variant)
