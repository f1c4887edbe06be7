"""Register, scratch and LDS budgets of the synthesis pass of the frame interpolation (k_interp_synth<channels, interleaved,
filled>; denseflow_amd/csrc/interpolate_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the six the launcher names (gray, interleaved
and planar 3-channel images, each with and without the second tier of the filled flows); none has scratch, which is a
condition of the kernel, and none has LDS; the registers stay within the 128 that four waves per SIMD leave (measured: 46 for
gray, 58 for interleaved and 62 for planar 3-channel images, the same with and without the second tier, so eight waves fit)."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(1, False), (3, True), (3, False)]  # (channels, interleaved) as is_launch_as instantiates them
VGPR_BOUND = 128


def _synth(c, il, filled):  # k_interp_synth<c, il, filled> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_114k_interp_synthILi{c}ELb{int(il)}ELb{int(filled)}EEEvNS_6IsArgsE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    want = [_synth(c, il, f) for c, il in FORMS for f in (False, True)]
    assert sorted(k for k in kernels if "k_interp_synth" in k) == sorted(want)
    for pinned in ("k_fp_", "k_flow_median", "k_warp", "k_flow_chain", "k_gm_", "k_fb_check"):
        assert not any(pinned in k for k in want)


@pytest.mark.parametrize("filled", [False, True])
@pytest.mark.parametrize("c,il", FORMS)
def test_the_synthesis_has_no_scratch_no_lds_and_registers_for_four_waves(kernels, c, il, filled):  # noqa: F811
    k = kernels[_synth(c, il, filled)]
    print(f"k_interp_synth<{c}, {il}, {filled}>: {k}")
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 4
