"""Register, scratch and LDS budgets of the two passes of the colour coding of flows (k_flowvis_max<masked> and
k_flowvis_colour<masked, interleaved, blended>; denseflow_amd/csrc/flow_colour_kernels.hip), read from the built library's
gfx950 code object with the method of tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the two
and the eight the launcher names; none has scratch, which is a condition of the kernels; LDS holds only the reduction's four
words (16 bytes) and the wheel (56 float4 = 896 bytes); the registers stay within the 128 that four waves per SIMD leave
(measured: 40 / 44 for the measuring pass without / with a mask, which holds four rows' loads at once; 44 planar and 46
interleaved for the colour pass, 69 for all four blended forms, the same with and without a mask: seven or eight waves fit)."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

VGPR_BOUND = 128
SIG = "EEv11FlowvisArgsNS_11FlowvisWideE"


def _max(masked):  # k_flowvis_max<masked> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_113k_flowvis_maxILb{int(masked)}E{SIG}"


def _colour(masked, il, blended):  # k_flowvis_colour<masked, il, blended>
    return f"_ZN12_GLOBAL__N_116k_flowvis_colourILb{int(masked)}ELb{int(il)}ELb{int(blended)}E{SIG}"


FORMS = [(m, il, b) for m in (False, True) for il in (False, True) for b in (False, True)]


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    want = [_max(m) for m in (False, True)] + [_colour(*f) for f in FORMS]
    assert sorted(k for k in kernels if "k_flowvis_" in k) == sorted(want)
    for pinned in ("k_fp_", "k_flow_median", "k_warp", "k_flow_chain", "k_gm_", "k_fb_check", "k_interp_synth", "k_farn_"):
        assert not any(pinned in k for k in want)


@pytest.mark.parametrize("masked", [False, True])
def test_the_measuring_pass_has_no_scratch_and_only_the_reductions_lds(kernels, masked):  # noqa: F811
    k = kernels[_max(masked)]
    print(f"k_flowvis_max<{masked}>: {k}")
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 16, k
    assert k["vgpr_count"] <= VGPR_BOUND, k


@pytest.mark.parametrize("masked,il,blended", FORMS)
def test_the_colour_pass_has_no_scratch_and_only_the_wheels_lds(kernels, masked, il, blended):  # noqa: F811
    k = kernels[_colour(masked, il, blended)]
    print(f"k_flowvis_colour<{masked}, {il}, {blended}>: {k}")
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 56 * 16, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 4
