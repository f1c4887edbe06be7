"""Register, scratch and LDS budgets of the forward-warp kernels (k_splat_scatter<channels, source form, lds window>,
k_splat_normalise<channels, interleaved>; denseflow_amd/csrc/splat_kernels.hip) and of the zero pass they launch (k_fs_zero;
denseflow_amd/csrc/flow_scatter.hip), read from the built library's gfx950
code object with the method of tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the seven
scatter forms and the five normalising forms the launcher names, all of the shipped LDS-window form; none of the kernels has
scratch; the scatter's window is 48 x 16 pixels of (1 + C) 64-bit words — 12 / 18 / 24 / 30 KiB, so at C = 4 five workgroups of
four waves fit into a CU's 160 KiB — and its registers (22 .. 28 measured) stay within the 64 that eight waves per SIMD leave;
the streaming passes have no LDS and stay within 64 registers too (14 for the zero pass, 34 / 40 / 48 / 56 for the normalising
pass of 1 / 2 / 3 / 4 channels).  Resource metadata only."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

U8, U8_IL, F32 = 0, 1, 2  # the source forms of splat_kernels.hip: byte planes, interleaved bytes, float planes
SCATTERS = [(1, U8), (3, U8_IL), (3, U8), (1, F32), (2, F32), (3, F32), (4, F32)]  # (channels, source form)
NORMALISES = [(1, False), (2, False), (3, False), (4, False), (3, True)]            # (channels, interleaved)
VGPR_BOUND = 64
ZERO = "_ZN12_GLOBAL__N_19k_fs_zeroEPyx"


def _scatter(c, form, window=True):  # k_splat_scatter<c, form, window> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_115k_splat_scatterILi{c}ELi{form}ELb{int(window)}EEEv9SplatArgs"


def _normalise(c, il):  # k_splat_normalise<c, il>
    return f"_ZN12_GLOBAL__N_117k_splat_normaliseILi{c}ELb{int(il)}EEEv9SplatArgsNS_9SplatWideE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    want = [_scatter(*f) for f in SCATTERS] + [_normalise(*f) for f in NORMALISES] + [ZERO]
    assert sorted(k for k in kernels if "k_splat_" in k or "k_fs_" in k) == sorted(want)


@pytest.mark.parametrize("c,form", SCATTERS)
def test_the_scatter_has_no_scratch_its_window_in_lds_and_registers_for_eight_waves(kernels, c, form):  # noqa: F811
    k = kernels[_scatter(c, form)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 48 * 16 * (1 + c) * 8 == (12288, 18432, 24576, 30720)[c - 1], k
    assert (160 * 1024) // k["group_segment_fixed_size"] >= 5
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 8


@pytest.mark.parametrize("name", [ZERO] + [_normalise(*f) for f in NORMALISES])
def test_the_streaming_passes_have_no_scratch_and_no_lds(kernels, name):  # noqa: F811
    k = kernels[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
