"""Register, scratch and LDS budgets of the flow-projection kernels (k_fp_scatter<imp, occ, lds window>, k_fp_normalise;
denseflow_amd/csrc/flow_project_kernels.hip) and of the one zero pass of the integer scatter (k_fs_zero;
denseflow_amd/csrc/flow_scatter.hip), read from the built library's gfx950 code object with the method
of tests/test_farneback_kernel_resources.py (no GPU needed): the scatter's instantiations are the four the launcher names, all
of the shipped LDS-window form; none of the kernels has scratch; the scatter's window is 48 x 16 pixels of three 64-bit words,
18432 bytes, so eight workgroups of four waves fit into a CU's 160 KiB, and its registers (26 measured) stay within the 64 that
eight waves per SIMD leave; the streaming passes have no LDS and stay within 64 registers too (14 and 38 measured)."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (importance, occ)
VGPR_BOUND = 64
WINDOW_BYTES = 48 * 16 * 3 * 8
ZERO, NORMALISE = "_ZN12_GLOBAL__N_19k_fs_zeroEPyx", "_ZN12_GLOBAL__N_114k_fp_normaliseE6FpArgsNS_6FpWideE"


def _scatter(imp, occ, window=True):  # k_fp_scatter<imp, occ, window> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_112k_fp_scatterILb{int(imp)}ELb{int(occ)}ELb{int(window)}EEEv6FpArgs"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    assert sorted(k for k in kernels if "k_fp_" in k or "k_fs_" in k) == sorted([_scatter(*f) for f in FORMS] + [ZERO, NORMALISE])
    assert not [k for k in kernels if "k_fp_zero" in k or "k_splat_zero" in k]  # the one zero pass is k_fs_zero


@pytest.mark.parametrize("imp,occ", FORMS)
def test_the_scatter_has_no_scratch_its_window_in_lds_and_registers_for_eight_waves(kernels, imp, occ):  # noqa: F811
    k = kernels[_scatter(imp, occ)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == WINDOW_BYTES == 18432, k
    assert 8 * k["group_segment_fixed_size"] <= 160 * 1024
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 8


@pytest.mark.parametrize("name", [ZERO, NORMALISE])
def test_the_streaming_passes_have_no_scratch_and_no_lds(kernels, name):  # noqa: F811
    k = kernels[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
