"""Register and LDS budgets of the two fast-pyramid kernels (k_farn_pyrdown for float and 8-bit sources, k_farn_pyrup_flow;
denseflow_amd/csrc/farneback_pyramid_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the ones the launchers name, none uses
scratch or LDS (the neighbours come from lane shifts), and the registers leave room for eight waves per SIMD — these are
streaming kernels that hide memory latency with occupancy."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

PYRDOWN_F32 = "_Z14k_farn_pyrdownIfEvPKT_xxiiPfxi"
PYRDOWN_U8 = "_Z14k_farn_pyrdownIhEvPKT_xxiiPfxi"
PYRUP = "_Z17k_farn_pyrup_flow11FarnPairCtxiiiiif"


def test_the_instantiations_are_the_ones_the_launchers_name(kernels):  # noqa: F811
    have = sorted(k for k in kernels if "k_farn_pyrdown" in k or "k_farn_pyrup" in k)
    assert have == sorted([PYRDOWN_F32, PYRDOWN_U8, PYRUP])


@pytest.mark.parametrize("name", [PYRDOWN_F32, PYRDOWN_U8, PYRUP])
def test_pyramid_kernels_have_no_scratch_no_lds_and_few_registers(kernels, name):  # noqa: F811
    k = kernels[name]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 64, k  # 512 registers per SIMD lane: eight waves
