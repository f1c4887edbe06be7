"""Registers, LDS and scratch of the TVL1 step and warp-and-head kernels, read from the built library's gfx950 code object
(no GPU needed), against the commit before their segment tail became one function (end_segment_tile,
denseflow_amd/csrc/tvl1_device_common.h): no instantiation needs more registers, every one has that commit's LDS size, and
none uses scratch.  k_tvl1_warp_head sits one register under its 128, k_tvl1_step_fused<true, *> at 128: a shared tail that
cost either of them a register would cost a wave per SIMD."""
import pytest

from tests.test_step_kernel_occupancy import kernels  # noqa: F401  (fixture)

MATHS = [0, 1, 2, 3]  # dfx_params.tvl1_math
# (vgpr_count, group_segment_fixed_size) of that commit, read with the same fixture from its library built by the same
# compiler; every instantiation of k_tvl1_step_fused, k_tvl1_step_fused_nbr_lds, k_tvl1_warp_head, k_tvl1_warp_head_regs
# and k_tvl1_step_fused_gamma
PARENT = {}
PARENT.update({f"_Z17k_tvl1_step_fusedILb1ELi{m}EEv12Tvl1LevelCtxiii": (128, 32840) for m in MATHS})
PARENT.update({f"_Z25k_tvl1_step_fused_nbr_ldsILi{m}EEv12Tvl1LevelCtxiii": (v, 36936)
               for m, v in zip(MATHS, (168, 158, 168, 168))})
PARENT.update({f"_Z16k_tvl1_warp_headILi{m}EEv12Tvl1LevelCtxi": (127, 40392) for m in MATHS})
PARENT.update({f"_Z21k_tvl1_warp_head_regsILi{m}EEv12Tvl1LevelCtxi": (v, 42312)
               for m, v in zip(MATHS, (167, 167, 167, 168))})
PARENT["_Z23k_tvl1_step_fused_gamma12Tvl1LevelCtxi"] = (162, 36936)
# k_tvl1_step_fused<false, 0>, the scalar tile form (impl 2)
SCALAR = "_Z17k_tvl1_step_fusedILb0ELi0EEv12Tvl1LevelCtxiii"
PARENT_SCALAR = (168, 49224)
NAMES = ("k_tvl1_step_fusedI", "k_tvl1_step_fused_nbr_ldsI", "k_tvl1_warp_headI", "k_tvl1_warp_head_regsI",
         "k_tvl1_step_fused_gamma1")


def test_the_instantiations_are_the_ones_the_launchers_name(kernels):
    have = sorted(k for k in kernels if any(n in k for n in NAMES))
    assert have == sorted(list(PARENT) + [SCALAR])


@pytest.mark.parametrize("name", sorted(PARENT))
def test_kernel_kept_its_registers_and_lds_and_has_no_scratch(kernels, name):
    k = kernels[name]
    vgpr, lds = PARENT[name]
    assert k["vgpr_count"] <= vgpr, k
    assert k["group_segment_fixed_size"] == lds, k
    assert k["private_segment_fixed_size"] == 0, k


def test_scalar_tile_form_kept_its_registers_and_lds_and_has_no_scratch(kernels):
    """k_tvl1_step_fused<false, 0> held 168 VGPRs (its limit at three waves per SIMD) and 12 bytes of scratch in that commit:
    two VGPRs, one row's 64-bit byte offset in fused_tile_iterate, were spilled from the tile's loads to its stores.  The
    store phase now forms its offsets again instead."""
    k = kernels[SCALAR]
    assert k["vgpr_count"] <= PARENT_SCALAR[0], k
    assert k["group_segment_fixed_size"] == PARENT_SCALAR[1], k
    assert k["private_segment_fixed_size"] == 0, k
