"""Register, scratch and LDS budgets of the warp kernel's instantiations (k_warp<channels, interleaved, statistics>,
denseflow_amd/csrc/warp_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): no instantiation has scratch; the forms without statistics have no
LDS, the forms with statistics the 32 bytes their block reduction declares (two 32-bit partial sums per wave); and every
form keeps registers for eight waves per SIMD except the planar 3-channel one with statistics, which DESIGN.md gives 80
registers (six waves per SIMD) rather than let it spill."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(c, il, st) for c, il in ((1, False), (3, True), (3, False)) for st in (False, True)]


def _name(c, il, st):  # k_warp<c, il, st> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_16k_warpILi{c}ELb{int(il)}ELb{int(st)}EEEv8WarpArgsNS_8WarpWideE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    assert sorted(k for k in kernels if "k_warp" in k) == sorted(_name(*f) for f in FORMS)


@pytest.mark.parametrize("c,il,st", FORMS)
def test_no_scratch_lds_only_for_the_reduction_and_registers_within_the_budget(kernels, c, il, st):  # noqa: F811
    k = kernels[_name(c, il, st)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == (32 if st else 0), k
    budget = 80 if (c, il, st) == (3, False, True) else 64  # 512 registers per SIMD lane: six waves, eight waves
    assert k["vgpr_count"] <= budget, k
