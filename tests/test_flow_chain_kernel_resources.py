"""Register, scratch and LDS budgets of the flow-chain kernel (k_flow_chain<occ, all>,
denseflow_amd/csrc/flow_chain_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the four the launcher names; none has
scratch (A, valid and the taps of a lane's four pixels are registers through all links); none has LDS (the taps are global
gathers, no window is staged); and each form's registers stay at or below the occupancy step above what was measured (512
registers per SIMD lane): 52 (no masks, every link emitted), 54 (no masks, last), 56 (masks, every link) and 58 (masks, last)
within 64, eight waves per SIMD, as DESIGN.md states."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (occ, all)
VGPR_BOUND = 64


def _name(occ, every):  # k_flow_chain<occ, all> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_112k_flow_chainILb{int(occ)}ELb{int(every)}EEEv6FcArgsNS_6FcWideE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    assert sorted(k for k in kernels if "k_flow_chain" in k) == sorted(_name(*f) for f in FORMS)


@pytest.mark.parametrize("occ,every", FORMS)
def test_no_scratch_no_lds_and_registers_for_eight_waves(kernels, occ, every):  # noqa: F811
    k = kernels[_name(occ, every)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 8
