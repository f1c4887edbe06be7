"""Register, scratch and LDS budgets of the flow-median kernel (k_flow_median<ksize, masked, mode>,
denseflow_amd/csrc/flow_median_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the six the launcher names; none has
scratch (every window and network index is a literal after unrolling); each has the LDS its staging declares — two planes of
keys, and a plane of exclusion words in the masked forms, of (16 + 2r) rows of 68 words; and each form's registers stay at
or below the occupancy step above what was measured (512 registers per SIMD lane): 3 x 3 unmasked 34 and masked 41 / 42
within 64 (eight waves per SIMD), 5 x 5 unmasked 76 within 80 (six), 5 x 5 masked 92 / 94 within 96 (five), as DESIGN.md
states."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(3, False, 0), (3, True, 0), (3, True, 1), (5, False, 0), (5, True, 0), (5, True, 1)]  # (ksize, masked, mode)
VGPR_BOUND = {(3, False): 64, (3, True): 64, (5, False): 80, (5, True): 96}
TILE_W, TILE_H = 64, 16  # FM_TILE_W, FM_TILE_H of flow_median_kernels.h


def _name(ksize, masked, mode):  # k_flow_median<ksize, masked, mode> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_113k_flow_medianILi{ksize}ELb{int(masked)}ELi{mode}EEEv6FmArgsNS_6FmWideE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    assert sorted(k for k in kernels if "k_flow_median" in k) == sorted(_name(*f) for f in FORMS)


@pytest.mark.parametrize("ksize,masked,mode", FORMS)
def test_no_scratch_the_staged_planes_and_registers_within_the_occupancy_step(kernels, ksize, masked, mode):  # noqa: F811
    k = kernels[_name(ksize, masked, mode)]
    r = ksize // 2
    pitch = (TILE_W + 2 * r + 3) // 4 * 4
    assert pitch == 68
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == (3 if masked else 2) * (TILE_H + 2 * r) * pitch * 4, k
    assert k["vgpr_count"] <= VGPR_BOUND[(ksize, masked)], k
    # the LDS never lowers the occupancy below what the registers allow (160 KB per CU, four SIMDs, 256-lane workgroups)
    waves = 512 // VGPR_BOUND[(ksize, masked)]
    assert waves * k["group_segment_fixed_size"] <= 160 * 1024, k
