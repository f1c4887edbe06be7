"""Register, scratch and LDS budgets of the motion descriptors' kernel (k_flow_hist<kinds, masked>;
denseflow_amd/csrc/flow_hist_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the fourteen the launcher names (kinds 1 .. 7,
without and with masks); none has scratch, which is a condition of the kernel; LDS holds the 64 x 49 64-bit sums of a band's
cells (25088 bytes) and the 64 x 3 float64 denominators (1536 bytes), within the 32 KiB the kernel may take; the registers stay
within the 128 that four waves per SIMD leave.  The measured values are printed (pytest -s) and quoted in the README."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

VGPR_BOUND = 128
LDS_BOUND = 32768
LDS_BYTES = 64 * 49 * 8 + 64 * 3 * 8
FORMS = [(k, m) for k in range(1, 8) for m in (False, True)]


def _name(kinds, masked):  # k_flow_hist<kinds, masked> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_111k_flow_histILi{kinds}ELb{int(masked)}EEEv6FhArgs"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    want = [_name(*f) for f in FORMS]
    assert sorted(k for k in kernels if "k_flow_hist" in k) == sorted(want)
    for pinned in ("k_fp_", "k_flow_median", "k_warp", "k_flow_chain", "k_gm_", "k_fb_check", "k_interp_synth", "k_farn_",
                   "k_flowvis_"):
        assert not any(pinned in k for k in want)


@pytest.mark.parametrize("kinds,masked", FORMS)
def test_no_scratch_lds_within_32k_and_at_most_128_registers(kernels, kinds, masked):  # noqa: F811
    k = kernels[_name(kinds, masked)]
    print(f"k_flow_hist<{kinds}, {masked}>: {k}")
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == LDS_BYTES <= LDS_BOUND, k
    assert k["vgpr_count"] <= VGPR_BOUND, k
    assert 512 // VGPR_BOUND == 4
