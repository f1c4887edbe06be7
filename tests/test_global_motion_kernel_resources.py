"""Register, scratch and LDS budgets of the global-motion kernels (k_gm_accumulate<model, first_round> and k_gm_apply,
denseflow_amd/csrc/global_motion_kernels.hip), read from the built library's gfx950 code object with the method of
tests/test_farneback_kernel_resources.py (no GPU needed): the instantiations are the ones the launcher names; none has
scratch; the accumulate forms have the 384 bytes of LDS their block reduction declares (twelve 64-bit partial sums per
wave) and the apply kernel none; the accumulate forms, measured at 76 registers, stay within 80 (six waves per SIMD, as
DESIGN.md states), the apply kernel within 64 (eight)."""
import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)

FORMS = [(model, first) for model in (0, 1) for first in (True, False)]
APPLY = "_ZN12_GLOBAL__N_110k_gm_applyE6GmArgsNS_6GmWideEf"


def _name(model, first):  # k_gm_accumulate<model, first> in the anonymous namespace
    return f"_ZN12_GLOBAL__N_115k_gm_accumulateILi{model}ELb{int(first)}EEEv6GmArgsNS_6GmWideEif"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    assert sorted(k for k in kernels if "k_gm_" in k) == sorted([_name(*f) for f in FORMS] + [APPLY])


@pytest.mark.parametrize("model,first", FORMS)
def test_accumulate_has_no_scratch_the_reductions_lds_and_registers_for_six_waves(kernels, model, first):  # noqa: F811
    k = kernels[_name(model, first)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 4 * 12 * 8, k
    assert k["vgpr_count"] <= 80, k  # 512 registers per SIMD lane: six waves


def test_apply_has_no_scratch_no_lds_and_registers_for_eight_waves(kernels):  # noqa: F811
    k = kernels[APPLY]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 64, k
