"""Register, scratch and LDS use of the kernels of the warp of typed planes (denseflow_amd/csrc/plane_warp_kernels.hip), read
from the built library's gfx950 code object with the method of tests/test_farneback_kernel_resources.py (no GPU needed): the
instantiations are exactly the ones the launcher names, none uses scratch or LDS, and every one keeps the registers of the
waves per SIMD it is compiled for — eight (64 registers) for both interleaved forms and the planar forms with 32-bit lane
offsets, where the taps bind as in k_warp; the planar forms with 64-bit lane offsets (a plane that spans 4 GiB or more)
hold up to 32 registers of tap offsets instead of 16 and are bounded at 96 (five waves per SIMD)."""
import itertools

import pytest

from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (the fixture that reads the code object)

SAMPLES, KEEPS, BIGS = (0, 1), (False, True), (False, True)


def _planar(sample, keep, big):  # k_pw_planar<sample, keep, big>
    return f"_ZN12_GLOBAL__N_111k_pw_planarILi{sample}ELb{int(keep)}ELb{int(big)}EEEv6PwArgsNS_6PwWideE"


def _interleaved(sample, keep):  # k_pw_interleaved<sample, keep>
    return f"_ZN12_GLOBAL__N_116k_pw_interleavedILi{sample}ELb{int(keep)}EEEv6PwArgsNS_6PwWideE"


def test_the_instantiations_are_the_ones_the_launcher_names(kernels):  # noqa: F811
    have = sorted(k for k in kernels if "k_pw_" in k)
    want = sorted([_planar(s, k, b) for s, k, b in itertools.product(SAMPLES, KEEPS, BIGS)] +
                  [_interleaved(s, k) for s, k in itertools.product(SAMPLES, KEEPS)])
    assert have == want
    for k in have:  # the names the other resource tests select their kernels by do not occur in these
        for other in ("k_warp", "k_fp_", "k_gm_", "k_splat_", "k_flow_", "k_interp_synth", "k_flowvis_", "k_fb_check", "k_farn_"):
            assert other not in k


@pytest.mark.parametrize("sample,keep,big", list(itertools.product(SAMPLES, KEEPS, BIGS)))
def test_planar_forms(kernels, sample, keep, big):  # noqa: F811
    k = kernels[_planar(sample, keep, big)]
    print("k_pw_planar<%d, %d, %d>:" % (sample, keep, big), k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= (96 if big else 64), k


@pytest.mark.parametrize("sample,keep", list(itertools.product(SAMPLES, KEEPS)))
def test_interleaved_forms(kernels, sample, keep):  # noqa: F811
    k = kernels[_interleaved(sample, keep)]
    print("k_pw_interleaved<%d, %d>:" % (sample, keep), k)
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 64, k
