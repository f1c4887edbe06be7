"""Register and LDS budgets of the Gaussian row-stream kernels (k_farn_gauss_stream, one instantiation per window 7 .. 21 and
form), read from the built library's gfx950 code object with the method of tests/test_farneback_kernel_resources.py (no GPU
needed): the instantiations are the ones the launchers name, none uses scratch, the ring is the box form's, and registers and
LDS fit the waves per SIMD each instantiation is compiled for (farn_gauss_wps, denseflow_amd/csrc/farneback_kernels.hip;
the table in DESIGN.md section 4).  That the box kernels did not grow is tests/test_farneback_kernel_resources.py itself."""
import pytest

from tests.test_farneback_kernel_resources import FORMS, HALVES, kernels  # noqa: F401  (fixture)


def _gauss(half, init, planar):  # k_farn_gauss_stream<half, init, planar>
    return (f"_Z19k_farn_gauss_streamILi{half}ELb{int(init)}ELb{int(planar)}EEv11FarnPairCtxiiiPfx8FarnInit12DfxPlanarOut"
            "11FarnWinTaps")


def _waves(half, planar):  # farn_gauss_wps: the box form's choice
    return 4 if (half <= 6 or (not planar and half <= 9)) else 3


def test_the_gaussian_instantiations_are_the_ones_the_launchers_name(kernels):  # noqa: F811
    have = sorted(k for k in kernels if "k_farn_gauss_stream" in k)
    assert have == sorted(_gauss(half, i, p) for half in HALVES for i, p in FORMS)
    assert "_Z22k_farn_iteration_gauss11FarnPairCtxiiii11FarnWinTaps" in kernels  # the generic kernel's Gaussian form


@pytest.mark.parametrize("init,planar", FORMS)
@pytest.mark.parametrize("half", HALVES)
def test_gaussian_stream_kernel_has_no_scratch_and_fits_its_waves(kernels, half, init, planar):  # noqa: F811
    k = kernels[_gauss(half, init, planar)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 20 * (6 + 2 * half) * (64 + 2 * half), k  # the ring: 20 B per M entry
    waves = _waves(half, planar)
    assert k["vgpr_count"] <= (128 if waves == 4 else 168), k  # 512 registers per SIMD lane
    assert waves * k["group_segment_fixed_size"] <= 160 * 1024, k  # 160 KB of LDS per CU


def test_generic_gaussian_kernel_has_no_scratch(kernels):  # noqa: F811
    k = kernels["_Z22k_farn_iteration_gauss11FarnPairCtxiiii11FarnWinTaps"]
    assert k["private_segment_fixed_size"] == 0, k
