"""Register and LDS budget of the forward-backward check kernel (k_fb_check, denseflow_amd/csrc/fb_check_kernels.hip), read
from the built library's gfx950 code object with the method of tests/test_farneback_kernel_resources.py (no GPU needed): one
kernel, no scratch, no LDS (the taps of a gather with an unbounded displacement are plain global loads), and registers for
eight waves per SIMD — a streaming kernel hides the gather's latency with occupancy."""
from tests.test_farneback_kernel_resources import kernels  # noqa: F401  (fixture)


def test_the_check_kernel_has_no_scratch_no_lds_and_few_registers(kernels):  # noqa: F811
    have = [k for k in kernels if "k_fb_check" in k]
    assert len(have) == 1, have
    k = kernels[have[0]]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 64, k  # 512 registers per SIMD lane: eight waves
