"""The TVL1 warp-and-head kernel's register budget, read from the built library's gfx950 code object (no GPU needed): the
lean form (the default, every arithmetic mode) fits 128 VGPRs = 4 waves per SIMD with no scratch and leaves room for 4
workgroups in a CU's LDS; the register form (DFX_VAR_TVL1_HEAD_NBR_LDS) is kept without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "denseflow_amd", "lib", "libdfx.so")
LLVM = "/opt/rocm/llvm/bin"
FIELDS = r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count):\s+(\d+)"


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tools = [_tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]
    if not os.path.exists(LIB) or None in tools:
        pytest.fail("needs the built library and the ROCm LLVM tools")
    objcopy, bundler, readelf = tools
    d = tmp_path_factory.mktemp("co")
    fatbin = str(d / "lib.fatbin")
    subprocess.run([objcopy, "-O", "binary", "--only-section=.hip_fatbin", LIB, fatbin], check=True)
    # the section holds one offload bundle per translation unit, back to back
    data = open(fatbin, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    notes = ""
    for i, s in enumerate(starts):
        part, co = str(d / f"b{i}.bundle"), str(d / f"b{i}.co")
        open(part, "wb").write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        subprocess.run([bundler, "--type=o", "--unbundle", f"--input={part}", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
        notes += subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    # one msgpack map per kernel in the metadata note: .group_segment_fixed_size ... .name ... .vgpr_count
    for block in re.split(r"\n\s*- \.", notes):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(FIELDS, block)}
    return out


@pytest.mark.parametrize("math", [0, 1, 2, 3])
def test_lean_head_kernel_runs_four_waves_per_simd(kernels, math):
    name = f"_Z16k_tvl1_warp_headILi{math}EEv12Tvl1LevelCtxi"  # k_tvl1_warp_head<math>
    assert name in kernels, sorted(k for k in kernels if "head" in k)
    k = kernels[name]
    assert k["vgpr_count"] <= 128, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] <= 40 * 1024, k  # 4 workgroups in 160 KB


@pytest.mark.parametrize("math", [0, 1, 2, 3])
def test_register_form_is_kept_without_scratch(kernels, math):
    name = f"_Z21k_tvl1_warp_head_regsILi{math}EEv12Tvl1LevelCtxi"  # k_tvl1_warp_head_regs<math>
    assert name in kernels, sorted(k for k in kernels if "head" in k)
    assert kernels[name]["private_segment_fixed_size"] == 0, kernels[name]
