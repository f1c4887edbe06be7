"""Register and LDS budgets of the Farneback row-stream iteration kernel (one instantiation per window 7 .. 21) and of the
polynomial-expansion kernels (polyN 5 and 7), read from the built library's gfx950 code object (no GPU needed): no
instantiation uses scratch, every one fits a CU's LDS several times over, and the instantiations of the reference's window
(winSize 13, half-width 6) need no more registers and LDS than before the kernel became a template on the window."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "denseflow_amd", "lib", "libdfx.so")
LLVM = "/opt/rocm/llvm/bin"
FIELDS = r"\.(group_segment_fixed_size|private_segment_fixed_size|vgpr_count):\s+(\d+)"

HALVES = range(3, 11)                                   # farn_stream_has_half (denseflow_amd/csrc/farneback_plan.h)
FORMS = [(False, False), (True, False), (False, True)]  # (INIT, PLANAR) as the launchers instantiate them
# k_farn_iter_stream<6, INIT, PLANAR> of the commit before this kernel was generalised (its only instantiations), read
# with this file's own method from that commit's library built by the same compiler: (vgpr_count, group_segment_fixed_size)
PARENT_HALF6 = {(False, False): (109, 27360), (True, False): (120, 27360), (False, True): (126, 27360)}
# k_farn_polyexp and k_farn_polyexp_rows<16> (polyN 5) of the same commit
PARENT_POLY5 = {"one_row": (25, 3072), "rows16": (53, 6144)}


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


def _stream(half, init, planar):  # k_farn_iter_stream<half, init, planar>
    return f"_Z18k_farn_iter_streamILi{half}ELb{int(init)}ELb{int(planar)}EEv11FarnPairCtxiifiPfx8FarnInit12DfxPlanarOut"


def _poly(form, n):  # k_farn_polyexp<n> / k_farn_polyexp_rows<16, n>
    sig = "EEvPKfxPKiPfx13FarnLevelGeom14FarnPolyConsts"
    return (f"_Z14k_farn_polyexpILi{n}" if form == "one_row" else f"_Z19k_farn_polyexp_rowsILi16ELi{n}") + sig


def test_the_instantiations_are_the_ones_the_launchers_name(kernels):
    have = sorted(k for k in kernels if "k_farn_iter_stream" in k or "k_farn_polyexp" in k)
    want = sorted([_stream(half, i, p) for half in HALVES for i, p in FORMS] +
                  [_poly(f, n) for f in ("one_row", "rows16") for n in (5, 7)])
    assert have == want


@pytest.mark.parametrize("init,planar", FORMS)
@pytest.mark.parametrize("half", HALVES)
def test_stream_kernel_has_no_scratch_and_fits_the_lds(kernels, half, init, planar):
    k = kernels[_stream(half, init, planar)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] <= 64 * 1024, k
    assert k["group_segment_fixed_size"] == 20 * (6 + 2 * half) * (64 + 2 * half), k  # the ring: 20 B per M entry
    # registers for the waves per SIMD the instantiation is compiled for and its LDS allows (512 registers per SIMD lane,
    # 160 KB of LDS per CU): three where the ring or the planar writer's window is large, four otherwise
    waves = 4 if (half <= 6 or (not planar and half <= 9)) else 3
    assert k["vgpr_count"] <= (128 if waves == 4 else 168), k
    assert waves * k["group_segment_fixed_size"] <= 160 * 1024, k


@pytest.mark.parametrize("form", ["one_row", "rows16"])
@pytest.mark.parametrize("n", [5, 7])
def test_polyexp_kernels_have_no_scratch(kernels, form, n):
    k = kernels[_poly(form, n)]
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] <= 64 * 1024, k


@pytest.mark.parametrize("init,planar", FORMS)
def test_reference_window_instantiations_did_not_grow(kernels, init, planar):
    k = kernels[_stream(6, init, planar)]
    vgpr, lds = PARENT_HALF6[(init, planar)]
    assert k["vgpr_count"] <= vgpr and k["group_segment_fixed_size"] <= lds, k


@pytest.mark.parametrize("form", ["one_row", "rows16"])
def test_poly_n_5_instantiations_did_not_grow(kernels, form):
    k = kernels[_poly(form, 5)]
    vgpr, lds = PARENT_POLY5[form]
    assert k["vgpr_count"] <= vgpr and k["group_segment_fixed_size"] <= lds, k
