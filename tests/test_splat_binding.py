"""The forward warp (splat) at the binding level (no GPU): include/dfx.h declares dfx_splat_device, dfx_splat_work_bytes and the
descriptor at DFX_VERSION >= 503, libdfx.so exports the symbols, engine.py binds them with a ctypes structure that has the
header's fields in the header's order, types, offsets and size (a C program compiled against the header prints them), and the
argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}  # every pointer is a c_void_p
STRUCT, CLASS = "dfx_splat_desc", "DfxSplatDesc"
FIELDS = ["d_src", "src_dtype", "channels", "layout", "src_pitch", "src_plane_stride", "src_image_stride", "d_flow",
          "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n", "t", "min_weight", "mode", "hole_mode", "out_dtype",
          "d_importance", "importance_pitch_floats", "importance_stride_floats", "d_occ", "occ_pitch", "occ_stride", "d_out",
          "out_pitch", "out_plane_stride", "out_image_stride", "d_hole", "hole_pitch", "hole_stride", "d_coverage",
          "coverage_pitch_floats", "coverage_stride_floats", "d_work", "work_bytes"]


def _source():
    return open(os.path.join(ROOT, "include", "dfx.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _source(), flags=re.S)


def _header_fields(struct):
    """[(name, ctypes type)] of a struct as the header declares it."""
    m = re.search(r"typedef struct \{([^{}]*)\}\s*" + struct + ";", _header())
    assert m, f"include/dfx.h does not declare {struct}"
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        d = re.fullmatch(r"(?:const )?(\w+) (\*?)(\w+)", decl)
        assert d, decl
        fields.append((d.group(3), C.c_void_p if d.group(2) else CTYPES[d.group(1)]))
    return fields


def test_the_header_declares_the_entry_points_at_version_503():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 503
    assert re.search(r"\bint\s+dfx_splat_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_splat_desc\s*\*\s*d\s*\)\s*;", src)
    assert re.search(r"\bsize_t\s+dfx_splat_work_bytes\s*\(\s*dfx_handle\s+h\s*,\s*int\s+channels\s*\)\s*;", src)
    assert "(0.5.3)" in _source()
    for name, value in (("DFX_SPLAT_MEAN", 0), ("DFX_SPLAT_SUM", 1), ("DFX_SPLAT_HOLE_ZERO", 0), ("DFX_SPLAT_HOLE_KEEP", 1)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", src).group(1)) == value


def test_every_field_of_the_struct_is_documented():
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", _source(), flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 35
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == FIELDS


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    src = _source()
    sec = src[src.index("along a flow (0.5.3)"):src.index("} dfx_splat_desc;")]
    whole = re.sub(r"\s*\n\s*\*\s*", " ", sec)
    for out_of_scope in ("typed (float16 / bfloat16) outputs", "several t per call",
                         "an importance computed by the library (exp stays the caller's)",
                         "fusing the splat into dfx_interpolate_device or dfx_calc_batch_bidir_device",
                         "host-pointer and submit forms", "the host shell and its CLI"):
        assert out_of_scope in whole[whole.index("Out of scope:"):], out_of_scope
    for text in ("skip the pixel if d_occ != NULL and occ[y][x] != 0", "px = (float)x + t*fu;   py = (float)y + t*fv",
                 "skip unless px > -1 && px < W && py > -1 && py < H", "tested before any conversion to int",
                 "imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)",
                 "x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)", "q_c = the byte",
                 "skip the pixel unless every channel has fabsf(v_c) <= 32768.f (false for NaN)",
                 "q_c = (int)rintf(v_c * 256.f)", "column weights {256 - bx, bx} and row weights {256 - by, by}",
                 "a tap outside [0, W) x [0, H) is dropped", "wt = wx * wy * iq",
                 "Wsum[tap] += wt (uint64);   S_c[tap] += wt * q_c", "two's-complement wrap on both sides",
                 "Wmin = max(1, (uint64)llrint((double)min_weight * 16777216.0))", "hole = Wsum < Wmin",
                 "DFX_SPLAT_MEAN: r_c = (double)S_c / (double)Wsum", "DFX_SPLAT_SUM:  r_c = (double)S_c / 16777216.0",
                 "r_c = r_c * (1.0 / 256.0)", "out_c = (float)r_c", "out_c = (uint8_t)llrint(r_c)",
                 "DFX_SPLAT_HOLE_KEEP does not write the pixel of d_out", "(float)((double)Wsum / 16777216.0)",
                 "no fused multiply-add", "is skipped, not clamped", "r_c lies in [0, 255] by construction",
                 "while |v| < 8192 with fewer than 1024 maximum-importance sources on one target",
                 "leaves dfx_get_stats alone", "dfx_device_bytes is unchanged", "d_out == d_src", "tests/splat_ref.py",
                 "(1 + channels) 64-bit words per pixel", "No float atomics",
                 "the result does not depend on how many images share a wave", "d_work not 8-byte aligned",
                 "dfx_flow_project_device's result with scale = 1, bit for bit", "DFX_ERR_UNSUPPORTED: a DFX_ALGO_FRAMES handle"):
        assert text in whole, text
    # the projection's and the interpolation's sections stay as they were: their out-of-scope lists still name the gap
    everything = re.sub(r"\s*\n\s*\*\s*", " ", src)
    assert "Out of scope: splatting of images or arbitrary payloads (softmax splatting of frames);" in everything
    assert "softmax splatting of the images themselves;" in everything


def test_the_reference_module_states_the_same_arithmetic():
    from tests import splat_ref as R

    doc = " ".join(R.__doc__.split())
    src = _source()
    sec = src[src.index("along a flow (0.5.3)"):src.index("} dfx_splat_desc;")]
    lines = [" ".join(ln.strip().lstrip("*").split()) for ln in sec.splitlines()]
    first = next(i for i, ln in enumerate(lines) if ln.startswith("skip the pixel if"))
    last = next(i for i, ln in enumerate(lines) if ln.startswith("coverage plane (float32, optional)"))
    assert last - first > 20
    for ln in lines[first:last + 1]:
        assert ln in doc, ln


def test_the_library_exports_and_the_binding_binds_the_symbols(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    raw = C.CDLL(dfx.library_path())
    assert hasattr(raw, "dfx_splat_device") and hasattr(raw, "dfx_splat_work_bytes")
    assert len(L.dfx_splat_device.argtypes) == 2
    assert L.dfx_splat_device.argtypes[1] is C.POINTER(E.DfxSplatDesc)
    assert L.dfx_splat_device.restype is C.c_int
    assert L.dfx_splat_work_bytes.restype is C.c_size_t and L.dfx_splat_work_bytes.argtypes == [C.c_void_p, C.c_int]
    assert L.dfx_splat_work_bytes(None, 3) == 0  # a NULL handle: nothing is dereferenced
    assert E.SPLAT_MODES == {"mean": 0, "sum": 1} and E.SPLAT_HOLES == {"zero": 0, "keep": 1} and E.SPLAT_MAX_CHANNELS == 4
    for name in ("splat", "splat_tensor", "splat_device", "splat_work_bytes"):
        assert callable(getattr(dfx.FlowEngine, name)), name


def test_the_ctypes_structure_is_the_headers(tmp_path):
    from denseflow_amd import engine as E

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None and os.path.exists("/opt/rocm/llvm/bin/clang"):
        cc = "/opt/rocm/llvm/bin/clang"
    assert cc, "needs a C compiler"
    fields = _header_fields(STRUCT)
    prints = f'    printf("sizeof %zu\\n", sizeof({STRUCT}));\n'
    prints += "".join(f'    printf("{n} %zu\\n", offsetof({STRUCT}, {n}));\n' for n, _ in fields)
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include "dfx.h"\nint main(void) {\n' + prints + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    got = {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        name, value = ln.split()
        got[name] = int(value)
    cls = getattr(E, CLASS)
    assert [(n, t) for n, t in cls._fields_] == fields
    assert got.pop("sizeof") == C.sizeof(cls)
    assert got == {n: getattr(cls, n).offset for n, _ in fields}


class _Untouchable:
    """Stands where the loaded library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_engine(dfx, w=8, h=4):
    eng = object.__new__(dfx.FlowEngine)  # no handle, no device: everything below must be refused before either is needed
    eng.width, eng.height, eng._device = w, h, 0
    eng._L, eng._h = _Untouchable(), None
    return eng


def _refused_settings(call):
    """The settings every wrapper refuses."""
    for bad in (0, 0.0, -0.0, float("nan"), float("inf"), 1e39, None, "1", True):
        with pytest.raises(ValueError, match="t must"):
            call(t=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0.25", True):
        with pytest.raises(ValueError, match="min_weight"):
            call(min_weight=bad)
    for bad in ("median", 0, None):
        with pytest.raises(ValueError, match="mode"):
            call(mode=bad)
    for bad in ("fill", 1, None):
        with pytest.raises(ValueError, match="holes"):
            call(holes=bad)
    with pytest.raises(ValueError, match="keep"):
        call(holes="keep")  # without out


def test_splat_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    gray = np.zeros((5, 4, 8), np.uint8)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    pay = np.zeros((5, 3, 4, 8), np.float32)
    imp = np.ones((5, 4, 8), np.float32)
    occ = np.zeros((5, 4, 8), np.uint8)
    for img in (gray, pay):
        _refused_settings(lambda **kw: eng.splat(img, flows, **kw))
    with pytest.raises(ValueError, match="images"):
        eng.splat(gray.astype(np.float64), flows)
    with pytest.raises(ValueError, match="images"):
        eng.splat(np.zeros((5, 4, 8, 2), np.uint8), flows)
    with pytest.raises(ValueError, match="images"):
        eng.splat(np.zeros((5, 3, 4, 8), np.uint8), flows)  # channels first needs layout="chw"
    with pytest.raises(ValueError, match="images"):
        eng.splat(np.zeros((5, 5, 4, 8), np.float32), flows)  # five channels
    with pytest.raises(ValueError, match="images"):
        eng.splat(np.zeros((5, 4, 8), np.float32), flows)  # a float payload names its channels
    with pytest.raises(ValueError, match="layout"):
        eng.splat(gray, flows, layout="nchw")
    with pytest.raises(ValueError, match="flows"):
        eng.splat(gray, flows[:4])
    with pytest.raises(ValueError, match="flows"):
        eng.splat(gray, flows.astype(np.float64))
    with pytest.raises(ValueError, match="importance"):
        eng.splat(gray, flows, importance=imp[:4])
    with pytest.raises(ValueError, match="occ"):
        eng.splat(gray, flows, occ=occ.astype(np.float32))
    with pytest.raises(ValueError, match="dtype"):
        eng.splat(gray, flows, dtype=np.float16)
    with pytest.raises(ValueError, match="dtype"):
        eng.splat(pay, flows, dtype=np.uint8)  # a float payload gives float32
    with pytest.raises(ValueError, match="sum"):
        eng.splat(gray, flows, mode="sum", dtype=np.uint8)
    with pytest.raises(ValueError, match="out"):
        eng.splat(gray, flows, holes="keep", out=np.zeros((5, 4, 8), np.float32))  # uint8 is the default dtype here
    with pytest.raises(ValueError, match="out"):
        eng.splat(gray, flows, holes="keep", out=np.zeros((4, 4, 8), np.uint8))
    # nothing to do never reaches the library either
    out, hole, cov = eng.splat(gray[:0], flows[:0], return_hole=True, return_coverage=True)
    assert out.shape == (0, 4, 8) and out.dtype == np.uint8 and hole.shape == (0, 4, 8) and cov.dtype == np.float32
    assert eng.splat(pay[:0], flows[:0]).shape == (0, 3, 4, 8)
    assert eng.splat(gray[:0], flows[:0], mode="sum").dtype == np.float32


def test_splat_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    gray = torch.zeros((5, 4, 8), dtype=torch.uint8)
    bgr = torch.zeros((5, 4, 8, 3), dtype=torch.uint8)
    pay = torch.zeros((5, 3, 4, 8))
    flows = torch.zeros((5, 2, 4, 8))
    imp = torch.ones((5, 4, 8))
    occ = torch.zeros((5, 4, 8), dtype=torch.uint8)
    for img in (gray, pay):
        _refused_settings(lambda **kw: eng.splat_tensor(img, flows, **kw))
    with pytest.raises(ValueError, match="images"):
        eng.splat_tensor(np.zeros((5, 4, 8), np.uint8), flows)
    with pytest.raises(ValueError, match="images"):
        eng.splat_tensor(gray.double(), flows)
    with pytest.raises(ValueError, match="images"):
        eng.splat_tensor(torch.zeros((5, 5, 4, 8)), flows)
    with pytest.raises(ValueError, match="innermost"):
        eng.splat_tensor(torch.zeros((5, 3, 4, 16))[..., ::2], flows)
    with pytest.raises(ValueError, match="overlap"):
        eng.splat_tensor(torch.zeros((1, 3, 4, 8)).expand(5, 3, 4, 8), flows)
    with pytest.raises(ValueError, match="interleaved"):
        eng.splat_tensor(torch.zeros((5, 4, 16, 3), dtype=torch.uint8)[:, :, ::2], flows)
    with pytest.raises(ValueError, match="flows"):
        eng.splat_tensor(gray, flows[:4])
    with pytest.raises(ValueError, match="flows"):
        eng.splat_tensor(gray, flows.double())
    with pytest.raises(ValueError, match="importance"):
        eng.splat_tensor(gray, flows, importance=imp.double())
    with pytest.raises(ValueError, match="occ"):
        eng.splat_tensor(gray, flows, occ=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="dtype"):
        eng.splat_tensor(gray, flows, dtype=torch.float16)
    with pytest.raises(ValueError, match="dtype"):
        eng.splat_tensor(pay, flows, dtype=torch.uint8)
    with pytest.raises(ValueError, match="sum"):
        eng.splat_tensor(bgr, flows, mode="sum", dtype=torch.uint8)
    with pytest.raises(ValueError, match="out"):
        eng.splat_tensor(gray, flows, out=torch.zeros((5, 4, 8)))  # uint8 is the default dtype here
    with pytest.raises(ValueError, match="out"):
        eng.splat_tensor(gray, flows, out=torch.zeros((4, 4, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="lie in memory"):
        eng.splat_tensor(bgr, flows, out=torch.zeros((5, 3, 4, 8), dtype=torch.uint8).permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match="in place"):
        eng.splat_tensor(gray, flows, out=gray)
    with pytest.raises(ValueError, match="work"):
        eng.splat_tensor(pay, flows, work=torch.zeros(4 * 8 * 4 * 8 - 1, dtype=torch.uint8))  # one byte short of 1 + 3 words
    with pytest.raises(ValueError, match="work"):
        eng.splat_tensor(gray, flows, work=torch.zeros((2, 2 * 4 * 8), dtype=torch.int64)[:, ::2])
    with pytest.raises(ValueError, match="work"):
        eng.splat_tensor(gray, flows, work=np.zeros(2 * 4 * 8, np.int64))
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.splat_tensor(bgr, flows, t=0.5, importance=imp, occ=occ, holes="keep", return_hole=True, return_coverage=True,
                         out=torch.zeros((5, 4, 8, 3), dtype=torch.uint8), work=torch.zeros(4 * 4 * 8, dtype=torch.int64))
