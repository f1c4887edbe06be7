"""The flow-projection call at the binding level (no GPU): include/dfx.h declares dfx_flow_project_device,
dfx_flow_project_work_bytes and the descriptor at DFX_VERSION >= 490, libdfx.so exports the symbols, engine.py binds them with a
ctypes structure that has the header's fields in the header's order, types, offsets and size (a C program compiled against
the header prints them), and the argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}  # every pointer is a c_void_p
STRUCT, CLASS = "dfx_project_desc", "DfxProjectDesc"
FIELDS = ["d_flow", "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n", "t", "scale", "min_weight",
          "d_importance", "importance_pitch_floats", "importance_stride_floats", "d_occ", "occ_pitch", "occ_stride", "d_out",
          "out_row_pitch_floats", "out_plane_stride_floats", "out_flow_stride_floats", "d_hole", "hole_pitch", "hole_stride",
          "d_coverage", "coverage_pitch_floats", "coverage_stride_floats", "d_work", "work_bytes"]


def _header():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


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


def test_the_header_declares_the_entry_points_at_version_490():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 490
    assert re.search(r"\bint\s+dfx_flow_project_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_project_desc\s*\*\s*d\s*\)\s*;", src)
    assert re.search(r"\bsize_t\s+dfx_flow_project_work_bytes\s*\(\s*dfx_handle\s+h\s*\)\s*;", src)
    assert "(0.4.9)" in open(os.path.join(ROOT, "include", "dfx.h")).read()


def test_every_field_of_the_struct_is_documented():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 26
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == FIELDS


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("splatting of images or arbitrary payloads (softmax splatting of frames)",
                         "typed (float16 / bfloat16) planes and interleaved flows", "host-pointer and submit forms",
                         "fusing the projection into dfx_calc_batch_bidir_device", "an importance computed by the library",
                         "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("skip the pixel if d_occ != NULL and occ[y][x] != 0", "px = (float)x + t*fu;   py = (float)y + t*fv",
                 "skip unless px > -1 && px < W && py > -1 && py < H", "tested before any conversion to int",
                 "imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)",
                 "(iq = 0 contributes nothing)", "x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)",
                 "qu = (int)rintf(fminf(fmaxf(fu * 256.f, -8388608.f), 8388608.f));   qv likewise",
                 "column weights {256 - bx, bx} and row weights {256 - by, by}", "a tap outside [0, W) x [0, H) is dropped",
                 "wt = wx * wy * iq", "the four wx*wy add up to 65536 exactly",
                 "Wsum[tap] += wt (uint64);   Su[tap] += wt * qu;   Sv[tap] += wt * qv", "two's-complement wrap on both sides",
                 "Wmin = max(1, (uint64)llrint((double)min_weight * 16777216.0))", "hole = Wsum < Wmin",
                 "out_u = hole ? +0.0f : (float)(((double)Su / (double)Wsum) * ((double)scale / 256.0));   out_v likewise",
                 "(float)((double)Wsum / 16777216.0)", "no fused multiply-add",
                 "while |F| < 8192 px with fewer than 1024 maximum-importance sources on one target",
                 "0.25 is a choice", "leaves dfx_get_stats alone", "dfx_device_bytes is unchanged", "d_out == d_flow",
                 "tests/flow_project_ref.py", "bit for bit, the coverage plane included", "No float atomics",
                 "the result does not depend on how many flows share a wave", "d_work not 8-byte aligned"):
        assert text in whole, text
    # the chain section's text stays: its out-of-scope list still opens with this direction
    assert "Out of scope: forward splatting and flow inversion;" in whole


def test_the_reference_module_states_the_same_arithmetic():
    from tests import flow_project_ref as R

    doc = " ".join(R.__doc__.split())
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    sec = src[src.index("holes marked (0.4.9)"):src.index("} dfx_project_desc;")]
    lines = [" ".join(ln.strip().lstrip("*").split()) for ln in sec.splitlines()]
    first = next(i for i, ln in enumerate(lines) if ln.startswith("skip the pixel if"))
    last = next(i for i, ln in enumerate(lines) if ln.startswith("coverage plane (float32, optional)"))
    for ln in lines[first:last + 1]:
        assert ln in doc, ln


def test_the_library_exports_and_the_binding_binds_the_symbols(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    raw = C.CDLL(dfx.library_path())
    assert hasattr(raw, "dfx_flow_project_device") and hasattr(raw, "dfx_flow_project_work_bytes")
    assert len(L.dfx_flow_project_device.argtypes) == 2
    assert L.dfx_flow_project_device.argtypes[1] is C.POINTER(E.DfxProjectDesc)
    assert L.dfx_flow_project_device.restype is C.c_int
    assert L.dfx_flow_project_work_bytes.restype is C.c_size_t and len(L.dfx_flow_project_work_bytes.argtypes) == 1
    assert E.PROJECT_WORDS == 3
    for name in ("flow_project", "flow_project_tensor", "flow_project_device", "flow_invert", "flow_project_work_bytes"):
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
    for bad in (float("nan"), float("-inf"), 1e39, "1", False):
        with pytest.raises(ValueError, match="scale"):
            call(scale=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0.25", True):
        with pytest.raises(ValueError, match="min_weight"):
            call(min_weight=bad)


def test_flow_project_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    imp = np.ones((5, 4, 8), np.float32)
    occ = np.zeros((5, 4, 8), np.uint8)
    _refused_settings(lambda **kw: eng.flow_project(flows, **kw))
    with pytest.raises(ValueError, match="min_weight"):
        eng.flow_invert(flows, min_weight=-1.0)
    with pytest.raises(TypeError):
        eng.flow_invert(flows, t=0.5)  # flow_invert fixes t and scale
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project(flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project(np.zeros((5, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project(np.zeros((5, 2, 4, 9), np.float32))
    with pytest.raises(ValueError, match="importance"):
        eng.flow_project(flows, importance=imp.astype(np.float64))
    with pytest.raises(ValueError, match="importance"):
        eng.flow_project(flows, importance=imp[:4])
    with pytest.raises(ValueError, match="occ"):
        eng.flow_project(flows, occ=occ.astype(np.float32))
    with pytest.raises(ValueError, match="occ"):
        eng.flow_project(flows, occ=occ[:4])
    # nothing to do never reaches the library either
    out, hole, cov = eng.flow_project(flows[:0], coverage=True)
    assert out.shape == (0, 2, 4, 8) and hole.shape == (0, 4, 8) and cov.shape == (0, 4, 8) and cov.dtype == np.float32
    assert len(eng.flow_invert(flows[:0])) == 2


def test_flow_project_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((5, 2, 4, 8))
    imp = torch.ones((5, 4, 8))
    occ = torch.zeros((5, 4, 8), dtype=torch.uint8)
    _refused_settings(lambda **kw: eng.flow_project_tensor(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project_tensor(flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project_tensor(np.zeros((5, 2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_project_tensor(torch.zeros((5, 4, 8, 2)).permute(0, 3, 1, 2))  # interleaved (u, v) pixels
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_project_tensor(torch.zeros((5, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="overlap"):
        eng.flow_project_tensor(torch.zeros((1, 2, 4, 8)).expand(5, 2, 4, 8))  # flows on top of each other
    with pytest.raises(ValueError, match="importance"):
        eng.flow_project_tensor(flows, importance=imp.double())
    with pytest.raises(ValueError, match="importance"):
        eng.flow_project_tensor(flows, importance=torch.ones((5, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="occ"):
        eng.flow_project_tensor(flows, occ=occ.float())
    with pytest.raises(ValueError, match="occ"):
        eng.flow_project_tensor(flows, occ=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="out"):
        eng.flow_project_tensor(flows, out=torch.zeros((5, 2, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        eng.flow_project_tensor(flows, out=torch.zeros((4, 2, 4, 8)))
    with pytest.raises(ValueError, match="in place"):
        eng.flow_project_tensor(flows, out=flows)
    with pytest.raises(ValueError, match="work"):
        eng.flow_project_tensor(flows, work=torch.zeros(3 * 8 * 4 * 8 - 1, dtype=torch.uint8))  # one byte short
    with pytest.raises(ValueError, match="work"):
        eng.flow_project_tensor(flows, work=torch.zeros((2, 3 * 4 * 8), dtype=torch.int64)[:, ::2])
    with pytest.raises(ValueError, match="work"):
        eng.flow_project_tensor(flows, work=np.zeros(3 * 4 * 8, np.int64))
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.flow_project_tensor(flows, t=0.5, scale=0.5, importance=imp, occ=occ, coverage=True, out=torch.zeros((5, 2, 4, 8)),
                                work=torch.zeros(3 * 4 * 8, dtype=torch.int64))
