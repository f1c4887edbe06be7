"""The flow-chain call at the binding level (no GPU): include/dfx.h declares dfx_flow_chain_device, its descriptor and
constants at DFX_VERSION >= 480, libdfx.so exports the symbol, engine.py binds it with a ctypes structure that has the
header's fields in the header's order, types, offsets and size (a C program compiled against the header prints them), and
the argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}  # every pointer is a c_void_p
STRUCT, CLASS = "dfx_chain_desc", "DfxChainDesc"


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


def test_the_header_declares_the_entry_point_and_constants_at_version_480():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 480
    for name, value in {"DFX_CHAIN_LAST": 0, "DFX_CHAIN_ALL": 1, "DFX_WARP_BORDER_ZERO": 0, "DFX_WARP_BORDER_CLAMP": 1}.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"\bint\s+dfx_flow_chain_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_chain_desc\s*\*\s*d\s*\)\s*;", src)


def test_every_field_of_the_struct_is_documented():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 22
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == [
        "d_flow", "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n", "first", "hop", "length", "anchors",
        "anchor_step", "emit", "border", "d_occ", "occ_pitch", "occ_stride", "d_out", "out_row_pitch_floats",
        "out_plane_stride_floats", "out_flow_stride_floats", "d_valid", "valid_pitch", "valid_stride"]


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("forward splatting and flow inversion", "bicubic sampling", "typed (float16 / bfloat16) planes",
                         "interleaved flows", "host-pointer and submit forms",
                         "fusing the chain into dfx_calc_batch_bidir_device",
                         "a helper that re-estimates a seeded long-range flow", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("A_{k+1}(p) = A_k(p) + F_k(p + A_k(p))", "A_0 = (+0, +0) and valid_0 = 1", "px = (float)x + Au;  py = (float)y + Av",
                 "t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0])", "s_c = t + ay*(b - t)", "A unchanged, bit for bit",
                 "(ax > 0 ? occ[y0][x1] : 0)", "valid_{k+1} = valid_k && inside && !occluded", "no fused multiply-add",
                 "subnormals kept", "valid never comes back once lost", "0 * (inf - x) is NaN",
                 "it does not say whether the end point p + A_k lies inside the last frame", "first + j*anchor_step + k*hop",
                 "leaves dfx_get_stats alone", "dfx_device_bytes is unchanged", "d_out == d_flow", "tests/flow_chain_ref.py",
                 "NaN where it is"):
        assert text in whole, text


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    assert hasattr(C.CDLL(dfx.library_path()), "dfx_flow_chain_device")
    assert len(L.dfx_flow_chain_device.argtypes) == 2
    assert L.dfx_flow_chain_device.argtypes[1] is C.POINTER(E.DfxChainDesc)
    assert L.dfx_flow_chain_device.restype is C.c_int
    assert E.CHAIN_EMITS == {"last": 0, "all": 1}


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
    """The settings every wrapper refuses, on 5 flows."""
    for bad in (0, -1, 1.0, True, "2", None):
        with pytest.raises(ValueError, match="length"):
            call(length=bad)
    for bad in (0, 1.0, False, "1", None):
        with pytest.raises(ValueError, match="hop"):
            call(length=2, hop=bad)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="anchor_step"):
            call(length=2, anchor_step=bad)
    for bad in (-1, 1.5, True, "1"):
        with pytest.raises(ValueError, match="anchors"):
            call(length=2, anchors=bad)
    for bad in (1.0, True, None):
        with pytest.raises(ValueError, match="first"):
            call(length=2, first=bad)
    for bad in ("every", 0, None, "LAST"):
        with pytest.raises(ValueError, match="emit"):
            call(length=2, emit=bad)
    for bad in ("reflect", 0, None):
        with pytest.raises(ValueError, match="border"):
            call(length=2, border=bad)
    # link indices outside the 5 flows
    with pytest.raises(ValueError, match="first"):
        call(length=2, first=-1)
    with pytest.raises(ValueError, match="first"):
        call(length=3, first=1, hop=-1)
    for kw in (dict(length=6, anchors=1), dict(length=2, anchors=5), dict(length=2, first=4, anchors=1),
               dict(length=3, hop=2, anchors=2), dict(length=2, anchors=3, anchor_step=2), dict(length=3, first=1, hop=-1, anchors=1),
               dict(length=1, first=5, anchors=1)):
        with pytest.raises(ValueError, match="anchors"):
            call(**kw)


def test_flow_chain_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    occ = np.zeros((5, 4, 8), np.uint8)
    _refused_settings(lambda **kw: eng.flow_chain(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain(flows.astype(np.float64), 2)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain(np.zeros((5, 4, 8, 2), np.float32), 2)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain(np.zeros((5, 2, 4, 9), np.float32), 2)
    with pytest.raises(ValueError, match="occ"):
        eng.flow_chain(flows, 2, occ=occ.astype(np.float32))
    with pytest.raises(ValueError, match="occ"):
        eng.flow_chain(flows, 2, occ=occ[:4])
    # nothing to do never reaches the library either: no chain fits, or none is asked for
    for kw in (dict(length=6), dict(length=2, anchors=0)):
        out, valid = eng.flow_chain(flows, emit="all", **kw)
        assert out.shape == (0, 2, 4, 8) and valid.shape == (0, 4, 8)


def test_flow_chain_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((5, 2, 4, 8))
    occ = torch.zeros((5, 4, 8), dtype=torch.uint8)
    _refused_settings(lambda **kw: eng.flow_chain_tensor(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain_tensor(flows.double(), 2)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain_tensor(np.zeros((5, 2, 4, 8), np.float32), 2)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_chain_tensor(torch.zeros((5, 4, 8, 2)).permute(0, 3, 1, 2), 2)  # interleaved (u, v) pixels
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_chain_tensor(torch.zeros((5, 2, 4, 16))[..., ::2], 2)
    with pytest.raises(ValueError, match="overlap"):
        eng.flow_chain_tensor(torch.zeros((1, 2, 4, 8)).expand(5, 2, 4, 8), 2)  # flows on top of each other
    with pytest.raises(ValueError, match="occ"):
        eng.flow_chain_tensor(flows, 2, occ=occ.float())
    with pytest.raises(ValueError, match="occ"):
        eng.flow_chain_tensor(flows, 2, occ=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="out"):
        eng.flow_chain_tensor(flows, 2, out=torch.zeros((4, 2, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        eng.flow_chain_tensor(flows, 2, out=torch.zeros((3, 2, 4, 8)))  # 4 chains of 2 links fit
    with pytest.raises(ValueError, match="out"):
        eng.flow_chain_tensor(flows, 2, emit="all", out=torch.zeros((4, 2, 4, 8)))  # 8 output flows
    with pytest.raises(ValueError, match="in place"):
        eng.flow_chain_tensor(flows, 1, out=flows)
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.flow_chain_tensor(flows, 2, occ=occ, emit="all", border="clamp", out=torch.zeros((8, 2, 4, 8)))
