"""The flow-median call at the binding level (no GPU): include/dfx.h declares dfx_flow_median_device, its descriptor and
constants at DFX_VERSION >= 470, libdfx.so exports the symbol, engine.py binds it with a ctypes structure that has the
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
STRUCT, CLASS = "dfx_median_desc", "DfxMedianDesc"


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


def test_the_header_declares_the_entry_point_and_constants_at_version_470():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 470
    for name, value in {"DFX_MEDIAN_ALL": 0, "DFX_MEDIAN_FILL": 1}.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"\bint\s+dfx_flow_median_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_median_desc\s*\*\s*d\s*\)\s*;", src)


def test_every_field_of_the_struct_is_documented():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 17
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("the median inside the TVL1 iteration", "ksize 7 and above", "weighted or bilateral (image-guided) medians",
                         "a joint vector median of (u, v)", "interleaved flows", "typed (float16 / bfloat16) planes",
                         "host-pointer and submit forms", "fusing the filter into the bidirectional call",
                         "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("key(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)", "(clamp(x + dx, 0, W-1), clamp(y + dy, 0, H-1))",
                 "rank (m - 1) >> 1", "with -0 below +0", "out = in bit for bit and mask_out = 1", "leaves dfx_get_stats alone",
                 "dfx_device_bytes is unchanged", "d_out == d_flow", "d_mask_out == d_mask", "tests/flow_median_ref.py",
                 "the bit pattern of one input sample"):
        assert text in whole, text


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    assert hasattr(C.CDLL(dfx.library_path()), "dfx_flow_median_device")
    assert len(L.dfx_flow_median_device.argtypes) == 2
    assert L.dfx_flow_median_device.argtypes[1] is C.POINTER(E.DfxMedianDesc)
    assert L.dfx_flow_median_device.restype is C.c_int
    assert E.MEDIAN_MODES == {"all": 0, "fill": 1}


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


def test_flow_median_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((2, 2, 4, 8), np.float32)
    mask = np.zeros((2, 4, 8), np.uint8)
    for bad in (1, 4, 7, 0, -3, 3.0, True, "5", None):
        with pytest.raises(ValueError, match="ksize"):
            eng.flow_median(flows, ksize=bad)
    for bad in ("median", 0, None, "ALL"):
        with pytest.raises(ValueError, match="mode"):
            eng.flow_median(flows, mode=bad)
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median(flows, mode="fill")
    for bad in (0, -1, 65, 1.5, True, "2"):
        with pytest.raises(ValueError, match="passes"):
            eng.flow_median(flows, passes=bad)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median(flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median(np.zeros((2, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median(np.zeros((2, 2, 4, 9), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median(flows, mask=mask.astype(np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median(flows, mask=mask[:1])


def test_flow_median_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((2, 2, 4, 8))
    mask = torch.zeros((2, 4, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="ksize"):
        eng.flow_median_tensor(flows, ksize=7)
    with pytest.raises(ValueError, match="mode"):
        eng.flow_median_tensor(flows, mode="inpaint")
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median_tensor(flows, mode="fill")
    with pytest.raises(ValueError, match="passes"):
        eng.flow_median_tensor(flows, passes=0)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median_tensor(flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median_tensor(np.zeros((2, 2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_median_tensor(torch.zeros((2, 4, 8, 2)).permute(0, 3, 1, 2))  # interleaved (u, v) pixels
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_median_tensor(torch.zeros((2, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="overlap"):
        eng.flow_median_tensor(torch.zeros((1, 2, 4, 8)).expand(2, 2, 4, 8))  # flows on top of each other
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median_tensor(flows, mask=mask.float())
    with pytest.raises(ValueError, match="mask"):
        eng.flow_median_tensor(flows, mask=torch.zeros((2, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="out"):
        eng.flow_median_tensor(flows, out=torch.zeros((2, 2, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        eng.flow_median_tensor(flows, out=torch.zeros((3, 2, 4, 8)))
    with pytest.raises(ValueError, match="in place"):
        eng.flow_median_tensor(flows, out=flows)
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.flow_median_tensor(flows, mask=mask, mode="fill", passes=2, out=torch.zeros((2, 2, 4, 8)))
