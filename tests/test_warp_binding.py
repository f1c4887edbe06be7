"""The backward warp at the binding level (no GPU): include/dfx.h declares dfx_warp_device, its descriptor and constants at
DFX_VERSION >= 450, libdfx.so exports the symbol, engine.py binds it with a ctypes structure that has the header's fields in
the header's order, types, offsets and size (a C program compiled against the header prints them), and the argument checks of
the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t}  # every pointer is a c_void_p


def _header():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_fields():
    """[(name, ctypes type)] of dfx_warp_desc as the header declares it."""
    m = re.search(r"typedef struct \{([^{}]*)\}\s*dfx_warp_desc;", _header())
    assert m, "include/dfx.h does not declare dfx_warp_desc"
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        d = re.fullmatch(r"(?:const )?(\w+) (\*?)(\w+)", decl)
        assert d, decl
        fields.append((d.group(3), C.c_void_p if d.group(2) else CTYPES[d.group(1)]))
    return fields


def test_the_header_declares_the_entry_point_and_constants_at_version_450():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 450
    for name, value in {"DFX_WARP_U8": 3, "DFX_WARP_BORDER_ZERO": 0, "DFX_WARP_BORDER_CLAMP": 1}.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"\bint\s+dfx_warp_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_warp_desc\s*\*\s*d\s*\)\s*;", src)


def test_every_field_of_the_descriptor_is_documented():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*dfx_warp_desc;", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields())
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("float source images", "bicubic sampling", "a host-pointer form", "a submit form",
                         "fusing the warp into dfx_calc_batch_bidir_device", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    assert "leaves dfx_get_stats alone" in whole and "dfx_device_bytes is unchanged" in whole


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    assert hasattr(C.CDLL(dfx.library_path()), "dfx_warp_device")
    assert len(L.dfx_warp_device.argtypes) == 2 and L.dfx_warp_device.argtypes[1] is C.POINTER(E.DfxWarpDesc)
    assert L.dfx_warp_device.restype is C.c_int
    assert E.WARP_U8 == 3 and E.WARP_BORDERS == {"zero": 0, "clamp": 1}


def test_the_ctypes_structure_is_the_headers(tmp_path):
    from denseflow_amd import engine as E

    fields = _header_fields()
    assert len(fields) == 25
    assert [(n, t) for n, t in E.DfxWarpDesc._fields_] == fields
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None and os.path.exists("/opt/rocm/llvm/bin/clang"):
        cc = "/opt/rocm/llvm/bin/clang"
    assert cc, "needs a C compiler"
    prog = tmp_path / "layout.c"
    prints = "".join(f'    printf("{n} %zu\\n", offsetof(dfx_warp_desc, {n}));\n' for n, _ in fields)
    prog.write_text('#include <stdio.h>\n#include "dfx.h"\nint main(void) {\n    printf("sizeof %zu\\n", sizeof(dfx_warp_desc));\n'
                    + prints + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got.pop("sizeof")) == C.sizeof(E.DfxWarpDesc)
    assert {n: int(v) for n, v in got.items()} == {n: getattr(E.DfxWarpDesc, n).offset for n, _ in fields}


class _Untouchable:
    """Stands where the loaded library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_engine(dfx, w=8, h=4):
    eng = object.__new__(dfx.FlowEngine)  # no handle, no device: everything below must be refused before either is needed
    eng.width, eng.height, eng._device = w, h, 0
    eng._L, eng._h = _Untouchable(), None
    return eng


def test_warp_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    img, img3, flows = np.zeros((2, 4, 8), np.uint8), np.zeros((2, 4, 8, 3), np.uint8), np.zeros((2, 2, 4, 8), np.float32)
    with pytest.raises(ValueError, match="border"):
        eng.warp(img, flows, border="reflect")
    with pytest.raises(ValueError, match="layout"):
        eng.warp(img3, flows, layout="nchw")
    for bad in (np.float64, np.int8, "half", object()):
        with pytest.raises(ValueError, match="dtype"):
            eng.warp(img, flows, dtype=bad)
    with pytest.raises(ValueError, match="uint8"):
        eng.warp(img.astype(np.float32), flows)
    with pytest.raises(ValueError, match="images must be"):
        eng.warp(np.zeros((2, 4, 9), np.uint8), flows)
    with pytest.raises(ValueError, match="images must be"):
        eng.warp(img3, flows, layout="chw")  # interleaved images declared channels-first
    with pytest.raises(ValueError, match="images must be"):
        eng.warp(np.zeros((2, 3, 4, 8), np.uint8), flows)  # and the other way round
    with pytest.raises(ValueError, match="flows"):
        eng.warp(img, flows[:1])
    with pytest.raises(ValueError, match="flows"):
        eng.warp(img, flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.warp(img, np.zeros((2, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="want_stats needs ref"):
        eng.warp(img, flows, want_stats=True)
    with pytest.raises(ValueError, match="ref"):
        eng.warp(img, flows, ref=img3)
    with pytest.raises(ValueError, match="occ"):
        eng.warp(img, flows, occ=np.zeros((2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="occ"):
        eng.warp(img, flows, occ=np.zeros((1, 4, 8), np.uint8))


def test_warp_error_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    frames = np.zeros((4, 4, 8), np.uint8)
    with pytest.raises(ValueError, match="step"):
        eng.warp_error(frames, np.zeros((4, 2, 4, 8), np.float32), 0)
    with pytest.raises(ValueError, match="frames"):
        eng.warp_error(frames.astype(np.int16), np.zeros((3, 2, 4, 8), np.float32), 1)
    with pytest.raises(ValueError, match="frames"):
        eng.warp_error(np.zeros((4, 5, 8), np.uint8), np.zeros((3, 2, 4, 8), np.float32), 1)
    with pytest.raises(ValueError, match="flows"):
        eng.warp_error(frames, np.zeros((3, 2, 4, 8), np.float32), 2)  # two flows for step 2, not three
    with pytest.raises(ValueError, match="flows"):
        eng.warp_error(frames, np.zeros((3, 2, 4, 8), np.float32), -2)
    with pytest.raises(ValueError, match="occ"):
        eng.warp_error(frames, np.zeros((3, 2, 4, 8), np.float32), -1, occ=np.zeros((4, 4, 8), np.uint8))


def test_warp_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    img = torch.zeros((2, 4, 8), dtype=torch.uint8)
    chw = torch.zeros((2, 3, 4, 8), dtype=torch.uint8)
    flows = torch.zeros((2, 2, 4, 8))
    with pytest.raises(ValueError, match="dtype"):
        eng.warp_tensor(img, flows, dtype=torch.float64)
    with pytest.raises(ValueError, match="dtype"):
        eng.warp_tensor(img, flows, dtype=np.uint8)  # numpy's, not torch's
    with pytest.raises(ValueError, match="border"):
        eng.warp_tensor(img, flows, border="wrap")
    with pytest.raises(ValueError, match="layout"):
        eng.warp_tensor(img, flows, layout="nhwc")
    with pytest.raises(ValueError, match="uint8"):
        eng.warp_tensor(img.float(), flows)
    with pytest.raises(ValueError, match="images must be"):
        eng.warp_tensor(torch.zeros((2, 4, 9), dtype=torch.uint8), flows)
    with pytest.raises(ValueError, match="innermost"):
        eng.warp_tensor(torch.zeros((2, 4, 16), dtype=torch.uint8)[..., ::2], flows)
    with pytest.raises(ValueError, match="overlap"):
        eng.warp_tensor(torch.zeros((1, 4, 8), dtype=torch.uint8).expand(2, 4, 8), flows)  # images on top of each other
    with pytest.raises(ValueError, match="overlap"):
        eng.warp_tensor(torch.zeros((2, 1, 4, 8), dtype=torch.uint8).expand(2, 3, 4, 8), flows)  # one plane shown three times
    with pytest.raises(ValueError, match="interleaved"):
        eng.warp_tensor(torch.zeros((2, 3, 4, 16), dtype=torch.uint8)[..., ::2], flows)
    with pytest.raises(ValueError, match="flows"):
        eng.warp_tensor(img, flows[:1])
    with pytest.raises(ValueError, match="flows"):
        eng.warp_tensor(img, flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.warp_tensor(img, torch.zeros((2, 4, 8, 2)).permute(0, 3, 1, 2))  # interleaved (u, v) pixels
    with pytest.raises(ValueError, match="want_stats needs ref"):
        eng.warp_tensor(img, flows, want_stats=True)
    with pytest.raises(ValueError, match="ref"):
        eng.warp_tensor(img, flows, ref=chw)
    with pytest.raises(ValueError, match="occ"):
        eng.warp_tensor(img, flows, occ=torch.zeros((2, 4, 8)))
    with pytest.raises(ValueError, match="out must be"):
        eng.warp_tensor(img, flows, out=torch.zeros((2, 4, 8)))  # a float32 out for the uint8 default
    with pytest.raises(ValueError, match="out must be"):
        eng.warp_tensor(img, flows, dtype=torch.float16, out=torch.zeros((2, 4, 9), dtype=torch.float16))
    with pytest.raises(ValueError, match="out must lie"):  # planar images, interleaved out
        eng.warp_tensor(chw, flows, out=torch.zeros((2, 4, 8, 3), dtype=torch.uint8).permute(0, 3, 1, 2))
    # everything right but CPU tensors: still refused before the library — contiguous NCHW, and the NCHW view of an NHWC batch
    with pytest.raises(ValueError, match="device"):
        eng.warp_tensor(chw, flows)
    with pytest.raises(ValueError, match="device"):
        eng.warp_tensor(torch.zeros((2, 4, 8, 3), dtype=torch.uint8).permute(0, 3, 1, 2), flows, dtype=torch.bfloat16)
