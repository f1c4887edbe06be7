"""The global-motion call at the binding level (no GPU): include/dfx.h declares dfx_global_motion_device, its descriptor, its
result record and constants at DFX_VERSION >= 460, libdfx.so exports the symbol, engine.py binds it with ctypes structures
that have the header's fields in the header's order, types, offsets and sizes (a C program compiled against the header prints
them), and the argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64,
          "uint32_t": C.c_uint32, "int64_t": C.c_int64}  # every pointer is a c_void_p
STRUCTS = {"dfx_gm_desc": "DfxGmDesc", "dfx_gm_result": "DfxGmResult"}


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
        d = re.fullmatch(r"(?:const )?(\w+) (\*?)(\w+)(?:\[(\d+)\])?", decl)
        assert d, decl
        t = C.c_void_p if d.group(2) else CTYPES[d.group(1)]
        fields.append((d.group(3), t * int(d.group(4)) if d.group(4) else t))
    return fields


def test_the_header_declares_the_entry_point_and_constants_at_version_460():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 460
    for name, value in {"DFX_GM_TRANSLATION": 0, "DFX_GM_AFFINE": 1}.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"\bint\s+dfx_global_motion_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_gm_desc\s*\*\s*d\s*\)\s*;", src)


@pytest.mark.parametrize("struct", list(STRUCTS))
def test_every_field_of_both_structs_is_documented(struct):
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + struct + ";", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(struct))
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln


def test_the_header_states_the_arithmetic_the_bound_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("homography and similarity models", "a median / histogram start", "soft (Tukey / Huber) weights",
                         "typed (float16 / bfloat16) output planes", "interleaved flows", "host-pointer and submit forms",
                         "fusing the fit into the flow calls", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("xc = 2x - (W-1)", "qu = (int)rintf(u * 256.0f)", "det = (S1*c00 + Sx*c01) + Sy*c02", "below 2^60",
                 "W, H <= 8192", "a0 = (P0 - P1*(W-1)) - P2*(H-1)", "leaves dfx_get_stats alone",
                 "dfx_device_bytes is unchanged", "no host synchronisation between rounds", "tests/global_motion_ref.py"):
        assert text in whole, text


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    assert hasattr(C.CDLL(dfx.library_path()), "dfx_global_motion_device")
    assert len(L.dfx_global_motion_device.argtypes) == 2
    assert L.dfx_global_motion_device.argtypes[1] is C.POINTER(E.DfxGmDesc)
    assert L.dfx_global_motion_device.restype is C.c_int
    assert E.GM_MODELS == {"translation": 0, "affine": 1} and E.GM_MAX_ROUNDS == 8


def test_the_ctypes_structures_are_the_headers(tmp_path):
    from denseflow_amd import engine as E

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None and os.path.exists("/opt/rocm/llvm/bin/clang"):
        cc = "/opt/rocm/llvm/bin/clang"
    assert cc, "needs a C compiler"
    assert len(_header_fields("dfx_gm_desc")) == 20 and len(_header_fields("dfx_gm_result")) == 8
    prints = ""
    for struct in STRUCTS:
        prints += f'    printf("{struct} sizeof %zu\\n", sizeof({struct}));\n'
        prints += "".join(f'    printf("{struct} {n} %zu\\n", offsetof({struct}, {n}));\n' for n, _ in _header_fields(struct))
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include "dfx.h"\nint main(void) {\n' + prints + "    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(prog), "-o", exe], check=True)
    got = {}
    for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, name, value = ln.split()
        got.setdefault(struct, {})[name] = int(value)
    for struct, cls_name in STRUCTS.items():
        cls = getattr(E, cls_name)
        fields = _header_fields(struct)
        assert [(n, t) for n, t in cls._fields_] == fields, struct
        assert got[struct].pop("sizeof") == C.sizeof(cls), struct
        assert got[struct] == {n: getattr(cls, n).offset for n, _ in fields}, struct
    # the documented layout of the record, and its NumPy twin
    assert C.sizeof(E.DfxGmResult) == 352 == E.GM_RESULT_DTYPE.itemsize
    assert {n: E.GM_RESULT_DTYPE.fields[n][1] for n in E.GM_RESULT_DTYPE.names} == {n: getattr(E.DfxGmResult, n).offset
                                                                                for n, _ in E.DfxGmResult._fields_}
    whole = open(os.path.join(ROOT, "include", "dfx.h")).read()
    for n, _ in E.DfxGmResult._fields_:
        assert re.search(r"\b" + n + r"(\[\d+\])?;\s*/\* offset " + str(getattr(E.DfxGmResult, n).offset) + ":", whole), n


class _Untouchable:
    """Stands where the loaded library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_engine(dfx, w=8, h=4):
    eng = object.__new__(dfx.FlowEngine)  # no handle, no device: everything below must be refused before either is needed
    eng.width, eng.height, eng._device = w, h, 0
    eng._L, eng._h = _Untouchable(), None
    return eng


def test_global_motion_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((2, 2, 4, 8), np.float32)
    for bad in ("rigid", 1, None):
        with pytest.raises(ValueError, match="model"):
            eng.global_motion(flows, model=bad)
    for bad in (0, 9, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="rounds"):
            eng.global_motion(flows, rounds=bad)
    for bad in (0.0, -0.5, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError, match="thr"):
            eng.global_motion(flows, thr=bad)
    for bad in (0.5, float("nan"), float("inf"), -2.0):
        with pytest.raises(ValueError, match="growth"):
            eng.global_motion(flows, growth=bad)
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion(flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion(np.zeros((2, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion(np.zeros((2, 2, 4, 9), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.global_motion(flows, mask=np.zeros((2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.global_motion(flows, mask=np.zeros((1, 4, 8), np.uint8))


def test_global_motion_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((2, 2, 4, 8))
    with pytest.raises(ValueError, match="model"):
        eng.global_motion_tensor(flows, model="homography")
    with pytest.raises(ValueError, match="rounds"):
        eng.global_motion_tensor(flows, rounds=0)
    with pytest.raises(ValueError, match="thr"):
        eng.global_motion_tensor(flows, thr=0.0)
    with pytest.raises(ValueError, match="growth"):
        eng.global_motion_tensor(flows, growth=0.9)
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion_tensor(flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion_tensor(np.zeros((2, 2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.global_motion_tensor(torch.zeros((2, 4, 8, 2)).permute(0, 3, 1, 2))  # interleaved (u, v) pixels
    with pytest.raises(ValueError, match="innermost"):
        eng.global_motion_tensor(torch.zeros((2, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="overlap"):
        eng.global_motion_tensor(torch.zeros((1, 2, 4, 8)).expand(2, 2, 4, 8))  # flows on top of each other
    with pytest.raises(ValueError, match="overlap"):
        eng.global_motion_tensor(torch.zeros((2, 1, 4, 8)).expand(2, 2, 4, 8))  # one plane shown twice
    with pytest.raises(ValueError, match="mask"):
        eng.global_motion_tensor(flows, mask=torch.zeros((2, 4, 8)))
    with pytest.raises(ValueError, match="mask"):
        eng.global_motion_tensor(flows, mask=torch.zeros((2, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="out"):
        eng.global_motion_tensor(flows, out=torch.zeros((2, 2, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="out"):
        eng.global_motion_tensor(flows, out=torch.zeros((3, 2, 4, 8)))
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.global_motion_tensor(flows, mask=torch.zeros((2, 4, 8), dtype=torch.uint8), out=flows)
