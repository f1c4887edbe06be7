"""The colour coding of flows at the binding level (no GPU): include/dfx.h declares dfx_flow_colour_device and the descriptor
at DFX_VERSION >= 501 with every field documented, libdfx.so exports the symbol, engine.py binds it with a ctypes structure
that has the header's fields in the header's order, types, offsets and size (a C program compiled against the header prints
them), and the argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "uint8_t": C.c_uint8}  # every pointer is a c_void_p
STRUCT, CLASS = "dfx_colour_desc", "DfxColourDesc"
FIELDS = ["d_flow", "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n",
          "d_mask", "mask_pitch", "mask_stride",
          "norm", "max_rad", "d_max2",
          "order", "layout", "d_out", "out_pitch", "out_plane_stride", "out_image_stride", "unknown",
          "d_frame", "frame_channels", "frame_layout", "frame_pitch", "frame_plane_stride", "frame_image_stride", "alpha256"]


def _raw():
    return open(os.path.join(ROOT, "include", "dfx.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


def _header_fields(struct):
    """[(name, ctypes type)] of a struct as the header declares it (name[k]: an array of k)."""
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


def test_the_header_declares_the_entry_point_at_version_501():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 501
    assert re.search(r"\bint\s+dfx_flow_colour_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_colour_desc\s*\*\s*d\s*\)\s*;", src)
    assert "(0.5.1)" in _raw()
    for name, value in (("DFX_COLOUR_NORM_FIXED", 0), ("DFX_COLOUR_NORM_FLOW", 1), ("DFX_COLOUR_NORM_BATCH", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name


def test_every_field_of_the_struct_is_documented():
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", _raw(), flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 25
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == FIELDS


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    whole = re.sub(r"\s*\n\s*\*\s*", " ", _raw())
    for out_of_scope in ("an HSV or cv::cartToPolar coding", "arrows or quiver overlays", "float or half-precision output images",
                         "JPEG files of the pictures", "interleaved or typed (float16 / bfloat16) input flows",
                         "host-pointer and submit forms", "fusing the colouring into the flow calls", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("RY 15, YG 6, GC 4, CB 11, BM 13, MR 6", "R 7773, G 5870, B 7395", "|u| <= 1e9f && |v| <= 1e9f",
                 "D = R + 0x1p-23f;  un = u / D;  vn = v / D;  rad = sqrtf(un*un + vn*vn)", "rad = fminf(rad, 1.0f)",
                 "a = atan2_turns(-vn, -un)", "t = mx > 0 ? mn / mx : 0", "if (signbit(x)) r = 3.1415927f - r",
                 "a = r * 0.31830987f", "c0 = 0x1.fffd5cp-1", "c5 = -0x1.81b21cp-7", "fk = (a + 1.0f) * 27.0f",
                 "k1 = (k0 == 54) ? 0 : k0 + 1", "col = (1.0f - f)*c0 + f*c1", "col = col*0.75f",
                 "byte = (uint8) fminf(fmaxf(floorf(255.0f*col), 0.0f), 255.0f)",
                 "out_c = (alpha256*byte_c + (256 - alpha256)*frame_c + 128) >> 8", "integer atomic max", "(255,114,0)",
                 "(191,0,0)", "tests/flow_colour_ref.py", "dfx_device_bytes is unchanged", "leaves dfx_get_stats alone",
                 "no host synchronisation between them", "A refused call writes nothing"):
        assert text in whole, text


def test_the_reference_module_states_the_same_arithmetic():
    from tests import flow_colour_ref as R

    doc = " ".join(R.__doc__.split())
    src = _raw()
    sec = src[src.index("unknown pixels marked (0.5.1)"):src.index("} dfx_colour_desc;")]
    lines = [" ".join(ln.strip().lstrip("*").split()) for ln in sec.splitlines()]
    for start, end in (("ax = |x|, ay = |y|", "a = r * 0.31830987f"), ("fk = (a + 1.0f) * 27.0f", "k1 = (k0 == 54)"),
                       ("col = (1.0f - f)*c0", "byte = (uint8)")):
        first = next(i for i, ln in enumerate(lines) if ln.startswith(start))
        last = next(i for i, ln in enumerate(lines) if ln.startswith(end))
        assert first < last
        for ln in lines[first:last + 1]:
            assert ln in doc, ln


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    raw = C.CDLL(dfx.library_path())
    assert hasattr(raw, "dfx_flow_colour_device")
    assert len(L.dfx_flow_colour_device.argtypes) == 2
    assert L.dfx_flow_colour_device.argtypes[1] is C.POINTER(E.DfxColourDesc)
    assert L.dfx_flow_colour_device.restype is C.c_int
    for name in ("flow_colour", "flow_colour_tensor", "flow_colour_device", "flow_colour_key"):
        assert callable(getattr(dfx.FlowEngine, name)), name
    assert callable(dfx.colour_wheel) and dfx.colour_wheel().shape == (55, 3)
    assert E.COLOUR_NORMS == {"fixed": 0, "flow": 1, "batch": 2}


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
    for bad in ("hsv", "FLOW", 1, None):
        with pytest.raises(ValueError, match="norm"):
            call(norm=bad)
    for bad in (None, 0, 0.0, -1.0, 1e-7, 1e10, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="max_rad"):
            call(norm="fixed", max_rad=bad)
    for norm in ("flow", "batch"):
        with pytest.raises(ValueError, match="max_rad"):
            call(norm=norm, max_rad=1.0)
    for bad in ("gbr", 0, None):
        with pytest.raises(ValueError, match="order"):
            call(order=bad)
    for bad in ("nhwc", 1, None):
        with pytest.raises(ValueError, match="layout"):
            call(layout=bad)
    for bad in ((0, 0), (0, 0, 256), (-1, 0, 0), (0.5, 0, 0), "abc", None, 7, (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="unknown"):
            call(unknown=bad)
    for bad in (-0.01, 1.01, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError, match="alpha"):
            call(alpha=bad)


def test_flow_colour_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    _refused_settings(lambda **kw: eng.flow_colour(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour(flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour(flows[:, :, :3])
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour(np.zeros((5, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_colour(flows, mask=np.zeros((5, 4, 8), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_colour(flows, mask=np.zeros((4, 4, 8), np.uint8))
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour(flows, frame=np.zeros((5, 4, 8), np.float32))
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour(flows, frame=np.zeros((5, 3, 4, 8), np.uint8))  # channels first under layout="hwc"
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour(flows, layout="chw", frame=np.zeros((5, 4, 8, 3), np.uint8))
    # nothing to do never reaches the library either
    out, radii, batch = eng.flow_colour(flows[:0], return_max=True)
    assert out.shape == (0, 4, 8, 3) and out.dtype == np.uint8 and radii.shape == (0,) and batch == 0
    assert eng.flow_colour(flows[:0], "fixed", 2.0, layout="chw").shape == (0, 3, 4, 8)
    for bad in (0, -3, 2.5, None, "65", True):
        with pytest.raises(ValueError, match="size"):
            eng.flow_colour_key(bad)


def test_flow_colour_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((5, 2, 4, 8))
    _refused_settings(lambda **kw: eng.flow_colour_tensor(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour_tensor(flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour_tensor(np.zeros((5, 2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_colour_tensor(torch.zeros((5, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="mask"):
        eng.flow_colour_tensor(flows, mask=torch.zeros((5, 4, 8)))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_colour_tensor(flows, mask=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour_tensor(flows, frame=torch.zeros((5, 4, 8)))
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour_tensor(flows, frame=torch.zeros((4, 4, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="frame"):
        eng.flow_colour_tensor(flows, frame=torch.zeros((5, 4, 8, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out"):
        eng.flow_colour_tensor(flows, out=torch.zeros((5, 4, 8, 3)))
    with pytest.raises(ValueError, match="out"):
        eng.flow_colour_tensor(flows, out=torch.zeros((5, 3, 4, 8), dtype=torch.uint8))  # the shape of layout="chw"
    with pytest.raises(ValueError, match="out"):
        eng.flow_colour_tensor(flows, out=torch.zeros((5, 4, 8, 6), dtype=torch.uint8)[..., ::2])
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.flow_colour_tensor(flows, "batch", mask=torch.zeros((5, 4, 8), dtype=torch.uint8), order="bgr", layout="chw",
                               frame=torch.zeros((5, 4, 8), dtype=torch.uint8), alpha=0.25, return_max=True,
                               out=torch.zeros((5, 3, 4, 8), dtype=torch.uint8))
