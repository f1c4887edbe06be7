"""The frame-interpolation call at the binding level (no GPU): include/dfx.h declares dfx_interpolate_device,
dfx_interpolate_work_bytes and the descriptor at DFX_VERSION >= 500, libdfx.so exports the symbols, engine.py binds them with a
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
STRUCT, CLASS = "dfx_interp_desc", "DfxInterpDesc"
FIELDS = ["d_img0", "d_img1", "channels", "layout", "img_pitch", "img_plane_stride", "img_image_stride",
          "d_fwd", "d_bwd", "row_pitch_floats", "plane_stride_floats", "flow_stride_floats",
          "n", "t", "min_weight", "fill_passes", "ksize",
          "d_occ_fwd", "d_occ_bwd", "occ_pitch", "occ_stride",
          "out_dtype", "d_out", "out_pitch", "out_plane_stride", "out_image_stride",
          "d_source", "source_pitch", "source_stride",
          "d_work", "work_bytes"]


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


def test_the_header_declares_the_entry_points_at_version_500():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 500
    assert re.search(r"\bint\s+dfx_interpolate_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_interp_desc\s*\*\s*d\s*\)\s*;", src)
    assert re.search(r"\bsize_t\s+dfx_interpolate_work_bytes\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_interp_desc\s*\*\s*d\s*\)\s*;", src)
    assert "(0.5.0)" in open(os.path.join(ROOT, "include", "dfx.h")).read()


def test_every_field_of_the_struct_is_documented():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", src, flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 31
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == FIELDS


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    whole = re.sub(r"\s*\n\s*\*\s*", " ", src)
    for out_of_scope in ("float16 / bfloat16 outputs", "several t per call", "softmax splatting of the images themselves",
                         "photometric statistics against a held-out frame", "bicubic sampling", "host-pointer and submit forms",
                         "fusing the interpolation into dfx_calc_batch_bidir_device", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("t1 = 1.0f - t", "scale = -t, min_weight, d_occ_fwd", "t = t1, scale = -t1", "scale = t1; the sums are the same, so H1 = H0",
                 "mask_out fed back as the mask", "With fill_passes = 0, Gf = G and Hf = H",
                 "px = (float)x + gu;  py = (float)y + gv", "prim_k = (H_k == 0) && inside_k;   cand_k = (Hf_k == 0) && inside_k",
                 "(w0, w1) = (prim_0 || prim_1) ? (prim_0, prim_1) : (cand_0, cand_1)", "o = s0 + t*(s1 - s0)",
                 "P0 + t*(P1 - P0)", "o = fminf(fmaxf(o, 0), 255)", "(uint8)rintf(o)", "3 never carries 4",
                 "no fused multiply-add", "rated LOW", "leaves dfx_get_stats alone", "dfx_device_bytes is unchanged",
                 "tests/interpolate_ref.py", "bit for bit in d_out and d_source", "d_work not 8-byte aligned",
                 "the result does not depend on how many pairs share a wave", "d_occ_bwd without d_bwd"):
        assert text in whole, text
    # the projection section's text stays: it still names the consumer
    assert "the two flows a frame interpolator warps both frames by (Baker et al. 2011; dfx_warp_device does that warp)" in whole


def test_the_reference_module_states_the_same_arithmetic():
    from tests import interpolate_ref as R

    doc = " ".join(R.__doc__.split())
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    sec = src[src.index("and their flows (0.5.0)"):src.index("} dfx_interp_desc;")]
    lines = [" ".join(ln.strip().lstrip("*").split()) for ln in sec.splitlines()]
    first = next(i for i, ln in enumerate(lines) if ln.startswith("px = (float)x + gu"))
    last = next(i for i, ln in enumerate(lines) if ln.startswith("(the filled flows) decided"))
    for ln in lines[first:last + 1]:
        assert ln in doc, ln


def test_the_library_exports_and_the_binding_binds_the_symbols(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    raw = C.CDLL(dfx.library_path())
    assert hasattr(raw, "dfx_interpolate_device") and hasattr(raw, "dfx_interpolate_work_bytes")
    assert len(L.dfx_interpolate_device.argtypes) == 2
    assert L.dfx_interpolate_device.argtypes[1] is C.POINTER(E.DfxInterpDesc)
    assert L.dfx_interpolate_device.restype is C.c_int
    assert L.dfx_interpolate_work_bytes.restype is C.c_size_t and len(L.dfx_interpolate_work_bytes.argtypes) == 2
    for name in ("interpolate", "interpolate_tensor", "interpolate_device", "interpolate_frames", "interpolate_work_bytes"):
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


def test_the_bindings_workspace_size_is_the_stated_layout():
    """Rows padded to 4 pixels, every region to 16 bytes: the sums (3 words per pixel), two flows of two planes and their
    twins, two hole planes and up to two mask planes per side, + 8 for taking the base up to 16 bytes."""
    from denseflow_amd import engine as E

    assert E._interp_work_bytes(8, 4, 0) == 3 * 8 * 32 + 16 * 32 + 2 * 32 + 8
    assert E._interp_work_bytes(8, 4, 1) == 3 * 8 * 32 + 2 * 16 * 32 + 2 * 2 * 32 + 8
    assert E._interp_work_bytes(8, 4, 2) == E._interp_work_bytes(8, 4, 16) == 3 * 8 * 32 + 2 * 16 * 32 + 3 * 2 * 32 + 8
    assert E._interp_work_bytes(5, 3, 0) == 368 + 16 * 24 + 48 + 8  # 15 pixels of sums (360 -> 368), rows of 8


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
    for bad in (0, 0.0, 1, 1.0, -0.5, 1.5, float("nan"), float("inf"), 1e-50, None, "0.5", True):
        with pytest.raises(ValueError, match="t must"):
            call(t=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "0.25", True):
        with pytest.raises(ValueError, match="min_weight"):
            call(min_weight=bad)
    for bad in (-1, 17, 1.0, None, "3", True):
        with pytest.raises(ValueError, match="fill_passes"):
            call(fill_passes=bad)
    for bad in (1, 4, 7, 3.0, None, "3", True):
        with pytest.raises(ValueError, match="ksize"):
            call(ksize=bad)


def test_interpolate_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    img = np.zeros((5, 4, 8), np.uint8)
    bgr = np.zeros((5, 4, 8, 3), np.uint8)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    occ = np.zeros((5, 4, 8), np.uint8)
    _refused_settings(lambda **kw: eng.interpolate(img, img, flows, **kw))
    with pytest.raises(ValueError, match="img0"):
        eng.interpolate(img.astype(np.float32), img, flows)
    with pytest.raises(ValueError, match="img1"):
        eng.interpolate(img, img.astype(np.int8), flows)
    with pytest.raises(ValueError, match="img1"):
        eng.interpolate(img, bgr, flows)
    with pytest.raises(ValueError, match="img0"):
        eng.interpolate(bgr, bgr, flows, layout="chw")
    with pytest.raises(ValueError, match="layout"):
        eng.interpolate(bgr, bgr, flows, layout="nhwc")
    with pytest.raises(ValueError, match="dtype"):
        eng.interpolate(img, img, flows, dtype=np.float16)
    with pytest.raises(ValueError, match="fwd"):
        eng.interpolate(img, img, flows.astype(np.float64))
    with pytest.raises(ValueError, match="fwd"):
        eng.interpolate(img, img, flows[:4])
    with pytest.raises(ValueError, match="bwd"):
        eng.interpolate(img, img, flows, np.zeros((5, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="occ_fwd"):
        eng.interpolate(img, img, flows, occ_fwd=occ.astype(np.float32))
    with pytest.raises(ValueError, match="occ_bwd needs bwd"):
        eng.interpolate(img, img, flows, occ_bwd=occ)
    with pytest.raises(ValueError, match="occ_bwd"):
        eng.interpolate(img, img, flows, flows, occ_bwd=occ[:4])
    # nothing to do never reaches the library either
    out, source = eng.interpolate(img[:0], img[:0], flows[:0], want_source=True)
    assert out.shape == (0, 4, 8) and out.dtype == np.uint8 and source.shape == (0, 4, 8)
    assert eng.interpolate(bgr[:0], bgr[:0], flows[:0], dtype=np.float32).shape == (0, 4, 8, 3)
    with pytest.raises(ValueError, match="step"):
        eng.interpolate_frames(list(img), step=0)
    with pytest.raises(ValueError, match="t must"):
        eng.interpolate_frames(list(img), ts=(0.5, 1.0))
    with pytest.raises(ValueError, match="frame shape"):
        eng.interpolate_frames([np.zeros((4, 9), np.uint8)] * 3)
    assert eng.interpolate_frames(list(img[:1])).shape == (0, 1, 4, 8)
    assert eng.interpolate_frames(list(img), ts=()).shape == (4, 0, 4, 8)


def test_interpolate_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    from denseflow_amd import engine as E

    eng = _bare_engine(dfx)
    img = torch.zeros((5, 4, 8), dtype=torch.uint8)
    flows = torch.zeros((5, 2, 4, 8))
    occ = torch.zeros((5, 4, 8), dtype=torch.uint8)
    _refused_settings(lambda **kw: eng.interpolate_tensor(img, img, flows, **kw))
    with pytest.raises(ValueError, match="img0"):
        eng.interpolate_tensor(img.float(), img, flows)
    with pytest.raises(ValueError, match="img1"):
        eng.interpolate_tensor(img, np.zeros((5, 4, 8), np.uint8), flows)
    with pytest.raises(ValueError, match="img1"):
        eng.interpolate_tensor(img, torch.zeros((5, 4, 16), dtype=torch.uint8)[..., :8], flows)  # other strides
    with pytest.raises(ValueError, match="img0"):
        eng.interpolate_tensor(torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2], img, flows)
    with pytest.raises(ValueError, match="dtype"):
        eng.interpolate_tensor(img, img, flows, dtype=torch.float16)
    with pytest.raises(ValueError, match="fwd"):
        eng.interpolate_tensor(img, img, flows.double())
    with pytest.raises(ValueError, match="fwd"):
        eng.interpolate_tensor(img, img, torch.zeros((5, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="bwd"):
        eng.interpolate_tensor(img, img, flows, torch.zeros((5, 2, 4, 16))[..., :8])  # not fwd's strides
    with pytest.raises(ValueError, match="occ_fwd"):
        eng.interpolate_tensor(img, img, flows, occ_fwd=occ.float())
    with pytest.raises(ValueError, match="occ_bwd needs bwd"):
        eng.interpolate_tensor(img, img, flows, occ_bwd=occ)
    with pytest.raises(ValueError, match="occ_bwd"):
        eng.interpolate_tensor(img, img, flows, flows, occ_fwd=occ, occ_bwd=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., :8])
    with pytest.raises(ValueError, match="out"):
        eng.interpolate_tensor(img, img, flows, out=torch.zeros((5, 4, 8)))
    with pytest.raises(ValueError, match="out"):
        eng.interpolate_tensor(img, img, flows, out=torch.zeros((4, 4, 8), dtype=torch.uint8))
    per = E._interp_work_bytes(8, 4, 3)
    with pytest.raises(ValueError, match="work"):
        eng.interpolate_tensor(img, img, flows, work=torch.zeros(per - 1, dtype=torch.uint8))  # one byte short
    with pytest.raises(ValueError, match="work"):
        eng.interpolate_tensor(img, img, flows, work=torch.zeros((2, per), dtype=torch.uint8)[:, ::2])
    with pytest.raises(ValueError, match="work"):
        eng.interpolate_tensor(img, img, flows, work=np.zeros(per, np.uint8))
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.interpolate_tensor(img, img, flows, flows, t=0.25, occ_fwd=occ, occ_bwd=occ, want_source=True, out=torch.zeros_like(img),
                               work=torch.zeros(per, dtype=torch.uint8))
