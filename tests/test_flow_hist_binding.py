"""The motion descriptors of flows at the binding level (no GPU): include/dfx.h declares dfx_flow_hist_device and the descriptor
at DFX_VERSION >= 502 with every field documented and the arithmetic stated, libdfx.so exports the symbol, engine.py binds it
with a ctypes structure that has the header's fields in the header's order, types, offsets and size (a C program compiled
against the header prints them), and the argument checks of the wrappers fire before the library is reached."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "uint8_t": C.c_uint8}  # every pointer is a c_void_p
STRUCT, CLASS = "dfx_hist_desc", "DfxHistDesc"
FIELDS = ["d_flow", "row_pitch_floats", "plane_stride_floats", "flow_stride_floats", "n",
          "d_mask", "mask_pitch", "mask_stride",
          "kinds", "cell", "bins", "still_thr", "norm",
          "d_sums", "sums_stride",
          "d_out", "out_slot_stride_floats", "out_col_stride_floats", "out_row_stride_floats", "out_flow_stride_floats"]


def _raw():
    return open(os.path.join(ROOT, "include", "dfx.h")).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _raw(), flags=re.S)


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


def test_the_header_declares_the_entry_point_at_version_502():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 502
    assert re.search(r"\bint\s+dfx_flow_hist_device\s*\(\s*dfx_handle\s+h\s*,\s*const\s+dfx_hist_desc\s*\*\s*d\s*\)\s*;", src)
    assert "(0.5.2)" in _raw()
    for name, value in (("DFX_HIST_HOF", 1), ("DFX_HIST_MBHX", 2), ("DFX_HIST_MBHY", 4), ("DFX_HIST_NORM_NONE", 0),
                        ("DFX_HIST_NORM_L1", 1), ("DFX_HIST_NORM_L1_SQRT", 2), ("DFX_HIST_NORM_L2", 3)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", src), name


def test_every_field_of_the_struct_is_documented():
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*" + STRUCT + ";", _raw(), flags=re.S).group(1)
    lines = [ln for ln in body.splitlines() if ln.strip()]
    assert len(lines) == len(_header_fields(STRUCT)) == 20
    for ln in lines:
        assert re.search(r";\s*/\*.{10,}\*/\s*$", ln), ln
    assert [n for n, _ in _header_fields(STRUCT)] == FIELDS


def test_the_header_states_the_arithmetic_and_what_is_out_of_scope():
    whole = re.sub(r"\s*\n\s*\*\s*", " ", _raw())
    for out_of_scope in ("HOG (it needs the frames)", "block normalisation over several cells", "temporal cells",
                         "sampling descriptors along dfx_flow_chain_device's trajectories", "integral histograms",
                         "hard (nearest) binning", "typed or interleaved flows", "host-pointer and submit forms",
                         "fusing the histograms into the flow calls", "the host shell and its CLI"):
        assert out_of_scope in whole, out_of_scope
    for text in ("|u| <= 1e9f && |v| <= 1e9f", "gx = u(min(x+1, W-1), y) - u(max(x-1, 0), y)",
                 "gy = u(x, min(y+1, H-1)) - u(x, max(y-1, 0))", "cv::Sobel with ksize = 1", "m = sqrtf(gx*gx + gy*gy)",
                 "a = atan2_turns(gy, gx)", "Q = llrintf(m * 256.0f)", "hb = 0.5f * (float)bins", "fk = a * hb",
                 "if (fk < 0) fk = fk + (float)bins", "k0 = (int)floorf(fk)", "f  = fk - (float)k0",
                 "if (k0 == bins) { k0 = 0; f = 0; }", "k1 = (k0 + 1 == bins) ? 0 : k0 + 1", "F  = (int)rintf(f * 256.0f)",
                 "w1 = (Q * F + 128) >> 8", "w0 = Q - w1", "if m <= still_thr", "D = 9 + 8 + 8", "< 2^53",
                 "(float)((double)S_b / 256.0)", "T ? (float)((double)S_b / (double)T) : 0",
                 "T ? (float)sqrt((double)S_b / (double)T) : 0", "E > 0 ? (float)((double)S_b / sqrt(E)) : 0", "5792",
                 "tests/flow_hist_ref.py", "dfx_device_bytes is unchanged", "leaves dfx_get_stats alone",
                 "A refused call writes nothing", "sums_stride < CH * CW * D"):
        assert text in whole, text


def test_the_reference_module_states_the_same_arithmetic():
    from tests import flow_hist_ref as R

    doc = " ".join(R.__doc__.split())
    src = _raw()
    sec = src[src.index("HOF and MBH cell histograms (0.5.2)"):src.index("} dfx_hist_desc;")]
    # a remark in parentheses set off by three or more spaces is the header's comment on a line, not part of it
    lines = [" ".join(re.split(r"\s{3,}\(", ln.strip().lstrip("*").strip())[0].split()) for ln in sec.splitlines()]
    first = next(i for i, ln in enumerate(lines) if ln.startswith("hb = 0.5f"))
    last = next(i for i, ln in enumerate(lines) if ln.startswith("w0 = Q - w1"))
    assert last - first + 1 == 10  # the ten lines of the binning
    for ln in lines[first:last + 1]:
        assert len(ln) > 8 and ln in doc, ln
    for ln in ("m = sqrtf(gx*gx + gy*gy)", "Q = llrintf(m * 256.0f)"):
        assert ln in doc and any(x.startswith(ln) for x in lines), ln


def test_the_library_exports_and_the_binding_binds_the_symbol(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    raw = C.CDLL(dfx.library_path())
    assert hasattr(raw, "dfx_flow_hist_device")
    assert len(L.dfx_flow_hist_device.argtypes) == 2
    assert L.dfx_flow_hist_device.argtypes[1] is C.POINTER(E.DfxHistDesc)
    assert L.dfx_flow_hist_device.restype is C.c_int
    for name in ("flow_hist", "flow_hist_tensor", "flow_hist_device"):
        assert callable(getattr(dfx.FlowEngine, name)), name
    assert E.HIST_KINDS == {"hof": 1, "mbhx": 2, "mbhy": 4} and E.HIST_NORMS == {"none": 0, "l1": 1, "l1_sqrt": 2, "l2": 3}
    names = dfx.flow_hist_slots()
    assert names == [f"hof{b}" for b in range(8)] + ["hof_still"] + [f"mbhx{b}" for b in range(8)] + [f"mbhy{b}" for b in range(8)]
    assert dfx.flow_hist_slots("mbhy", 2) == ["mbhy0", "mbhy1"]
    assert dfx.flow_hist_slots(("mbhx", "hof"), 3) == ["hof0", "hof1", "hof2", "hof_still", "mbhx0", "mbhx1", "mbhx2"]
    for bad in ((), ("hog",), ("hof", "hof"), None, 7):
        with pytest.raises(ValueError, match="kinds"):
            dfx.flow_hist_slots(bad)
    for bad in (1, 17, 8.0, None, True):
        with pytest.raises(ValueError, match="bins"):
            dfx.flow_hist_slots("hof", bad)


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
    for bad in ((), "hog", ("hof", "hog"), ("mbhx", "mbhx"), 7, None):
        with pytest.raises(ValueError, match="kinds"):
            call(kinds=bad)
    for bad in (0, 2, 12, 64, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="cell"):
            call(cell=bad)
    for bad in (1, 17, 0, 8.0, "8", None, True):
        with pytest.raises(ValueError, match="bins"):
            call(bins=bad)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, None, "0.4", True):
        with pytest.raises(ValueError, match="still_thr"):
            call(still_thr=bad)
    for bad in ("L2", "l2_hys", 0, None):
        with pytest.raises(ValueError, match="norm"):
            call(norm=bad)


def test_flow_hist_refuses_bad_arguments_before_the_library(dfx):
    eng = _bare_engine(dfx)
    flows = np.zeros((5, 2, 4, 8), np.float32)
    _refused_settings(lambda **kw: eng.flow_hist(flows, **kw))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist(flows.astype(np.float64))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist(flows[:, :, :3])
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist(np.zeros((5, 4, 8, 2), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_hist(flows, mask=np.zeros((5, 4, 8), np.float32))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_hist(flows, mask=np.zeros((4, 4, 8), np.uint8))
    # nothing to do never reaches the library either
    out, sums = eng.flow_hist(flows[:0], want_sums=True)
    assert out.shape == (0, 25, 1, 1) and out.dtype == np.float32 and sums.shape == (0, 1, 1, 25) and sums.dtype == np.int64
    assert eng.flow_hist(flows[:0], "hof", 4, 16).shape == (0, 17, 1, 2)


def test_flow_hist_tensor_refuses_bad_arguments_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    flows = torch.zeros((5, 2, 4, 8))
    _refused_settings(lambda **kw: eng.flow_hist_tensor(flows, **kw))
    for bad in ("nhwc", 1, None):
        with pytest.raises(ValueError, match="layout"):
            eng.flow_hist_tensor(flows, layout=bad)
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist_tensor(flows.double())
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist_tensor(np.zeros((5, 2, 4, 8), np.float32))
    with pytest.raises(ValueError, match="flows"):
        eng.flow_hist_tensor(torch.zeros((5, 2, 4, 16))[..., ::2])
    with pytest.raises(ValueError, match="mask"):
        eng.flow_hist_tensor(flows, mask=torch.zeros((5, 4, 8)))
    with pytest.raises(ValueError, match="mask"):
        eng.flow_hist_tensor(flows, mask=torch.zeros((5, 4, 16), dtype=torch.uint8)[..., ::2])
    with pytest.raises(ValueError, match="out"):
        eng.flow_hist_tensor(flows, out=torch.zeros((5, 25, 1, 1), dtype=torch.float64))
    with pytest.raises(ValueError, match="out"):
        eng.flow_hist_tensor(flows, out=torch.zeros((5, 1, 1, 25)))  # the shape of layout="hwc"
    with pytest.raises(ValueError, match="out"):
        eng.flow_hist_tensor(flows, layout="hwc", out=torch.zeros((5, 25, 1, 1)))
    # everything right but CPU tensors: still refused before the library
    with pytest.raises(ValueError, match="device"):
        eng.flow_hist_tensor(flows, ("hof", "mbhx"), 4, 9, 0.0, "l2", mask=torch.zeros((5, 4, 8), dtype=torch.uint8),
                             want_sums=True, layout="hwc", out=torch.zeros((5, 1, 2, 19)))
