"""Typed planar output and source layouts at the binding level (no GPU): include/dfx.h declares the new entry points at
DFX_VERSION >= 430, libdfx.so exports them, engine.py binds them with the same number of arguments, and the argument checks
of the binding fire before the library is reached."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {
    "dfx_calc_batch_planar_as": 10,
    "dfx_calc_batch_planar_as_device": 12,
    "dfx_calc_batch_planar_as_init_device": 16,
    "dfx_set_source_format_ex": 7,
    "dfx_prepare_frames_layout": 11,
    "dfx_prepare_frames_layout_device": 14,
}


def _header():
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_arity(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"include/dfx.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


def _binding_arity(name):
    src = open(os.path.join(ROOT, "denseflow_amd", "engine.py")).read()
    m = re.search(r"L\." + name + r"\.argtypes\s*=\s*\[(.*?)\]\n", src, flags=re.S)
    assert m, f"engine.py does not bind {name}"
    args = re.sub(r"\([^()]*\)", "", m.group(1))  # C.POINTER(vp) -> C.POINTER
    return len([a for a in args.split(",") if a.strip()])


def test_the_header_declares_the_constants_at_version_430():
    src = _header()
    assert int(re.search(r"#define\s+DFX_VERSION\s+(\d+)", src).group(1)) >= 430
    want = {"DFX_PLANAR_F32": 0, "DFX_PLANAR_F16": 1, "DFX_PLANAR_BF16": 2, "DFX_SRC_BGR": 0, "DFX_SRC_RGB": 1,
            "DFX_SRC_INTERLEAVED": 0, "DFX_SRC_PLANAR": 1}
    for name, value in want.items():
        m = re.search(r"#define\s+" + name + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == value, name


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_header_and_binding_agree(name):
    assert _header_arity(name) == ENTRY_POINTS[name]
    assert _binding_arity(name) == ENTRY_POINTS[name]


def test_library_exports_and_binds_the_entry_points(dfx):
    from denseflow_amd import engine as E

    L = dfx.load_library()
    for name, arity in ENTRY_POINTS.items():
        assert len(getattr(L, name).argtypes) == arity, name
    assert hasattr(L, "dfxi_probe_planar_value_as")  # the device self-check of the stored bits (selftest.hip)
    assert (E.PLANAR_F32, E.PLANAR_F16, E.PLANAR_BF16) == (0, 1, 2)
    assert E.SRC_ORDERS == {"bgr": 0, "rgb": 1} and E.SRC_LAYOUTS == {"hwc": 0, "chw": 1}


class _Untouchable:
    """Stands where the loaded library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_engine(dfx, w=8, h=4):
    eng = object.__new__(dfx.FlowEngine)  # no handle, no device: everything below must be refused before either is needed
    eng.width, eng.height, eng._device = w, h, 0
    eng._L, eng._h = _Untouchable(), None
    return eng


def test_flow_tensor_refuses_bad_dtypes_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    good = torch.zeros((3, 4, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="dtype"):
        eng.flow_tensor(good, 1, dtype=torch.float64)  # an unknown dtype
    with pytest.raises(ValueError, match="dtype"):
        eng.flow_tensor(good, 1, dtype=np.float16)  # numpy's, not torch's
    with pytest.raises(ValueError, match="float16"):
        eng.flow_tensor(good, 1, dtype=torch.float16, out=torch.zeros((2, 2, 4, 8)))  # a float32 out for half planes
    with pytest.raises(ValueError, match="bfloat16"):
        eng.flow_tensor(good, 1, dtype=torch.bfloat16, out=torch.zeros((2, 2, 4, 8), dtype=torch.float16))
    with pytest.raises(ValueError, match="float32"):
        eng.flow_tensor(good, 1, out=torch.zeros((2, 2, 4, 8), dtype=torch.float16))  # the default stays float32
    with pytest.raises(ValueError, match="shape"):
        eng.flow_tensor(good, 1, dtype=torch.float16, out=torch.zeros((2, 2, 4, 9), dtype=torch.float16))
    with pytest.raises(ValueError, match="out:"):
        eng.flow_tensor(good, 1, dtype=torch.float16, out=torch.zeros((2, 2, 8, 4), dtype=torch.float16).transpose(2, 3))
    with pytest.raises(ValueError, match="device"):
        eng.flow_tensor(good, 1, dtype=torch.float16)  # everything right but a CPU tensor: still before the library


def test_numpy_forms_refuse_unknown_dtypes_before_the_library(dfx):
    eng = _bare_engine(dfx)
    frames = [np.zeros((4, 8), np.uint8)] * 3
    for bad in (np.float64, "half", "bf16", np.int16, object()):
        with pytest.raises(ValueError, match="dtype"):
            eng.calc_optflows_planar(frames, 1, dtype=bad)
        with pytest.raises(ValueError, match="dtype"):
            eng.calc_optflows_planar_device(0, 8, 32, 3, 1, None, 0, 8, 32, 64, dtype=bad)


def test_source_format_refuses_unknown_orders_and_layouts_before_the_library(dfx):
    eng = _bare_engine(dfx)
    with pytest.raises(ValueError, match="order"):
        eng.set_source_format(10, 6, 3, order="gbr")
    with pytest.raises(ValueError, match="layout"):
        eng.set_source_format(10, 6, 3, layout="nchw")
    with pytest.raises(ValueError, match="3-channel"):
        eng.set_source_format(10, 6, 1, order="rgb")
    with pytest.raises(ValueError, match="3-channel"):
        eng.set_source_format(10, 6, 1, layout="chw")
    rgb = [np.zeros((6, 10, 3), np.uint8)]
    with pytest.raises(ValueError, match="order"):
        eng.prepare_frames(rgb, order="gbr")
    with pytest.raises(ValueError, match="layout"):
        eng.prepare_frames(rgb, layout="nchw")
    with pytest.raises(ValueError, match=r"\(3, h, w\)"):
        eng.prepare_frames(rgb, layout="chw")  # interleaved frames declared channels-first
    with pytest.raises(ValueError, match="3-channel"):
        eng.prepare_frames([np.zeros((6, 10), np.uint8)], order="rgb")


def test_flow_tensor_checks_channels_first_strides_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    eng._src, eng._src_chw, eng._src_fmt = (3, 6, 10), True, (10, 6, 3, 1, 1)  # as set_source_format(10, 6, 3, "rgb", "chw") leaves it
    with pytest.raises(ValueError, match=r"\(N,\)"):
        eng.flow_tensor(torch.zeros((3, 6, 10, 3), dtype=torch.uint8), 1)  # an interleaved shape
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_tensor(torch.zeros((3, 3, 6, 20), dtype=torch.uint8)[..., ::2], 1)
    with pytest.raises(ValueError, match="overlap"):  # the planes' rows interleave: plane stride 10 < a plane
        eng.flow_tensor(torch.zeros((3, 6, 3, 10), dtype=torch.uint8).permute(0, 2, 1, 3), 1)
    with pytest.raises(ValueError, match="overlap"):  # one plane shown three times
        eng.flow_tensor(torch.zeros((3, 1, 6, 10), dtype=torch.uint8).expand(3, 3, 6, 10), 1)
    with pytest.raises(ValueError, match="overlap"):  # frames on top of each other
        eng.flow_tensor(torch.zeros((1, 3, 6, 10), dtype=torch.uint8).expand(3, 3, 6, 10), 1)
    with pytest.raises(ValueError, match="device"):  # dense planes, and the permuted view of an NHWC batch: accepted so far
        eng.flow_tensor(torch.zeros((3, 3, 6, 10), dtype=torch.uint8), 1)
    with pytest.raises(ValueError, match="device"):
        eng.flow_tensor(torch.zeros((3, 6, 10, 3), dtype=torch.uint8).permute(0, 3, 1, 2), 1)
