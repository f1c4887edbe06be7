"""The planar entry points at the binding level (no GPU): include/dfx.h declares them, engine.py binds them with the same
number of arguments, FlowEngine.flow_tensor refuses bad tensors before it reaches the library, and importing the package
does not import torch."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dfx_calc_batch_planar", "dfx_calc_batch_planar_device"]


def _header_arity(name):
    src = open(os.path.join(ROOT, "include", "dfx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"include/dfx.h does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


def _binding_arity(name):
    src = open(os.path.join(ROOT, "denseflow_amd", "engine.py")).read()
    m = re.search(r"L\." + name + r"\.argtypes\s*=\s*\[(.*?)\]\n", src, flags=re.S)
    assert m, f"engine.py does not bind {name}"
    args = re.sub(r"\([^()]*\)", "", m.group(1))  # C.POINTER(vp) -> C.POINTER
    return len([a for a in args.split(",") if a.strip()])


@pytest.mark.parametrize("name,arity", [("dfx_calc_batch_planar", 9), ("dfx_calc_batch_planar_device", 11)])
def test_header_and_binding_agree(name, arity):
    assert _header_arity(name) == arity
    assert _binding_arity(name) == arity


def test_library_exports_and_binds_the_entry_points(dfx):
    L = dfx.load_library()
    for name in ENTRY_POINTS:
        fn = getattr(L, name)
        assert len(fn.argtypes) == _header_arity(name)
    assert hasattr(L, "dfxi_probe_planar_value")  # the device self-check of the stored value (selftest.hip)
    assert callable(dfx.FlowEngine.calc_optflows_planar) and callable(dfx.FlowEngine.flow_tensor)


class _Untouchable:
    """Stands where the loaded library would: any use of it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name})")


def _bare_engine(dfx, w=8, h=4):
    eng = object.__new__(dfx.FlowEngine)  # no handle, no device: everything below must be refused before either is needed
    eng.width, eng.height, eng._device = w, h, 0
    eng._L, eng._h = _Untouchable(), None
    return eng


def test_flow_tensor_refuses_bad_tensors_before_the_library(dfx):
    import torch

    eng = _bare_engine(dfx)
    good = torch.zeros((3, 4, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="device"):
        eng.flow_tensor(good, 1)  # a CPU tensor
    with pytest.raises(ValueError, match="uint8"):
        eng.flow_tensor(good.float(), 1)
    with pytest.raises(ValueError, match=r"\(N,\)"):
        eng.flow_tensor(good[0], 1)  # rank
    with pytest.raises(ValueError, match=r"\(N,\)"):
        eng.flow_tensor(torch.zeros((3, 8, 4), dtype=torch.uint8), 1)  # shape
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_tensor(torch.zeros((3, 8, 4), dtype=torch.uint8).transpose(1, 2), 1)
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_tensor(torch.zeros((3, 4, 16), dtype=torch.uint8)[:, :, ::2], 1)
    with pytest.raises(ValueError, match="shape"):
        eng.flow_tensor(good, 1, out=torch.zeros((2, 2, 4, 9)))
    with pytest.raises(ValueError, match="shape"):
        eng.flow_tensor(good, 1, out=torch.zeros((3, 2, 4, 8)))  # three frames give two flows
    with pytest.raises(ValueError, match="float32"):
        eng.flow_tensor(good, 1, out=torch.zeros((2, 2, 4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match="out:"):
        eng.flow_tensor(good, 1, out=torch.zeros((2, 2, 8, 4)).transpose(2, 3))
    with pytest.raises(ValueError, match="out:"):
        eng.flow_tensor(good, 1, out=torch.zeros((2, 2, 4, 1)).expand(2, 2, 4, 8))  # rows on top of each other
    with pytest.raises(ValueError):
        eng.flow_tensor([[0]], 1)  # not a tensor at all
    eng._src = (6, 10, 3)  # as set_source_format(10, 6, 3) leaves it: BGR frames
    with pytest.raises(ValueError, match=r"\(N,\)"):
        eng.flow_tensor(good, 1)
    with pytest.raises(ValueError, match="innermost"):
        eng.flow_tensor(torch.zeros((3, 6, 10, 6), dtype=torch.uint8)[..., ::2], 1)


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import denseflow_amd; import denseflow_amd.engine; sys.exit(1 if 'torch' in sys.modules else 0)"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, "import denseflow_amd pulled torch in\n" + r.stderr
