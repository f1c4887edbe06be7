"""denseflow_amd — MI355X-native dense optical flow behind denseflow's calc_optflows_imp boundary.

This package is a thin ctypes binding of the C ABI in include/dfx.h (implemented by the
hand-written HIP kernels under denseflow_amd/csrc/).  It exists so that tests and bench.py can
drive the exact entry points a denseflow maintainer would bind; the compute path is entirely
inside libdfx.so.  There is no CPU fallback: a missing library or GPU raises.

Tensor consumers: FlowEngine.calc_optflows_planar (numpy) and FlowEngine.flow_tensor (torch tensors in, an
(M, 2, H, W) float32 torch tensor out, optionally bounded to [-1, 1]); torch is imported only inside flow_tensor.
FlowEngine.flow_colour / flow_colour_tensor draw flows as colour images on the Middlebury wheel (colour_wheel()).
FlowEngine.flow_hist / flow_hist_tensor give the HOF / MBHx / MBHy cell histograms of flows (flow_hist_slots()).
FlowEngine.splat / splat_tensor carry images and float payloads forward along a flow (the forward warp; holes marked).
FlowEngine.warp_planes / warp_planes_tensor gather float, half and label planes backward along a flow (any channel count).
"""
from .engine import (  # noqa: F401
    DfxError,
    DfxParams,
    DfxStats,
    FARN_WINDOW_BOX,
    FARN_WINDOW_GAUSSIAN,
    FlowEngine,
    algo_from_name,
    build_library,
    colour_wheel,
    device_count,
    flow_hist_slots,
    library_path,
    load_library,
)

__all__ = [
    "DfxError",
    "DfxParams",
    "DfxStats",
    "FARN_WINDOW_BOX",
    "FARN_WINDOW_GAUSSIAN",
    "FlowEngine",
    "algo_from_name",
    "build_library",
    "colour_wheel",
    "device_count",
    "flow_hist_slots",
    "library_path",
    "load_library",
]
