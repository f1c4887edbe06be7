"""ctypes binding of include/dfx.h.

Mirrors the reference operator interface for the hot path: `FlowEngine.calc_optflows` takes the
gray frames of one FlowBuffer and a step and returns the list of CV_32FC2-shaped flows exactly as
DenseFlow::calc_optflows_imp does (/root/reference is not needed at run time; the behaviour is the
one at src/denseflow_gpu.cpp:307-342).  Errors carry the reference's message texts.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_LIB_DIR = os.path.join(_HERE, "lib")
_LIB = os.path.join(_LIB_DIR, "libdfx.so")
_CSRC = os.path.join(_HERE, "csrc")

DFX_MAX_LEVELS = 32
DFX_MAX_WARPS = 16

ALGO_TVL1, ALGO_FARN, ALGO_BROX, ALGO_FRAMES = 0, 1, 2, 3
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED, ERR_NV_DISABLED, ERR_UNKNOWN_ALGO = range(7)


class DfxError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


class DfxParams(C.Structure):
    _fields_ = [
        ("tvl1_tau", C.c_double),
        ("tvl1_lambda", C.c_double),
        ("tvl1_theta", C.c_double),
        ("tvl1_nscales", C.c_int),
        ("tvl1_warps", C.c_int),
        ("tvl1_epsilon", C.c_double),
        ("tvl1_iterations", C.c_int),
        ("tvl1_scale_step", C.c_double),
        ("farn_num_levels", C.c_int),
        ("farn_pyr_scale", C.c_double),
        ("farn_win_size", C.c_int),
        ("farn_num_iters", C.c_int),
        ("farn_poly_n", C.c_int),
        ("farn_poly_sigma", C.c_double),
        ("farn_flags", C.c_int),
        ("farn_window", C.c_int),
        ("brox_alpha", C.c_float),
        ("brox_gamma", C.c_float),
        ("brox_scale_factor", C.c_float),
        ("brox_inner_iterations", C.c_int),
        ("brox_outer_iterations", C.c_int),
        ("brox_solver_iterations", C.c_int),
        ("max_batch", C.c_int),
        ("impl", C.c_int),
        ("tvl1_fuse_k", C.c_int),
        ("tvl1_math", C.c_int),
        ("variant", C.c_int),
        ("step_group", C.c_int),
        ("blocking_sync", C.c_int),
        ("tvl1_gamma", C.c_double),
        ("farn_fast_pyramids", C.c_int),  # last: a library built before it (DFX_LIBRARY A/B) reads the fields it knows
    ]


# dfx_params.farn_window (include/dfx.h): FlowEngine(..., "farn", farn_window=FARN_WINDOW_GAUSSIAN) is how upstream's
# OPTFLOW_FARNEBACK_GAUSSIAN is requested; farn_flags stays refused unless 0
FARN_WINDOW_BOX, FARN_WINDOW_GAUSSIAN = 0, 1
# dfx_params.farn_fast_pyramids: FlowEngine(..., "farn", farn_fast_pyramids=1) is upstream's fastPyramids (pyrDown frame pyramids,
# pyrUp flows); it needs farn_pyr_scale = 0.5 and even level sizes below the coarsest level (DfxError otherwise)

# dfx_params.variant bits (include/dfx.h): cross-check / measurement forms of the tuned kernels, all bit-identical
VAR_TVL1_CLASSIC_GEOM, VAR_TVL1_WARP_IN_STEP = 0x01, 0x02
VAR_FARN_EVAL_ZERO_TAPS, VAR_FARN_POLY_ONE_ROW, VAR_FARN_M_IN_HBM = 0x04, 0x08, 0x10
VAR_TVL1_WARP_GATHER = 0x20
VAR_TVL1_NO_HEAD = 0x40
VAR_BROX_SOR_PROGRESS = 0x80
VAR_BROX_SOR_PER_TILE = 0x100
VAR_TVL1_STEP_NBR_LDS = 0x200  # TVL1 step kernel in its register form (3 waves per SIMD), not the lean one (4)
VAR_TVL1_HEAD_NBR_LDS = 0x400  # TVL1 warp-and-head kernel in its register form (3 waves per SIMD), not the lean one (4)


class DfxStats(C.Structure):
    _fields_ = [
        ("pairs", C.c_uint64),
        ("batch", C.c_int),
        ("kernel_launches", C.c_uint64),
        ("noop_steps", C.c_uint64),
        ("device_ms", C.c_double),
        ("step_ms", C.c_double),
        ("step_launches", C.c_uint64),
        ("level_ms", C.c_double * DFX_MAX_LEVELS),
        ("level_launches", C.c_uint64 * DFX_MAX_LEVELS),
        ("algorithmic_bytes", C.c_double),
        ("step_algorithmic_bytes", C.c_double),
        ("levels", C.c_int),
        ("level_w", C.c_int * DFX_MAX_LEVELS),
        ("level_h", C.c_int * DFX_MAX_LEVELS),
        ("tvl1_iters", (C.c_int * DFX_MAX_WARPS) * DFX_MAX_LEVELS),
        ("tvl1_checks", C.c_int),
        ("tvl1_total_iters", C.c_uint64),
        ("tvl1_px_iters", C.c_double),
        ("tvl1_lane_iters", C.c_double),
    ]

    def iters_table(self):
        return [[self.tvl1_iters[s][w] for w in range(DFX_MAX_WARPS)] for s in range(self.levels)]


class DfxWarpDesc(C.Structure):
    """dfx_warp_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_src", C.c_void_p),
        ("channels", C.c_int),
        ("layout", C.c_int),
        ("src_pitch", C.c_size_t),
        ("src_plane_stride", C.c_size_t),
        ("src_image_stride", C.c_size_t),
        ("d_ref", C.c_void_p),
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("border", C.c_int),
        ("out_dtype", C.c_int),
        ("d_out", C.c_void_p),
        ("out_pitch", C.c_size_t),
        ("out_plane_stride", C.c_size_t),
        ("out_image_stride", C.c_size_t),
        ("d_occ", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("d_valid", C.c_void_p),
        ("valid_pitch", C.c_size_t),
        ("valid_stride", C.c_size_t),
        ("d_stats", C.c_void_p),
    ]


class DfxGmResult(C.Structure):
    """dfx_gm_result of include/dfx.h, field for field: one record per flow, the results and the call's only workspace."""
    _fields_ = [
        ("a", C.c_double * 6),
        ("p", C.c_float * 6),
        ("valid", C.c_uint64),
        ("inliers", C.c_uint64 * 8),
        ("status", C.c_uint32),
        ("rounds", C.c_uint32),
        ("sums", C.c_int64 * 12),
        ("work", C.c_uint64 * 13),
    ]


class DfxGmDesc(C.Structure):
    """dfx_gm_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("model", C.c_int),
        ("rounds", C.c_int),
        ("thr", C.c_float),
        ("growth", C.c_float),
        ("d_mask", C.c_void_p),
        ("mask_pitch", C.c_size_t),
        ("mask_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_row_pitch_floats", C.c_size_t),
        ("out_plane_stride_floats", C.c_size_t),
        ("out_flow_stride_floats", C.c_size_t),
        ("d_moving", C.c_void_p),
        ("moving_pitch", C.c_size_t),
        ("moving_stride", C.c_size_t),
        ("d_result", C.c_void_p),
    ]


GM_RESULT_DTYPE = np.dtype([("a", "<f8", 6), ("p", "<f4", 6), ("valid", "<u8"), ("inliers", "<u8", 8), ("status", "<u4"),
                            ("rounds", "<u4"), ("sums", "<i8", 12), ("work", "<u8", 13)])  # dfx_gm_result as a NumPy record


class DfxMedianDesc(C.Structure):
    """dfx_median_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("ksize", C.c_int),
        ("mode", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_pitch", C.c_size_t),
        ("mask_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_row_pitch_floats", C.c_size_t),
        ("out_plane_stride_floats", C.c_size_t),
        ("out_flow_stride_floats", C.c_size_t),
        ("d_mask_out", C.c_void_p),
        ("mask_out_pitch", C.c_size_t),
        ("mask_out_stride", C.c_size_t),
    ]


class DfxChainDesc(C.Structure):
    """dfx_chain_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("first", C.c_int),
        ("hop", C.c_int),
        ("length", C.c_int),
        ("anchors", C.c_int),
        ("anchor_step", C.c_int),
        ("emit", C.c_int),
        ("border", C.c_int),
        ("d_occ", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_row_pitch_floats", C.c_size_t),
        ("out_plane_stride_floats", C.c_size_t),
        ("out_flow_stride_floats", C.c_size_t),
        ("d_valid", C.c_void_p),
        ("valid_pitch", C.c_size_t),
        ("valid_stride", C.c_size_t),
    ]


class DfxProjectDesc(C.Structure):
    """dfx_project_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("t", C.c_float),
        ("scale", C.c_float),
        ("min_weight", C.c_float),
        ("d_importance", C.c_void_p),
        ("importance_pitch_floats", C.c_size_t),
        ("importance_stride_floats", C.c_size_t),
        ("d_occ", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_row_pitch_floats", C.c_size_t),
        ("out_plane_stride_floats", C.c_size_t),
        ("out_flow_stride_floats", C.c_size_t),
        ("d_hole", C.c_void_p),
        ("hole_pitch", C.c_size_t),
        ("hole_stride", C.c_size_t),
        ("d_coverage", C.c_void_p),
        ("coverage_pitch_floats", C.c_size_t),
        ("coverage_stride_floats", C.c_size_t),
        ("d_work", C.c_void_p),
        ("work_bytes", C.c_size_t),
    ]


class DfxSplatDesc(C.Structure):
    """dfx_splat_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_src", C.c_void_p),
        ("src_dtype", C.c_int),
        ("channels", C.c_int),
        ("layout", C.c_int),
        ("src_pitch", C.c_size_t),
        ("src_plane_stride", C.c_size_t),
        ("src_image_stride", C.c_size_t),
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("t", C.c_float),
        ("min_weight", C.c_float),
        ("mode", C.c_int),
        ("hole_mode", C.c_int),
        ("out_dtype", C.c_int),
        ("d_importance", C.c_void_p),
        ("importance_pitch_floats", C.c_size_t),
        ("importance_stride_floats", C.c_size_t),
        ("d_occ", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_pitch", C.c_size_t),
        ("out_plane_stride", C.c_size_t),
        ("out_image_stride", C.c_size_t),
        ("d_hole", C.c_void_p),
        ("hole_pitch", C.c_size_t),
        ("hole_stride", C.c_size_t),
        ("d_coverage", C.c_void_p),
        ("coverage_pitch_floats", C.c_size_t),
        ("coverage_stride_floats", C.c_size_t),
        ("d_work", C.c_void_p),
        ("work_bytes", C.c_size_t),
    ]


class DfxWarpPlanesDesc(C.Structure):
    """dfx_warp_planes_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_src", C.c_void_p),
        ("src_dtype", C.c_int),
        ("channels", C.c_int),
        ("layout", C.c_int),
        ("src_pitch", C.c_size_t),
        ("src_plane_stride", C.c_size_t),
        ("src_image_stride", C.c_size_t),
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("border", C.c_int),
        ("sample", C.c_int),
        ("invalid", C.c_int),
        ("out_dtype", C.c_int),
        ("d_out", C.c_void_p),
        ("out_pitch", C.c_size_t),
        ("out_plane_stride", C.c_size_t),
        ("out_image_stride", C.c_size_t),
        ("d_occ", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("d_valid", C.c_void_p),
        ("valid_pitch", C.c_size_t),
        ("valid_stride", C.c_size_t),
    ]


class DfxInterpDesc(C.Structure):
    """dfx_interp_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_img0", C.c_void_p),
        ("d_img1", C.c_void_p),
        ("channels", C.c_int),
        ("layout", C.c_int),
        ("img_pitch", C.c_size_t),
        ("img_plane_stride", C.c_size_t),
        ("img_image_stride", C.c_size_t),
        ("d_fwd", C.c_void_p),
        ("d_bwd", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("t", C.c_float),
        ("min_weight", C.c_float),
        ("fill_passes", C.c_int),
        ("ksize", C.c_int),
        ("d_occ_fwd", C.c_void_p),
        ("d_occ_bwd", C.c_void_p),
        ("occ_pitch", C.c_size_t),
        ("occ_stride", C.c_size_t),
        ("out_dtype", C.c_int),
        ("d_out", C.c_void_p),
        ("out_pitch", C.c_size_t),
        ("out_plane_stride", C.c_size_t),
        ("out_image_stride", C.c_size_t),
        ("d_source", C.c_void_p),
        ("source_pitch", C.c_size_t),
        ("source_stride", C.c_size_t),
        ("d_work", C.c_void_p),
        ("work_bytes", C.c_size_t),
    ]


class DfxColourDesc(C.Structure):
    """dfx_colour_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_pitch", C.c_size_t),
        ("mask_stride", C.c_size_t),
        ("norm", C.c_int),
        ("max_rad", C.c_float),
        ("d_max2", C.c_void_p),
        ("order", C.c_int),
        ("layout", C.c_int),
        ("d_out", C.c_void_p),
        ("out_pitch", C.c_size_t),
        ("out_plane_stride", C.c_size_t),
        ("out_image_stride", C.c_size_t),
        ("unknown", C.c_uint8 * 3),
        ("d_frame", C.c_void_p),
        ("frame_channels", C.c_int),
        ("frame_layout", C.c_int),
        ("frame_pitch", C.c_size_t),
        ("frame_plane_stride", C.c_size_t),
        ("frame_image_stride", C.c_size_t),
        ("alpha256", C.c_int),
    ]


class DfxHistDesc(C.Structure):
    """dfx_hist_desc of include/dfx.h, field for field."""
    _fields_ = [
        ("d_flow", C.c_void_p),
        ("row_pitch_floats", C.c_size_t),
        ("plane_stride_floats", C.c_size_t),
        ("flow_stride_floats", C.c_size_t),
        ("n", C.c_int),
        ("d_mask", C.c_void_p),
        ("mask_pitch", C.c_size_t),
        ("mask_stride", C.c_size_t),
        ("kinds", C.c_int),
        ("cell", C.c_int),
        ("bins", C.c_int),
        ("still_thr", C.c_float),
        ("norm", C.c_int),
        ("d_sums", C.c_void_p),
        ("sums_stride", C.c_size_t),
        ("d_out", C.c_void_p),
        ("out_slot_stride_floats", C.c_size_t),
        ("out_col_stride_floats", C.c_size_t),
        ("out_row_stride_floats", C.c_size_t),
        ("out_flow_stride_floats", C.c_size_t),
    ]


# ------------------------------------------------------------------------------------------ build

def library_path() -> str:
    return _LIB


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into denseflow_amd/lib/libdfx.so (cross-compiles without a GPU)."""
    srcs = sorted(
        os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".hip") or f.endswith(".cpp")
    )
    inc = os.path.join(_ROOT, "include")
    deps = srcs + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")] + [
        os.path.join(inc, f) for f in os.listdir(inc) if f.startswith("dfx") and f.endswith(".h")
    ]
    if not force and os.path.exists(_LIB) and all(os.path.getmtime(_LIB) >= os.path.getmtime(d) for d in deps):
        return _LIB
    os.makedirs(_LIB_DIR, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [
        hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
        "-I" + os.path.join(_ROOT, "include"), "-o", _LIB,
    ] + srcs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stdout + r.stderr)
    return _LIB


_lib = None


def load_library():
    """dlopen libdfx.so.  torch (if present) is imported first so both share one HIP runtime."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise DfxError(ERR_NO_DEVICE, f"{_LIB} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # torch bundles its own libamdhip64.so (HIP 7.0 in torch 2.10+rocm7.0); importing it first makes the loader reuse that
    # copy, which a process that also holds torch tensors needs (one runtime per process).  A torch-free process
    # (DFX_NO_TORCH=1: binding-level switch, the library itself reads no environment) gets the system runtime libdfx.so
    # was linked against (/opt/rocm, HIP 7.2) — what a C++ caller such as build/denseflow runs on.  The two runtimes differ
    # in how they execute device-to-host copies (shader blit vs SDMA: DESIGN.md section 5).
    if os.environ.get("DFX_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the library itself
            pass
    L = C.CDLL(os.environ.get("DFX_LIBRARY", _LIB))  # DFX_LIBRARY: A/B a differently built libdfx.so
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.dfx_device_count.restype = i
    L.dfx_default_params.argtypes = [C.POINTER(DfxParams)]
    L.dfx_algo_from_name.argtypes = [C.c_char_p, C.POINTER(i)]
    L.dfx_algo_from_name.restype = i
    L.dfx_algo_error_message.argtypes = [i, C.c_char_p, C.c_char_p, sz]
    L.dfx_algo_error_message.restype = C.c_char_p
    L.dfx_create.argtypes = [C.POINTER(vp), i, i, i, i, C.POINTER(DfxParams)]
    L.dfx_create.restype = i
    L.dfx_calc.argtypes = [vp, vp, sz, vp, sz, vp, sz]
    L.dfx_calc.restype = i
    L.dfx_calc_batch.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), sz]
    L.dfx_calc_batch.restype = i
    L.dfx_calc_batch_device.argtypes = [vp, vp, sz, sz, i, i, vp, sz]
    L.dfx_calc_batch_device.restype = i
    if hasattr(L, "dfx_calc_batch_planar"):  # a library built before the planar output (DFX_LIBRARY A/B) still loads
        L.dfx_calc_batch_planar.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, C.POINTER(vp), C.POINTER(vp), sz]
        L.dfx_calc_batch_planar.restype = i
        L.dfx_calc_batch_planar_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, vp, sz, sz, sz]
        L.dfx_calc_batch_planar_device.restype = i
    if hasattr(L, "dfx_calc_batch_planar_as"):  # a library built before the typed planes / source layouts still loads
        L.dfx_calc_batch_planar_as.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, i, C.POINTER(vp), C.POINTER(vp), sz]
        L.dfx_calc_batch_planar_as.restype = i
        L.dfx_calc_batch_planar_as_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, i, vp, sz, sz, sz]
        L.dfx_calc_batch_planar_as_device.restype = i
        L.dfx_calc_batch_planar_as_init_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, i, vp, sz, sz, sz, vp, sz, sz, sz]
        L.dfx_calc_batch_planar_as_init_device.restype = i
        L.dfx_set_source_format_ex.argtypes = [vp, i, i, i, i, i, sz]
        L.dfx_set_source_format_ex.restype = i
        L.dfx_prepare_frames_layout.argtypes = [vp, C.POINTER(vp), sz, i, i, i, i, i, i, C.POINTER(vp), sz]
        L.dfx_prepare_frames_layout.restype = i
        L.dfx_prepare_frames_layout_device.argtypes = [vp, vp, sz, sz, sz, i, i, i, i, i, i, vp, sz, sz]
        L.dfx_prepare_frames_layout_device.restype = i
    if hasattr(L, "dfx_calc_batch_bidir_device"):  # a library built before the bidirectional call (DFX_LIBRARY A/B) still loads
        f32 = C.c_float
        L.dfx_calc_batch_bidir_device.argtypes = [vp, vp, sz, sz, i, i, vp, vp, sz, sz, sz, f32, f32, vp, vp, sz, sz]
        L.dfx_calc_batch_bidir_device.restype = i
        L.dfx_fb_check_device.argtypes = [vp, vp, vp, sz, sz, sz, i, f32, f32, vp, sz, sz, vp, sz, sz]
        L.dfx_fb_check_device.restype = i
    if hasattr(L, "dfx_warp_device"):  # a library built before the warp (DFX_LIBRARY A/B) still loads
        L.dfx_warp_device.argtypes = [vp, C.POINTER(DfxWarpDesc)]
        L.dfx_warp_device.restype = i
    if hasattr(L, "dfx_global_motion_device"):  # a library built before the global motion (DFX_LIBRARY A/B) still loads
        L.dfx_global_motion_device.argtypes = [vp, C.POINTER(DfxGmDesc)]
        L.dfx_global_motion_device.restype = i
    if hasattr(L, "dfx_flow_median_device"):  # a library built before the flow median (DFX_LIBRARY A/B) still loads
        L.dfx_flow_median_device.argtypes = [vp, C.POINTER(DfxMedianDesc)]
        L.dfx_flow_median_device.restype = i
    if hasattr(L, "dfx_flow_chain_device"):  # a library built before the flow chain (DFX_LIBRARY A/B) still loads
        L.dfx_flow_chain_device.argtypes = [vp, C.POINTER(DfxChainDesc)]
        L.dfx_flow_chain_device.restype = i
    if hasattr(L, "dfx_flow_project_device"):  # a library built before the flow projection (DFX_LIBRARY A/B) still loads
        L.dfx_flow_project_device.argtypes = [vp, C.POINTER(DfxProjectDesc)]
        L.dfx_flow_project_device.restype = i
        L.dfx_flow_project_work_bytes.argtypes = [vp]
        L.dfx_flow_project_work_bytes.restype = sz
    if hasattr(L, "dfx_interpolate_device"):  # a library built before the frame interpolation (DFX_LIBRARY A/B) still loads
        L.dfx_interpolate_device.argtypes = [vp, C.POINTER(DfxInterpDesc)]
        L.dfx_interpolate_device.restype = i
        L.dfx_interpolate_work_bytes.argtypes = [vp, C.POINTER(DfxInterpDesc)]
        L.dfx_interpolate_work_bytes.restype = sz
    if hasattr(L, "dfx_flow_colour_device"):  # a library built before the colour coding (DFX_LIBRARY A/B) still loads
        L.dfx_flow_colour_device.argtypes = [vp, C.POINTER(DfxColourDesc)]
        L.dfx_flow_colour_device.restype = i
    if hasattr(L, "dfx_flow_hist_device"):  # a library built before the motion descriptors (DFX_LIBRARY A/B) still loads
        L.dfx_flow_hist_device.argtypes = [vp, C.POINTER(DfxHistDesc)]
        L.dfx_flow_hist_device.restype = i
    if hasattr(L, "dfx_warp_planes_device"):  # a library built before the warp of planes (DFX_LIBRARY A/B) still loads
        L.dfx_warp_planes_device.argtypes = [vp, C.POINTER(DfxWarpPlanesDesc)]
        L.dfx_warp_planes_device.restype = i
    if hasattr(L, "dfx_splat_device"):  # a library built before the forward warp (DFX_LIBRARY A/B) still loads
        L.dfx_splat_device.argtypes = [vp, C.POINTER(DfxSplatDesc)]
        L.dfx_splat_device.restype = i
        L.dfx_splat_work_bytes.argtypes = [vp, i]
        L.dfx_splat_work_bytes.restype = sz
    if hasattr(L, "dfxi_probe_planar_value_as"):  # test hook (selftest.hip)
        L.dfxi_probe_planar_value_as.argtypes = [i, i, vp, C.c_float, vp, sz]
        L.dfxi_probe_planar_value_as.restype = i
    if hasattr(L, "dfx_calc_batch_init"):  # a library built before the initial flows (DFX_LIBRARY A/B) still loads
        L.dfx_calc_batch_init.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), sz, C.POINTER(vp), sz]
        L.dfx_calc_batch_init.restype = i
        L.dfx_calc_batch_init_device.argtypes = [vp, vp, sz, sz, i, i, vp, sz, vp, sz]
        L.dfx_calc_batch_init_device.restype = i
        L.dfx_calc_batch_planar_init_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, vp, vp, sz, sz, sz]
        L.dfx_calc_batch_planar_init_device.restype = i
    L.dfx_calc_batch_u8.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, C.c_double, C.POINTER(vp), C.POINTER(vp), sz]
    L.dfx_calc_batch_u8.restype = i
    L.dfx_submit_batch.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), sz, C.POINTER(C.c_uint64)]
    L.dfx_submit_batch.restype = i
    L.dfx_submit_batch_u8.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, C.c_double, C.POINTER(vp), C.POINTER(vp),
                                      sz, C.POINTER(C.c_uint64)]
    L.dfx_submit_batch_u8.restype = i
    u32p = C.POINTER(C.c_uint32)
    L.dfx_calc_batch_jpeg.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, C.c_double, i, C.POINTER(vp),
                                      C.POINTER(vp), sz, u32p, u32p]
    L.dfx_calc_batch_jpeg.restype = i
    L.dfx_submit_batch_jpeg.argtypes = [vp, C.POINTER(vp), sz, i, i, C.c_double, C.c_double, i, C.POINTER(vp),
                                        C.POINTER(vp), sz, u32p, u32p, C.POINTER(C.c_uint64)]
    L.dfx_submit_batch_jpeg.restype = i
    L.dfx_encode_jpeg.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), sz, u32p]
    L.dfx_encode_jpeg.restype = i
    L.dfx_jpeg_capacity.argtypes = [vp]
    L.dfx_jpeg_capacity.restype = sz
    L.dfx_next_segments.argtypes = [vp, C.POINTER(C.c_int), i]
    L.dfx_next_segments.restype = i
    L.dfx_next_segments_src.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(sz), i, i]
    L.dfx_next_segments_src.restype = i
    L.dfx_wait.argtypes = [vp, C.c_uint64]
    L.dfx_wait.restype = i
    L.dfx_calc_batch_u8_device.argtypes = [vp, vp, sz, sz, i, i, C.c_double, C.c_double, vp, vp, sz, sz]
    L.dfx_calc_batch_u8_device.restype = i
    dp = C.POINTER(C.c_double)
    L.dfx_calc_batch_png.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), C.POINTER(vp), sz, dp]
    L.dfx_calc_batch_png.restype = i
    L.dfx_submit_batch_png.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), C.POINTER(vp), sz, dp, C.POINTER(C.c_uint64)]
    L.dfx_submit_batch_png.restype = i
    L.dfx_calc_batch_png_device.argtypes = [vp, vp, sz, sz, i, i, vp, vp, sz, sz, vp]
    L.dfx_calc_batch_png_device.restype = i
    L.dfx_flow_to_png_device.argtypes = [vp, vp, sz, i, vp, vp, sz, sz, vp]
    L.dfx_flow_to_png_device.restype = i
    L.dfx_flow_to_u8_device.argtypes = [vp, vp, sz, i, C.c_double, C.c_double, vp, vp, sz, sz]
    L.dfx_flow_to_u8_device.restype = i
    L.dfx_set_source_format.argtypes = [vp, i, i, i]
    L.dfx_set_source_format.restype = i
    L.dfx_prepare_frames.argtypes = [vp, C.POINTER(vp), sz, i, i, i, i, C.POINTER(vp), sz]
    L.dfx_prepare_frames.restype = i
    L.dfx_prepare_frames_device.argtypes = [vp, vp, sz, sz, i, i, i, i, vp, sz, sz]
    L.dfx_prepare_frames_device.restype = i
    L.dfx_prepare_frames_bgr.argtypes = [vp, C.POINTER(vp), sz, i, i, i, C.POINTER(vp), sz]
    L.dfx_prepare_frames_bgr.restype = i
    L.dfx_prepare_frames_bgr_device.argtypes = [vp, vp, sz, sz, i, i, i, vp, sz, sz]
    L.dfx_prepare_frames_bgr_device.restype = i
    L.dfx_encode_jpeg_bgr.argtypes = [vp, C.POINTER(vp), sz, i, i, C.POINTER(vp), sz, u32p]
    L.dfx_encode_jpeg_bgr.restype = i
    L.dfx_jpeg_capacity_bgr.argtypes = [vp]
    L.dfx_jpeg_capacity_bgr.restype = sz
    L.dfx_extract_frames.argtypes = [vp, C.POINTER(vp), sz, i, i, i, i, C.POINTER(vp), sz, u32p]
    L.dfx_extract_frames.restype = i
    L.dfx_submit_extract_frames.argtypes = [vp, C.POINTER(vp), sz, i, i, i, i, C.POINTER(vp), sz, u32p,
                                            C.POINTER(C.c_uint64)]
    L.dfx_submit_extract_frames.restype = i
    L.dfx_frames_device_bytes.argtypes = [vp]
    L.dfx_frames_device_bytes.restype = sz
    L.dfx_set_size.argtypes = [vp, i, i]
    L.dfx_set_size.restype = i
    L.dfx_device_bytes.argtypes = [vp]
    L.dfx_device_bytes.restype = sz
    L.dfx_get_stats.argtypes = [vp, C.POINTER(DfxStats)]
    L.dfx_get_stats.restype = i
    L.dfx_reset_stats.argtypes = [vp]
    if hasattr(L, "dfxi_tvl1_batch_tables"):  # test hook; a library built before it (DFX_LIBRARY A/B) still loads
        L.dfxi_tvl1_batch_tables.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
        L.dfxi_tvl1_batch_tables.restype = i
    L.dfx_last_error.argtypes = [vp]
    L.dfx_last_error.restype = C.c_char_p
    L.dfx_destroy.argtypes = [vp]
    L.dfx_device_malloc.argtypes = [vp, C.POINTER(vp), sz]
    L.dfx_device_malloc.restype = i
    L.dfx_device_free.argtypes = [vp, vp]
    L.dfx_device_free.restype = i
    L.dfx_memcpy_h2d.argtypes = [vp, vp, vp, sz]
    L.dfx_memcpy_h2d.restype = i
    L.dfx_memcpy_d2h.argtypes = [vp, vp, vp, sz]
    L.dfx_memcpy_d2h.restype = i
    L.dfx_host_alloc.argtypes = [C.POINTER(vp), sz]
    L.dfx_host_alloc.restype = i
    L.dfx_host_free.argtypes = [vp]
    L.dfx_host_free.restype = i
    _lib = L
    return L


def device_count() -> int:
    return int(load_library().dfx_device_count())


def algo_from_name(name: str) -> int:
    """Map -a=<name>; raises with the reference's runtime_error texts (src/denseflow_gpu.cpp:296, :336)."""
    L = load_library()
    out = C.c_int(0)
    rc = L.dfx_algo_from_name(name.encode(), C.byref(out))
    if rc != OK:
        buf = C.create_string_buffer(256)
        L.dfx_algo_error_message(rc, name.encode(), buf, 256)
        raise DfxError(rc, buf.value.decode())
    return out.value


def default_params() -> DfxParams:
    p = DfxParams()
    load_library().dfx_default_params(C.byref(p))
    return p


PLANAR_F32, PLANAR_F16, PLANAR_BF16 = 0, 1, 2  # DFX_PLANAR_* of include/dfx.h
SRC_ORDERS = {"bgr": 0, "rgb": 1}   # DFX_SRC_BGR / DFX_SRC_RGB
SRC_LAYOUTS = {"hwc": 0, "chw": 1}  # DFX_SRC_INTERLEAVED / DFX_SRC_PLANAR


def _planar_dtype(dtype):
    """(DFX_PLANAR_* code, numpy dtype of the array that holds the planes) for np.float32, np.float16 or "bfloat16" (which
    numpy has no type for: its planes come back as np.uint16 bit patterns)."""
    if isinstance(dtype, str):
        if dtype == "bfloat16":
            return PLANAR_BF16, np.dtype(np.uint16)
        if dtype not in ("float32", "float16"):
            raise ValueError('dtype must be np.float32, np.float16 or "bfloat16"')
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError('dtype must be np.float32, np.float16 or "bfloat16"') from None
    if dt == np.float32:
        return PLANAR_F32, dt
    if dt == np.float16:
        return PLANAR_F16, dt
    raise ValueError('dtype must be np.float32, np.float16 or "bfloat16"')


WARP_U8 = 3                               # DFX_WARP_U8: the fourth out_dtype of dfx_warp_device
WARP_BORDERS = {"zero": 0, "clamp": 1}    # DFX_WARP_BORDER_ZERO / DFX_WARP_BORDER_CLAMP
WARP_SAMPLES = {"bilinear": 0, "nearest": 1}  # DFX_SAMPLE_BILINEAR / DFX_SAMPLE_NEAREST
WARP_INVALIDS = {"zero": 0, "keep": 1}    # DFX_WARP_INVALID_ZERO / DFX_WARP_INVALID_KEEP


GM_MODELS = {"translation": 0, "affine": 1}  # DFX_GM_TRANSLATION / DFX_GM_AFFINE
GM_MAX_ROUNDS = 8


def _gm_settings(model, rounds, thr, growth):
    """(model code, rounds, thr, growth) checked as dfx_global_motion_device checks them, before the library is reached."""
    if not isinstance(model, str) or model not in GM_MODELS:
        raise ValueError('model must be "translation" or "affine"')
    if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or not 1 <= int(rounds) <= GM_MAX_ROUNDS:
        raise ValueError("rounds must be an integer 1 .. 8")
    thr32, growth32 = np.float32(thr), np.float32(growth)
    if not np.isfinite(thr32) or not thr32 > 0:
        raise ValueError("thr must be finite and > 0")
    if not np.isfinite(growth32) or not growth32 >= 1:
        raise ValueError("growth must be finite and >= 1")
    return GM_MODELS[model], int(rounds), float(thr32), float(growth32)


def _gm_info(rec):
    """The counts and the status of n result records (a GM_RESULT_DTYPE array) as the wrappers return them."""
    return {"valid": rec["valid"].copy(), "inliers": rec["inliers"].copy(), "status": rec["status"].copy(),
            "rounds": rec["rounds"].copy()}


MEDIAN_MODES = {"all": 0, "fill": 1}  # DFX_MEDIAN_ALL / DFX_MEDIAN_FILL
MEDIAN_MAX_PASSES = 64


def _median_settings(ksize, mode, passes, has_mask):
    """(ksize, mode code, passes) checked as dfx_flow_median_device checks them, before the library is reached."""
    if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)) or int(ksize) not in (3, 5):
        raise ValueError("ksize must be 3 or 5")
    if not isinstance(mode, str) or mode not in MEDIAN_MODES:
        raise ValueError('mode must be "all" or "fill"')
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= int(passes) <= MEDIAN_MAX_PASSES:
        raise ValueError("passes must be an integer 1 .. 64")
    if mode == "fill" and not has_mask:
        raise ValueError('mode "fill" needs a mask')
    return int(ksize), MEDIAN_MODES[mode], int(passes)


CHAIN_EMITS = {"last": 0, "all": 1}  # DFX_CHAIN_LAST / DFX_CHAIN_ALL


def _chain_settings(n, length, first, hop, anchors, anchor_step, emit, border):
    """(length, first, hop, anchors, anchor_step, emit code, border code) checked as dfx_flow_chain_device checks them,
    before the library is reached; anchors None: as many chains as fit into the n flows (possibly none)."""
    def whole(v, name):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer")
        return int(v)

    length, first, hop, anchor_step = whole(length, "length"), whole(first, "first"), whole(hop, "hop"), whole(anchor_step, "anchor_step")
    if length < 1:
        raise ValueError("length must be >= 1")
    if hop == 0:
        raise ValueError("hop must not be 0")
    if anchor_step < 1:
        raise ValueError("anchor_step must be >= 1")
    if not isinstance(emit, str) or emit not in CHAIN_EMITS:
        raise ValueError('emit must be "last" or "all"')
    code = _warp_border(border)
    k1 = (length - 1) * hop
    lo, hi = first + min(k1, 0), first + max(k1, 0)  # the lowest and highest link index of anchor 0
    if anchors is None:
        if first < 0 or lo < 0:
            raise ValueError("first: a link index first + k * hop lies below 0")
        anchors = max(0, (n - 1 - hi) // anchor_step + 1)
    else:
        anchors = whole(anchors, "anchors")
        if anchors < 0:
            raise ValueError("anchors must be >= 0")
        if anchors and (lo < 0 or hi + (anchors - 1) * anchor_step >= n):
            raise ValueError("anchors: a link index first + j * anchor_step + k * hop lies outside the flows")
    return length, first, hop, anchors, anchor_step, CHAIN_EMITS[emit], code


PROJECT_WORDS = 3  # 64-bit words per pixel of the projection's workspace (Wsum, Su, Sv)


def _project_settings(t, scale, min_weight):
    """(t, scale, min_weight) as float32 values, checked as dfx_flow_project_device checks them, before the library is
    reached; scale None: -t (the flow back to time 0)."""
    def real(v, name):
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number")
        with np.errstate(over="ignore"):
            v32 = np.float32(v)
        if not np.isfinite(v32):
            raise ValueError(f"{name} must be finite")
        return v32

    t32 = real(t, "t")
    if t32 == 0:
        raise ValueError("t must be nonzero")
    scale32 = -t32 if scale is None else real(scale, "scale")
    mw32 = real(min_weight, "min_weight")
    if not mw32 >= 0:
        raise ValueError("min_weight must be >= 0")
    return float(t32), float(scale32), float(mw32)


SPLAT_MODES = {"mean": 0, "sum": 1}  # DFX_SPLAT_MEAN / DFX_SPLAT_SUM
SPLAT_HOLES = {"zero": 0, "keep": 1}  # DFX_SPLAT_HOLE_ZERO / DFX_SPLAT_HOLE_KEEP
SPLAT_MAX_CHANNELS = 4


def _splat_settings(t, min_weight, mode, holes, src_u8, out_u8):
    """(t, min_weight, mode code, hole-mode code), t and min_weight as float32 values, checked as dfx_splat_device checks
    them, before the library is reached.  src_u8 / out_u8: whether the source and the output are 8-bit."""
    t, _, min_weight = _project_settings(t, None, min_weight)
    if not isinstance(mode, str) or mode not in SPLAT_MODES:
        raise ValueError('mode must be "mean" or "sum"')
    if not isinstance(holes, str) or holes not in SPLAT_HOLES:
        raise ValueError('holes must be "zero" or "keep"')
    if out_u8 and not src_u8:
        raise ValueError("dtype uint8 needs uint8 images: a float32 payload gives float32")
    if out_u8 and mode != "mean":
        raise ValueError('mode "sum" needs dtype float32')
    return t, min_weight, SPLAT_MODES[mode], SPLAT_HOLES[holes]


INTERP_MAX_PASSES = 16


def _interp_settings(t, min_weight, fill_passes, ksize):
    """(t, min_weight, fill_passes, ksize), t and min_weight as float32 values, checked as dfx_interpolate_device checks
    them, before the library is reached."""
    def real(v, name):
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a number")
        with np.errstate(over="ignore"):
            v32 = np.float32(v)
        if not np.isfinite(v32):
            raise ValueError(f"{name} must be finite")
        return v32

    t32 = real(t, "t")
    if not (t32 > 0 and t32 < 1):
        raise ValueError("t must be inside (0, 1)")
    mw32 = real(min_weight, "min_weight")
    if not mw32 >= 0:
        raise ValueError("min_weight must be >= 0")
    if isinstance(fill_passes, bool) or not isinstance(fill_passes, (int, np.integer)) or not 0 <= fill_passes <= INTERP_MAX_PASSES:
        raise ValueError("fill_passes must be an integer 0 .. 16")
    if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)) or ksize not in (3, 5):
        raise ValueError("ksize must be 3 or 5")
    return float(t32), float(mw32), int(fill_passes), int(ksize)


def _interp_work_bytes(w, h, fill_passes):
    """interp_work_bytes of denseflow_amd/csrc/interpolate_kernels.hip: what dfx_interpolate_work_bytes returns for one pair."""
    up16 = lambda b: (b + 15) & ~15  # noqa: E731
    pp = ((w + 3) & ~3) * h
    sums, g, hole = up16(w * h * PROJECT_WORDS * 8), up16(16 * pp), up16(2 * pp)
    return sums + g * (2 if fill_passes > 0 else 1) + hole * (1 + (fill_passes > 0) + (fill_passes > 1)) + 8


COLOUR_NORMS = {"fixed": 0, "flow": 1, "batch": 2}  # DFX_COLOUR_NORM_FIXED / _FLOW / _BATCH
COLOUR_WHEEL_SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))


def colour_wheel() -> np.ndarray:
    """The (55, 3) uint8 RGB colour wheel of Baker et al. 2011 that dfx_flow_colour_device interpolates on (include/dfx.h)."""
    rows = []
    for name, length in COLOUR_WHEEL_SEGMENTS:
        for j in range(length):
            q = 255 * j // length
            rows.append({"RY": (255, q, 0), "YG": (255 - q, 255, 0), "GC": (0, 255, q), "CB": (0, 255 - q, 255),
                         "BM": (q, 0, 255), "MR": (255, 0, 255 - q)}[name])
    return np.array(rows, np.uint8)


def _colour_settings(norm, max_rad, order, layout, unknown, alpha):
    """(norm code, max_rad, order code, layout code, unknown bytes, alpha256), checked as dfx_flow_colour_device checks them,
    before the library is reached.  max_rad belongs to norm="fixed" and to it alone."""
    if not isinstance(norm, str) or norm not in COLOUR_NORMS:
        raise ValueError('norm must be "fixed", "flow" or "batch"')
    code = COLOUR_NORMS[norm]
    rad = 0.0
    if code == 0:
        if isinstance(max_rad, (bool, str)) or not isinstance(max_rad, (int, float, np.integer, np.floating)):
            raise ValueError('max_rad must be a number with norm="fixed"')
        with np.errstate(over="ignore"):
            r32 = np.float32(max_rad)
        if not (np.isfinite(r32) and np.float32(1e-6) <= r32 <= np.float32(1e9)):
            raise ValueError("max_rad must be finite and in [1e-6, 1e9]")
        rad = float(r32)
    elif max_rad is not None:
        raise ValueError('max_rad applies to norm="fixed" only')
    if not isinstance(order, str) or order not in SRC_ORDERS:
        raise ValueError('order must be "bgr" or "rgb"')
    lay = _warp_layout(layout)
    try:
        unk = tuple(int(c) for c in unknown)
        ok = len(unk) == 3 and all(0 <= c <= 255 and int(u) == u and not isinstance(u, bool) for c, u in zip(unk, unknown))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("unknown must be three integers 0 .. 255")
    if isinstance(alpha, (bool, str)) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0 <= alpha <= 1:
        raise ValueError("alpha must be a number in [0, 1]")
    return code, rad, SRC_ORDERS[order], lay, unk, int(round(float(alpha) * 256))


HIST_KINDS = {"hof": 1, "mbhx": 2, "mbhy": 4}  # DFX_HIST_HOF / _MBHX / _MBHY
HIST_NORMS = {"none": 0, "l1": 1, "l1_sqrt": 2, "l2": 3}  # DFX_HIST_NORM_*
HIST_CELLS = (4, 8, 16, 32)


def _hist_kinds(kinds):
    """The bit set of a kind name or a sequence of distinct kind names."""
    names = (kinds,) if isinstance(kinds, str) else kinds
    try:
        names = tuple(names)
        ok = len(names) > 0 and all(isinstance(k, str) and k in HIST_KINDS for k in names) and len(set(names)) == len(names)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError('kinds must be one or more of "hof", "mbhx", "mbhy", each once')
    return sum(HIST_KINDS[k] for k in names)


def _hist_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= bins <= 16:
        raise ValueError("bins must be an integer 2 .. 16")
    return int(bins)


def flow_hist_slots(kinds=("hof", "mbhx", "mbhy"), bins: int = 8):
    """The names of the D slots of a cell in their order (dfx_flow_hist_device): "hof0" .. "hof<bins-1>", "hof_still",
    "mbhx0" .., "mbhy0" ..; the channels lie in that order whatever the order of `kinds`."""
    code, bins = _hist_kinds(kinds), _hist_bins(bins)
    names = []
    for k, bit in HIST_KINDS.items():
        if code & bit:
            names += [f"{k}{b}" for b in range(bins)] + (["hof_still"] if bit == 1 else [])
    return names


def _hist_settings(kinds, cell, bins, still_thr, norm):
    """(kinds code, cell, bins, still_thr, norm code, D), checked as dfx_flow_hist_device checks them, before the library is
    reached."""
    code, bins = _hist_kinds(kinds), _hist_bins(bins)
    if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or cell not in HIST_CELLS:
        raise ValueError("cell must be 4, 8, 16 or 32")
    if isinstance(still_thr, (bool, str)) or not isinstance(still_thr, (int, float, np.integer, np.floating)):
        raise ValueError("still_thr must be a finite number")
    with np.errstate(over="ignore"):
        thr = np.float32(still_thr)
    if not np.isfinite(thr):
        raise ValueError("still_thr must be a finite number")
    if not isinstance(norm, str) or norm not in HIST_NORMS:
        raise ValueError('norm must be "none", "l1", "l1_sqrt" or "l2"')
    D = ((bins + 1) if code & 1 else 0) + (bins if code & 2 else 0) + (bins if code & 4 else 0)
    return code, int(cell), bins, float(thr), HIST_NORMS[norm], D


def _warp_border(border):
    if not isinstance(border, str) or border not in WARP_BORDERS:
        raise ValueError('border must be "zero" or "clamp"')
    return WARP_BORDERS[border]


def _warp_planes_settings(sample, border, invalid):
    """(sample, border, invalid) codes of dfx_warp_planes_device."""
    if not isinstance(sample, str) or sample not in WARP_SAMPLES:
        raise ValueError('sample must be "bilinear" or "nearest"')
    if not isinstance(invalid, str) or invalid not in WARP_INVALIDS:
        raise ValueError('invalid must be "zero" or "keep"')
    return WARP_SAMPLES[sample], _warp_border(border), WARP_INVALIDS[invalid]


def _warp_planes_np_dtypes(src, sample, dtype):
    """(src code, out code, numpy dtype of the result) for a numpy source dtype.  Bilinear: float32, float16, or uint16 holding
    bfloat16 bit patterns; dtype (None: the source's) is np.float32, np.float16 or "bfloat16".  Nearest: any 1-, 2- or 4-byte
    integer or float type, copied as bit patterns; dtype must be None or the source's."""
    src = np.dtype(src)
    if sample:
        if src.kind not in "iuf" or src.itemsize not in (1, 2, 4):
            raise ValueError('planes must be a 1-, 2- or 4-byte integer or float array for sample="nearest"')
        same = dtype is None or (src == np.uint16 if isinstance(dtype, str) and dtype == "bfloat16" else np.dtype(dtype) == src)
        if not same:
            raise ValueError('sample="nearest" copies elements: dtype must be None or the planes\' dtype')
        code = {1: WARP_U8, 2: PLANAR_F16, 4: PLANAR_F32}[src.itemsize]
        return code, code, src
    codes = {np.dtype(np.float32): PLANAR_F32, np.dtype(np.float16): PLANAR_F16, np.dtype(np.uint16): PLANAR_BF16}
    if src not in codes:
        raise ValueError('planes must be float32, float16 or uint16 (bfloat16 bit patterns) for sample="bilinear" '
                         '(integers take sample="nearest")')
    if dtype is None:
        return codes[src], codes[src], src
    out_code, np_dt = _planar_dtype(dtype)
    return codes[src], out_code, np_dt


def _warp_layout(layout):
    if not isinstance(layout, str) or layout not in SRC_LAYOUTS:
        raise ValueError('layout must be "hwc" or "chw"')
    return SRC_LAYOUTS[layout]


def _warp_dtype(dtype):
    """(out_dtype code, numpy dtype of the array that holds the warped images): np.uint8 next to what _planar_dtype takes."""
    if dtype is np.uint8 or (isinstance(dtype, (str, np.dtype)) and dtype == "uint8"):
        return WARP_U8, np.dtype(np.uint8)
    try:
        return _planar_dtype(dtype)
    except ValueError:
        raise ValueError('dtype must be np.uint8, np.float32, np.float16 or "bfloat16"') from None


# -- what the calls on finished flows (fb_check .. flow_colour) share: how flows and per-item planes lie in memory.  A
# dimension of extent 1 takes its stride from the dense layout, not from the tensor (torch leaves such a stride arbitrary).
def _flow_geometry(t, H, W, what, lead="M", n=None, tail=""):
    """(row pitch, plane stride, flow stride), in floats, of a torch.float32 tensor of flows (lead, 2, H, W), read from its
    strides; with n, there must be exactly n flows.  `lead` and `tail` only word the refusal."""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or tuple(t.shape[1:]) != (2, H, W) or \
            (n is not None and t.shape[0] != n):
        raise ValueError(f"{what} must be an ({lead}, 2, H, W) torch.float32 tensor{tail}")
    st = t.stride()
    pitch = st[2] if H > 1 else W
    plane, flow = st[1], (st[0] if t.shape[0] > 1 else 2 * st[1])
    if (st[3] != 1 and W > 1) or pitch < W or plane < H * pitch or flow < 2 * plane:
        raise ValueError(f"{what}: the innermost dimension must be contiguous and rows, planes and flows must not overlap")
    return pitch, plane, flow


def _plane_geometry(t, n, H, W, dtype, what, lead="M", noun="masks"):
    """(row pitch, stride), in elements, of a torch tensor of n planes (n, H, W) of that dtype — masks, weights — read from
    its strides.  `lead` and `noun` only word the refusals."""
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n, H, W):
        raise ValueError(f"{what} must be an ({lead}, H, W) {dtype} tensor")
    st = t.stride()
    pitch = st[1] if H > 1 else W
    stride = st[0] if n > 1 else H * pitch
    if (st[2] != 1 and W > 1) or pitch < W or stride < H * pitch:
        raise ValueError(f"{what}: the innermost dimension must be contiguous and rows and {noun} must not overlap")
    return pitch, stride


def _np_flows(a, H, W, what="flows", lead="M", n=None, tail=""):
    """Flows given to a numpy wrapper as a contiguous (lead, 2, H, W) float32 array; with n, exactly n flows."""
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim != 4 or a.shape[1:] != (2, H, W) or (n is not None and a.shape[0] != n):
        raise ValueError(f"{what} must be ({lead}, 2, H, W) float32{tail}")
    return np.ascontiguousarray(a)


def _np_planes(a, n, H, W, dtype, what, lead="M"):
    """An optional (n, H, W) array of that dtype given to a numpy wrapper, contiguous; None stays None."""
    if a is None:
        return None
    a = np.asarray(a)
    if a.dtype != dtype or a.shape != (n, H, W):
        raise ValueError(f"{what} must be ({lead}, H, W) {np.dtype(dtype).name}")
    return np.ascontiguousarray(a)


def _source_codes(channels, order, layout):
    if order not in SRC_ORDERS:
        raise ValueError('order must be "bgr" or "rgb"')
    if layout not in SRC_LAYOUTS:
        raise ValueError('layout must be "hwc" or "chw"')
    if channels != 3 and (SRC_ORDERS[order] or SRC_LAYOUTS[layout]):
        raise ValueError("order and layout apply to a 3-channel source only")
    return SRC_ORDERS[order], SRC_LAYOUTS[layout]


class FlowEngine:
    """One handle = one device + one private stream set (not thread-safe), sized for width x height (set_size re-plans it
    for another size inside its allocations)."""

    def __init__(self, width: int, height: int, algorithm: str = "tvl1", device: int = 0,
                 params: DfxParams | None = None, **knobs):
        self._L = load_library()
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        self._device = int(device)
        self.algorithm = algorithm
        # "frames": a handle without flow state, for the colour frame extraction (no -a=<name> maps to it)
        algo = ALGO_FRAMES if algorithm == "frames" else algo_from_name(algorithm)
        if knobs:
            if params is None:
                params = default_params()
            for k, v in knobs.items():
                setattr(params, k, v)
        rc = self._L.dfx_create(C.byref(self._h), int(device), algo, self.width, self.height,
                                C.byref(params) if params is not None else None)
        if rc != OK:
            msg = self._L.dfx_last_error(None).decode()
            self._h = C.c_void_p()
            raise DfxError(rc, msg or f"dfx_create failed with status {rc}")

    # -- helpers -----------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != OK:
            raise DfxError(rc, self._L.dfx_last_error(self._h).decode() or f"dfx status {rc}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.dfx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- one handle, many frame sizes (dfx_set_size) ------------------------------------------------------------
    def set_size(self, width: int, height: int):
        """Re-plan the engine for width x height frames inside its allocations: waits for everything outstanding, cancels
        a pending next_segments, restores the default source format.  Afterwards the engine computes what a fresh one of
        that size computes.  On failure (DfxError) it stays usable at its previous size."""
        self._pending_seg = self._armed_seg = self._pending_src = self._armed_src = None
        self._check(self._L.dfx_set_size(self._h, int(width), int(height)))
        self.width, self.height = int(width), int(height)
        self._src = self._src_fmt = None
        self._src_chw = False

    def device_bytes(self) -> int:
        """Device memory this handle holds right now, all kinds together."""
        return int(self._L.dfx_device_bytes(self._h))

    # -- frame preparation on the device (reference: cvtColor + cv::resize in load_frames_batch) ----------
    def set_source_format(self, src_width: int = 0, src_height: int = 0, channels: int = 1, order: str = "bgr",
                          layout: str = "hwc"):
        """Frames passed to calc / calc_optflows* are src_width x src_height with 1 (gray) or 3 channels from now on and are
        converted / resized to the engine's size on the device.  () restores the default.
        order "bgr" | "rgb": the channel order of a colour source.  layout "hwc": interleaved (Hs, Ws, 3) frames; "chw":
        channels-first (3, Hs, Ws) frames, three byte planes (dfx_set_source_format_ex)."""
        o, l = _source_codes(int(channels), order, layout) if src_width else (0, 0)
        if o or l:
            self._check(self._L.dfx_set_source_format_ex(self._h, int(src_width), int(src_height), int(channels), o, l, 0))
        else:
            self._check(self._L.dfx_set_source_format(self._h, int(src_width), int(src_height), int(channels)))
        self._src_chw = bool(l)
        if not src_width:
            self._src = None
        elif l:
            self._src = (3, int(src_height), int(src_width))
        else:
            self._src = (int(src_height), int(src_width)) + ((3,) if channels == 3 else ())
        self._src_fmt = (int(src_width), int(src_height), int(channels), o, l) if src_width else None

    def _host_pitch(self, frame) -> int:
        """Bytes per row of a host frame as the library counts them: for a channels-first frame the row pitch of one plane."""
        return frame.strides[1] if getattr(self, "_src_chw", False) and frame.ndim == 3 else frame.strides[0]

    def _frame_shape(self):
        return getattr(self, "_src", None) or (self.height, self.width)

    def prepare_frames(self, frames, order: str = "bgr", layout: str = "hwc"):
        """cvtColor(BGR2GRAY) + cv::resize to the engine's size for a list of (h, w) or (h, w, 3) uint8 frames.
        order "rgb": the colour frames are R, G, B; layout "chw": they are (3, h, w)."""
        src = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        n = len(src)
        out = [np.empty((self.height, self.width), np.uint8) for _ in range(n)]
        if order not in SRC_ORDERS or layout not in SRC_LAYOUTS:
            _source_codes(3, order, layout)
        chw = layout == "chw"
        if n == 0:
            return out
        shp = src[0].shape
        if chw:
            if any(f.shape != shp for f in src) or len(shp) != 3 or shp[0] != 3:
                raise ValueError("frames must share one (3, h, w) shape")
            sh, sw, ch = shp[1], shp[2], 3
        else:
            if any(f.shape != shp for f in src) or len(shp) not in (2, 3) or (len(shp) == 3 and shp[2] != 3):
                raise ValueError("frames must share one (h, w) or (h, w, 3) shape")
            sh, sw, ch = shp[0], shp[1], 1 if len(shp) == 2 else 3
        o, l = _source_codes(ch, order, layout)
        sp = (C.c_void_p * n)(*[f.ctypes.data for f in src])
        op = (C.c_void_p * n)(*[f.ctypes.data for f in out])
        if o or l:
            self._check(self._L.dfx_prepare_frames_layout(self._h, sp, sw if chw else sw * ch, sw, sh, ch, o, l, n, op,
                                                          self.width))
        else:
            self._check(self._L.dfx_prepare_frames(self._h, sp, sw * ch, sw, sh, ch, n, op, self.width))
        return out

    def prepare_frames_layout_device(self, d_src_ptr: int, src_pitch: int, src_frame_stride: int, plane_stride: int,
                                     src_width: int, src_height: int, channels: int, order: str, layout: str, n: int,
                                     d_gray_ptr: int, gray_pitch: int, gray_frame_stride: int):
        """prepare_frames_device for a source of the given order and layout; layout "chw": src_pitch is the row pitch of one
        plane and plane c of a frame starts c * plane_stride bytes behind it (0: src_pitch * src_height)."""
        o, l = _source_codes(int(channels), order, layout)
        self._check(self._L.dfx_prepare_frames_layout_device(self._h, d_src_ptr, src_pitch, src_frame_stride, plane_stride,
                                                             int(src_width), int(src_height), int(channels), o, l, int(n),
                                                             d_gray_ptr, gray_pitch, gray_frame_stride))

    def prepare_frames_device(self, d_src_ptr: int, src_pitch: int, src_frame_stride: int, src_width: int,
                              src_height: int, channels: int, n: int, d_gray_ptr: int, gray_pitch: int,
                              gray_frame_stride: int):
        self._check(self._L.dfx_prepare_frames_device(self._h, d_src_ptr, src_pitch, src_frame_stride, int(src_width),
                                                      int(src_height), int(channels), int(n), d_gray_ptr, gray_pitch,
                                                      gray_frame_stride))

    # -- several short clips in one FlowBuffer (dfx_next_segments) ------------------------------------------
    def next_segments(self, seg_frames, src_sizes=None, channels: int = 1):
        """The NEXT calc_optflows* / submit_optflows call carries len(seg_frames) clips back to back, clip s being
        seg_frames[s] consecutive frames; pairs are formed inside each clip only (outputs in clip order).

        src_sizes: one (width, height) per clip (dfx_next_segments_src) — that one call then accepts frames of differing
        shapes, (h, w) for channels = 1 or (h, w, 3) for channels = 3, each clip with its own row pitch (the frames of a
        clip may be views with padded rows; they must share their strides); every clip is converted / resized to the
        engine's size on the device."""
        self._pending_seg = [int(x) for x in seg_frames]
        self._pending_src = None
        if src_sizes is not None:
            src = [(int(w), int(h)) for w, h in src_sizes]
            if len(src) != len(self._pending_seg) or channels not in (1, 3):
                self._pending_seg = None
                raise ValueError("one (width, height) per clip, and channels 1 or 3")
            self._pending_src = (src, int(channels))

    def _num_pairs(self, n: int, step: int) -> int:
        seg, self._pending_seg = getattr(self, "_pending_seg", None), None
        src, self._pending_src = getattr(self, "_pending_src", None), None
        self._armed_seg = self._armed_src = self._armed_pitch = None
        if seg is None:
            return max(n - abs(step), 0)
        if sum(seg) != n or min(seg, default=0) < 0:
            raise ValueError("segment lengths must be >= 0 and add up to the number of frames")
        self._armed_seg, self._armed_src = seg, src
        return sum(max(x - abs(step), 0) for x in seg)

    def _frames_in(self, frames):
        """The frames of a call as uint8 arrays: C-contiguous, or — under next_segments(src_sizes=...) — with dense pixels
        and any row pitch."""
        if getattr(self, "_pending_src", None) is None:
            return [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        out = []
        for f in frames:
            f = np.asarray(f)
            dense = f.dtype == np.uint8 and f.ndim in (2, 3) and f.strides[-1] == 1 and (f.ndim == 2 or f.strides[1] == f.shape[2])
            out.append(f if dense else np.ascontiguousarray(f, dtype=np.uint8))
        return out

    def _check_shapes(self, frames):
        src = getattr(self, "_armed_src", None)
        if src is None:
            for f in frames:
                if f.shape != self._frame_shape():
                    raise ValueError("frame shape does not match the engine")
            return
        sizes, ch = src
        pitches, k = [], 0
        for (w, h), n in zip(sizes, self._armed_seg):
            want = (h, w) if ch == 1 else (h, w, 3)
            clip = frames[k:k + n]
            k += n
            if any(f.shape != want or f.strides != clip[0].strides for f in clip):
                self._armed_seg = self._armed_src = None
                raise ValueError("the frames of a clip must have its declared shape and one row pitch")
            pitches.append(clip[0].strides[0] if clip else w * ch)
        self._armed_pitch = pitches

    def _arm(self):  # right in front of the library call the declaration is meant for
        seg, self._armed_seg = getattr(self, "_armed_seg", None), None
        src, self._armed_src = getattr(self, "_armed_src", None), None
        if seg is None:
            return
        cnt = max(len(seg), 1)
        if src is None:
            self._check(self._L.dfx_next_segments(self._h, (C.c_int * cnt)(*seg), len(seg)))
            return
        sizes, ch = src
        pitches = getattr(self, "_armed_pitch", None) or [w * ch for w, _ in sizes]
        wh = [v for s in sizes for v in s]
        self._check(self._L.dfx_next_segments_src(self._h, (C.c_int * cnt)(*seg), (C.c_int * (2 * cnt))(*wh),
                                                  (C.c_size_t * cnt)(*pitches), len(seg), ch))

    # -- the hot path ------------------------------------------------------------------------
    def _seeds_in(self, init, m: int):
        """The initial flows of a host-pointer call: m (H, W, 2) float32 arrays with dense pixels and one common row pitch
        (views with padded rows are taken as they are).  Returns (arrays, pitch in bytes)."""
        seeds = []
        for s in init:
            s = np.asarray(s)
            ok = s.dtype == np.float32 and s.shape == (self.height, self.width, 2) and s.strides[1:] == (8, 4)
            seeds.append(s if ok else np.ascontiguousarray(s, dtype=np.float32))
        if len(seeds) != m or any(s.shape != (self.height, self.width, 2) for s in seeds):
            raise ValueError("init must hold one (H, W, 2) float32 flow per output flow")
        pitch = seeds[0].strides[0] if seeds and self.height > 1 else self.width * 8
        if any(self.height > 1 and s.strides[0] != pitch for s in seeds):
            seeds = [np.ascontiguousarray(s) for s in seeds]
            pitch = self.width * 8
        return seeds, pitch

    def calc(self, frame_a: np.ndarray, frame_b: np.ndarray, init: np.ndarray | None = None) -> np.ndarray:
        """alg->calc(a, b): one (H, W, 2) float32 flow, channel 0 = u (x), 1 = v (y).
        init: an (H, W, 2) float32 flow in pixels to start from (TVL1's useInitialFlow, Farneback's
        OPTFLOW_USE_INITIAL_FLOW; dfx_calc_batch_init with the two frames) instead of zero."""
        if init is not None:
            return self.calc_optflows([frame_a, frame_b], 1, init=[init])[0]
        a = np.ascontiguousarray(frame_a, dtype=np.uint8)
        b = np.ascontiguousarray(frame_b, dtype=np.uint8)
        if a.shape != self._frame_shape() or b.shape != a.shape:
            raise ValueError("frame shape does not match the engine")
        out = np.empty((self.height, self.width, 2), dtype=np.float32)
        self._check(self._L.dfx_calc(self._h, a.ctypes.data, self._host_pitch(a), b.ctypes.data, self._host_pitch(b),
                                     out.ctypes.data, out.strides[0]))
        return out

    def calc_optflows(self, frames_gray, step: int, init=None):
        """The loop of DenseFlow::calc_optflows_imp (src/denseflow_gpu.cpp:307-342) for one FlowBuffer.
        init: one (H, W, 2) float32 initial flow per output flow, in output order (dfx_calc_batch_init)."""
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        flows = [np.empty((self.height, self.width, 2), dtype=np.float32) for _ in range(m)]
        if m == 0:
            return flows
        self._check_shapes(frames)
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        op = (C.c_void_p * m)(*[f.ctypes.data for f in flows])
        if init is not None:
            try:
                seeds, ipitch = self._seeds_in(init, m)
            except ValueError:
                self._armed_seg = self._armed_src = None
                raise
            ip = (C.c_void_p * m)(*[s.ctypes.data for s in seeds])
            self._arm()
            self._check(self._L.dfx_calc_batch_init(self._h, fp, self._host_pitch(frames[0]), n, int(step), ip, ipitch, op,
                                                    self.width * 8))
            return flows
        self._arm()
        self._check(self._L.dfx_calc_batch(self._h, fp, self._host_pitch(frames[0]), n, int(step), op, self.width * 8))
        return flows

    # -- asynchronous FlowBuffers (dfx_submit_batch* / dfx_wait) -----------------------------------------------
    def submit_optflows(self, frames_gray, step: int, bound: float | None = None):
        """dfx_submit_batch (bound None: float flows) or dfx_submit_batch_u8 (planes bounded to [-bound, bound]).
        Returns (ticket, outputs); the outputs are valid after wait(ticket).  The output arrays are created here and
        must be kept alive by the caller until then."""
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        self._check_shapes(frames)
        t = C.c_uint64(0)
        fp = (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in frames])
        pitch = self._host_pitch(frames[0]) if n else self.width
        if bound is None:
            flows = [np.empty((self.height, self.width, 2), dtype=np.float32) for _ in range(m)]
            op = (C.c_void_p * max(m, 1))(*[f.ctypes.data for f in flows])
            self._arm()
            self._check(self._L.dfx_submit_batch(self._h, fp, pitch, n, int(step), op, self.width * 8, C.byref(t)))
            return t.value, flows
        img_x = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        img_y = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        xp = (C.c_void_p * max(m, 1))(*[f.ctypes.data for f in img_x])
        yp = (C.c_void_p * max(m, 1))(*[f.ctypes.data for f in img_y])
        self._arm()
        self._check(self._L.dfx_submit_batch_u8(self._h, fp, pitch, n, int(step), -float(bound), float(bound), xp, yp,
                                                self.width, C.byref(t)))
        return t.value, (img_x, img_y)

    def wait(self, ticket: int = 0):
        self._check(self._L.dfx_wait(self._h, int(ticket)))

    def calc_optflows_device(self, d_frames_ptr: int, pitch: int, frame_stride: int, n_frames: int, step: int,
                             d_flows_ptr: int, flow_stride_floats: int, init: int | None = None,
                             init_stride_floats: int | None = None):
        """Frames and flows already resident in HBM (raw device pointers, e.g. torch .data_ptr()).
        init: device pointer of the initial flows, in the layout of the flows (dfx_calc_batch_init_device), flow i at
        init + i * init_stride_floats (default: flow_stride_floats); it may be d_flows_ptr itself with the same stride —
        refinement in place."""
        self._num_pairs(n_frames, step)
        self._arm()
        if init is not None:
            self._check(self._L.dfx_calc_batch_init_device(
                self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step), init,
                flow_stride_floats if init_stride_floats is None else int(init_stride_floats), d_flows_ptr,
                flow_stride_floats))
            return
        self._check(self._L.dfx_calc_batch_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step),
                                                  d_flows_ptr, flow_stride_floats))

    # -- planar float flows for tensor consumers (dfx_calc_batch_planar*) --------------------------------------
    def calc_optflows_planar(self, frames_gray, step: int, bound: float | None = None, dtype=np.float32) -> np.ndarray:
        """calc_optflows as one (M, 2, H, W) array: channel 0 = u, 1 = v, written as planes by the engine's last kernel.
        bound None: the raw flow values; bound > 0: clamp(x, -bound, bound) / bound in float32, NaN -> 0.
        dtype: np.float32, or np.float16 / "bfloat16" — the float32 value rounded once (to nearest even) in the same store
        (dfx_calc_batch_planar_as); bfloat16 planes come back as an np.uint16 array of bit patterns."""
        code, np_dt = _planar_dtype(dtype)
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        out = np.empty((m, 2, self.height, self.width), dtype=np_dt)
        if m == 0:
            return out
        self._check_shapes(frames)
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        up = (C.c_void_p * m)(*[out[k, 0].ctypes.data for k in range(m)])
        vp = (C.c_void_p * m)(*[out[k, 1].ctypes.data for k in range(m)])
        pitch = self._host_pitch(frames[0])
        self._arm()
        if code != PLANAR_F32:
            self._check(self._L.dfx_calc_batch_planar_as(self._h, fp, pitch, n, int(step),
                                                         0.0 if bound is None else float(bound), code, up, vp,
                                                         self.width * np_dt.itemsize))
            return out
        self._check(self._L.dfx_calc_batch_planar(self._h, fp, pitch, n, int(step),
                                                  0.0 if bound is None else float(bound), up, vp, self.width * 4))
        return out

    def calc_optflows_planar_device(self, d_frames_ptr: int, pitch: int, frame_stride: int, n_frames: int, step: int,
                                    bound: float | None, d_out_ptr: int, row_pitch_floats: int, plane_stride_floats: int,
                                    flow_stride_floats: int, dtype=None):
        """Frames and planes resident in HBM (raw device pointers): flow i's u plane at d_out + i * flow_stride_floats, its
        v plane plane_stride_floats behind it, rows row_pitch_floats apart.
        dtype None: float32 planes (dfx_calc_batch_planar_device).  np.float32 / np.float16 / "bfloat16": planes of that
        type through dfx_calc_batch_planar_as_device, the three strides in elements of it."""
        code = None if dtype is None else _planar_dtype(dtype)[0]
        self._num_pairs(n_frames, step)
        self._arm()
        if code is not None:
            self._check(self._L.dfx_calc_batch_planar_as_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames,
                                                                int(step), 0.0 if bound is None else float(bound), code,
                                                                d_out_ptr, row_pitch_floats, plane_stride_floats,
                                                                flow_stride_floats))
            return
        self._check(self._L.dfx_calc_batch_planar_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step),
                                                         0.0 if bound is None else float(bound), d_out_ptr,
                                                         row_pitch_floats, plane_stride_floats, flow_stride_floats))

    def flow_tensor(self, frames, step: int, bound: float | None = None, out=None, init=None, dtype=None):
        """Flows of a FlowBuffer of torch frames as an (M, 2, H, W) torch tensor on the same device, the layout (and, with
        bound, the [-1, 1] scaling) a two-stream / TSN / I3D network takes: no pointer handling, no permute pass, no
        clamp-and-divide pass.

        frames: torch.uint8 tensor on this handle's device, (N, H, W), or — when a source format is set — (N, Hs, Ws) gray,
        (N, Hs, Ws, 3) interleaved colour or (N, 3, Hs, Ws) channels-first colour (layout "chw"), BGR or RGB as declared.
        Any strides as long as the innermost dimension is contiguous (interleaved: the pixel's three bytes too) and rows,
        planes and frames do not overlap; row pitch, plane stride and frame stride are taken from the tensor, so a
        permuted view of an NHWC batch or a slice of a larger tensor is read where it lies.
        dtype: torch.float32 (default), torch.float16 or torch.bfloat16 — the float32 value rounded once, to nearest even,
        in the store that writes the plane (dfx_calc_batch_planar_as_device).
        out: optional (M, 2, H, W) tensor of that dtype on that device to write into, any strides with a contiguous
        innermost dimension that do not make rows, planes or flows overlap; otherwise the result is allocated.
        bound None: raw flow values, bit for bit those of calc_optflows; bound > 0: clamp(x, -bound, bound) / bound.
        init: optional (M, 2, H, W) float32 tensor on that device, the initial flow of every output flow in raw pixels
        (whatever bound and dtype are).  With float32 planes the library reads it with the strides of `out`: without
        `out` any strides are accepted (a contiguous copy is made if needed); with `out` it must have out's strides, and it
        may be `out` itself (refinement in place).  With half planes it is made contiguous.

        Streams: torch's current stream on that device is synchronised before the call, so frames produced on it just
        before are complete; the library call returns with all its device work complete, so the result may be used on
        any stream afterwards without further synchronisation.

        Raises ValueError — before the library is reached — for a wrong dtype, device, rank or shape, a non-contiguous
        innermost dimension, overlapping rows, planes or frames, or an `out` that does not match."""
        import torch

        codes = {torch.float32: PLANAR_F32, torch.float16: PLANAR_F16, torch.bfloat16: PLANAR_BF16}
        tdt = torch.float32 if dtype is None else dtype
        if tdt not in codes:
            raise ValueError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
        code = codes[tdt]
        n, pitch, frame_stride, layout = self._tensor_frames(frames)
        dev = frames.device
        m = self._peek_pairs(n, step)
        want = (m, 2, self.height, self.width)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != tdt or out.device != dev:
                raise ValueError(f"out must be a {tdt} tensor on the frames' device")
            if tuple(out.shape) != want:
                raise ValueError(f"out must have shape {want}")
            so = out.stride()
            row_pitch = so[2] if self.height > 1 else self.width
            out_plane_stride, flow_stride = so[1], (so[0] if m > 1 else 2 * so[1])
            if so[3] != 1 or row_pitch < self.width or out_plane_stride < self.height * row_pitch or flow_stride < 2 * out_plane_stride:
                raise ValueError("out: the innermost dimension must be contiguous and rows, planes and flows must not overlap")
        self._check_devices(frames, "frames must be on this handle's device")
        if init is not None:
            if not isinstance(init, torch.Tensor) or init.dtype != torch.float32 or init.device != dev:
                raise ValueError("init must be a torch.float32 tensor on the frames' device")
            if tuple(init.shape) != want:
                raise ValueError(f"init must have shape {want}")
            if out is None or code != PLANAR_F32:
                init = init.contiguous()
            elif init.stride() != out.stride():
                raise ValueError("init must have the strides of out")
        if out is None:
            out = torch.empty(want, dtype=tdt, device=dev)
            row_pitch, out_plane_stride = self.width, self.height * self.width
            flow_stride = 2 * out_plane_stride
        self._num_pairs(n, step)
        torch.cuda.current_stream(dev).synchronize()
        if layout is not None:  # how THIS tensor lies in memory, declared for this call only
            self._set_call_layout(*layout)
            try:
                return self._flow_tensor_call(code, frames, pitch, frame_stride, n, step, bound, init, out, m, row_pitch,
                                              out_plane_stride, flow_stride)
            finally:
                self._set_call_layout(1, 0)
        return self._flow_tensor_call(code, frames, pitch, frame_stride, n, step, bound, init, out, m, row_pitch,
                                      out_plane_stride, flow_stride)

    def _flow_tensor_call(self, code, frames, pitch, frame_stride, n, step, bound, init, out, m, row_pitch, out_plane_stride,
                          flow_stride):
        self._arm()
        fptr, optr = frames.data_ptr() if n else None, out.data_ptr() if m else None
        b = 0.0 if bound is None else float(bound)
        if init is not None and m:  # (no output flow: nothing to seed)
            if code != PLANAR_F32:
                hw = self.height * self.width
                self._check(self._L.dfx_calc_batch_planar_as_init_device(
                    self._h, fptr, pitch, frame_stride, n, int(step), b, code, init.data_ptr(), self.width, hw, 2 * hw,
                    optr, row_pitch, out_plane_stride, flow_stride))
                return out
            self._check(self._L.dfx_calc_batch_planar_init_device(
                self._h, fptr, pitch, frame_stride, n, int(step), b, init.data_ptr(), optr, row_pitch, out_plane_stride,
                flow_stride))
            return out
        if code != PLANAR_F32:
            self._check(self._L.dfx_calc_batch_planar_as_device(self._h, fptr, pitch, frame_stride, n, int(step), b, code,
                                                                optr, row_pitch, out_plane_stride, flow_stride))
            return out
        self._check(self._L.dfx_calc_batch_planar_device(self._h, fptr, pitch, frame_stride, n, int(step), b, optr,
                                                         row_pitch, out_plane_stride, flow_stride))
        return out

    def _set_call_layout(self, layout: int, plane_stride: int):
        """The memory layout and plane stride of the tensor the next device-resident call reads; size, channels and order stay
        the declared ones (host frames hold dense planes and take plane stride 0)."""
        sw, sh, ch, o, _ = self._src_fmt
        self._check(self._L.dfx_set_source_format_ex(self._h, sw, sh, ch, o, int(layout), int(plane_stride)))

    def _peek_pairs(self, n: int, step: int) -> int:
        """The number of flows the next call gives for n frames, a pending next_segments included; consumes nothing."""
        seg = getattr(self, "_pending_seg", None)
        if seg is None:
            return max(n - abs(int(step)), 0)
        if sum(seg) != n or min(seg, default=0) < 0:
            raise ValueError("segment lengths must be >= 0 and add up to the number of frames")
        return sum(max(x - abs(int(step)), 0) for x in seg)

    # -- both directions of every pair and the forward-backward occlusion mask (dfx_calc_batch_bidir_device) ----
    def calc_optflows_bidir_device(self, d_frames_ptr: int, pitch: int, frame_stride: int, n_frames: int, step: int,
                                   d_fwd_ptr: int, d_bwd_ptr: int, row_pitch_floats: int, plane_stride_floats: int,
                                   flow_stride_floats: int, alpha1: float = 0.01, alpha2: float = 0.5,
                                   d_occ_fwd_ptr: int | None = None, d_occ_bwd_ptr: int | None = None, occ_pitch: int = 0,
                                   occ_stride: int = 0):
        """Frames, planes and masks resident in HBM (raw device pointers): the flows of `step` to d_fwd and those of -step to
        d_bwd, both in the layout of calc_optflows_planar_device, every frame built once; with mask pointers the
        forward-backward check of (fwd, bwd) to d_occ_fwd and of (bwd, fwd) to d_occ_bwd (uint8 planes, 0 = consistent,
        1 = occluded or leaving the frame), both None: no check."""
        self._num_pairs(n_frames, step)
        self._arm()
        self._check(self._L.dfx_calc_batch_bidir_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step),
                                                        d_fwd_ptr, d_bwd_ptr, row_pitch_floats, plane_stride_floats,
                                                        flow_stride_floats, float(alpha1), float(alpha2), d_occ_fwd_ptr,
                                                        d_occ_bwd_ptr, occ_pitch, occ_stride))

    def fb_check_device(self, d_fwd_ptr: int, d_bwd_ptr: int, row_pitch_floats: int, plane_stride_floats: int,
                        flow_stride_floats: int, n: int, alpha1: float, alpha2: float, d_occ_ptr: int, occ_pitch: int,
                        occ_stride: int, d_err_ptr: int | None = None, err_pitch_floats: int = 0,
                        err_stride_floats: int = 0):
        """The forward-backward check of n planar float32 flows that are already in device memory (dfx_fb_check_device)."""
        self._check(self._L.dfx_fb_check_device(self._h, d_fwd_ptr, d_bwd_ptr, row_pitch_floats, plane_stride_floats,
                                                flow_stride_floats, int(n), float(alpha1), float(alpha2), d_occ_ptr,
                                                occ_pitch, occ_stride, d_err_ptr, err_pitch_floats, err_stride_floats))

    def _dev_bufs(self, sizes):
        """Device buffers of the given byte sizes (dfx_device_malloc; at least one byte each) as a list of pointers."""
        ptrs = []
        try:
            for b in sizes:
                p = C.c_void_p()
                self._check(self._L.dfx_device_malloc(self._h, C.byref(p), max(int(b), 1)))
                ptrs.append(p)
        except DfxError:
            self._dev_free(ptrs)
            raise
        return ptrs

    def _dev_free(self, ptrs):
        for p in ptrs:
            self._L.dfx_device_free(self._h, p)

    @contextlib.contextmanager
    def _staged(self, ins, outs, scratch=()):
        """The device side of a numpy wrapper's call: buffers for the arrays `ins` and `outs` (None entries allowed) and for
        the `scratch` byte sizes, the inputs uploaded; yields the device pointers in that order, None for an absent array;
        on a clean exit the outputs are downloaded; the buffers are freed either way."""
        arrays = list(ins) + list(outs)
        bufs = self._dev_bufs([x.nbytes for x in arrays if x is not None] + list(scratch))
        try:
            free = iter(bufs)
            ptrs = [None if x is None else next(free) for x in arrays]
            for p, x in zip(ptrs, ins):
                if x is not None:
                    self._check(self._L.dfx_memcpy_h2d(self._h, p, x.ctypes.data, x.nbytes))
            yield ptrs + list(free)
            for p, x in zip(ptrs[len(ins):], outs):
                if x is not None:
                    self._check(self._L.dfx_memcpy_d2h(self._h, x.ctypes.data, p, x.nbytes))
        finally:
            self._dev_free(bufs)

    def _check_devices(self, first, first_msg, others=(), others_msg=""):
        """ValueError(first_msg) unless the torch tensor `first` is on this handle's device, ValueError(others_msg) unless
        the `others` (None entries allowed) are on first's."""
        dev = first.device
        if dev.type != "cuda" or (dev.index is not None and dev.index != getattr(self, "_device", dev.index)):
            raise ValueError(first_msg)
        if any(t is not None and t.device != dev for t in others):
            raise ValueError(others_msg)

    def calc_optflows_bidir(self, frames_gray, step: int, check: bool = True, alpha1: float = 0.01, alpha2: float = 0.5):
        """Both directions of every pair of a FlowBuffer, every frame uploaded and built once: (fwd, bwd, occ_fwd, occ_bwd),
        two (M, 2, H, W) float32 arrays — fwd what calc_optflows_planar gives for `step`, bwd what it gives for -step — and
        two (M, H, W) uint8 masks of the forward-backward check (0 = consistent, 1 = occluded or leaving the frame;
        alpha1 / alpha2: UnFlow's constants by default), None with check=False.  The frames go to the device through
        dfx_device_malloc / dfx_memcpy_h2d and the call is dfx_calc_batch_bidir_device."""
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames_gray]
        n = len(frames)
        if any(f.shape != self._frame_shape() for f in frames):
            raise ValueError("frame shape does not match the engine")
        m = self._num_pairs(n, step)
        H, W = self.height, self.width
        fwd, bwd = np.empty((m, 2, H, W), np.float32), np.empty((m, 2, H, W), np.float32)
        occ = (np.empty((m, H, W), np.uint8), np.empty((m, H, W), np.uint8)) if check else (None, None)
        if m == 0:
            self._armed_seg = self._armed_src = None
            return fwd, bwd, occ[0], occ[1]
        pitch = self._host_pitch(frames[0])
        fb = frames[0].nbytes
        bufs = self._dev_bufs([n * fb, fwd.nbytes, bwd.nbytes] + ([m * H * W] * 2 if check else []))
        try:
            for k, f in enumerate(frames):
                self._check(self._L.dfx_memcpy_h2d(self._h, bufs[0].value + k * fb, f.ctypes.data, fb))
            self._arm()
            self._check(self._L.dfx_calc_batch_bidir_device(
                self._h, bufs[0], pitch, fb, n, int(step), bufs[1], bufs[2], W, H * W, 2 * H * W, float(alpha1),
                float(alpha2), bufs[3] if check else None, bufs[4] if check else None, W, H * W))
            self._check(self._L.dfx_memcpy_d2h(self._h, fwd.ctypes.data, bufs[1], fwd.nbytes))
            self._check(self._L.dfx_memcpy_d2h(self._h, bwd.ctypes.data, bufs[2], bwd.nbytes))
            if check:
                self._check(self._L.dfx_memcpy_d2h(self._h, occ[0].ctypes.data, bufs[3], occ[0].nbytes))
                self._check(self._L.dfx_memcpy_d2h(self._h, occ[1].ctypes.data, bufs[4], occ[1].nbytes))
        finally:
            self._dev_free(bufs)
        return fwd, bwd, occ[0], occ[1]

    def fb_check(self, fwd, bwd, alpha1: float = 0.01, alpha2: float = 0.5, want_err: bool = False):
        """The forward-backward check of n flows given as (n, 2, H, W) float32 arrays: the (n, H, W) uint8 mask of fwd against
        bwd (0 = consistent, 1 = occluded or leaving the frame), and with want_err=True (mask, err) with the (n, H, W)
        float32 squared residual, +inf where the flow leaves the frame (dfx_fb_check_device)."""
        H, W = self.height, self.width
        fwd, bwd = np.ascontiguousarray(fwd, dtype=np.float32), np.ascontiguousarray(bwd, dtype=np.float32)
        if fwd.ndim != 4 or fwd.shape[1:] != (2, H, W) or bwd.shape != fwd.shape:
            raise ValueError("fwd and bwd must both be (n, 2, H, W)")
        n = fwd.shape[0]
        occ = np.empty((n, H, W), np.uint8)
        err = np.empty((n, H, W), np.float32) if want_err else None
        if n:
            with self._staged((fwd, bwd), (occ, err)) as (d_fwd, d_bwd, d_occ, d_err):
                self.fb_check_device(d_fwd, d_bwd, W, H * W, 2 * H * W, n, alpha1, alpha2, d_occ, W, H * W, d_err, W, H * W)
        return (occ, err) if want_err else occ

    # -- the backward warp of 8-bit images by a flow, its valid mask and photometric statistics (dfx_warp_device) ----
    def warp_device(self, d_src_ptr: int, channels: int, layout: int, src_pitch: int, src_plane_stride: int,
                    src_image_stride: int, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int,
                    flow_stride_floats: int, n: int, border: int = 0, out_dtype: int = WARP_U8,
                    d_out_ptr: int | None = None, out_pitch: int = 0, out_plane_stride: int = 0, out_image_stride: int = 0,
                    d_ref_ptr: int | None = None, d_occ_ptr: int | None = None, occ_pitch: int = 0, occ_stride: int = 0,
                    d_valid_ptr: int | None = None, valid_pitch: int = 0, valid_stride: int = 0,
                    d_stats_ptr: int | None = None):
        """n 8-bit images that are already in device memory, sampled at the positions n planar float32 flows name: the fields
        of dfx_warp_desc (include/dfx.h) as arguments, codes and raw pointers as the header gives them."""
        d = DfxWarpDesc(d_src_ptr, int(channels), int(layout), src_pitch, src_plane_stride, src_image_stride, d_ref_ptr,
                        d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), int(border),
                        int(out_dtype), d_out_ptr, out_pitch, out_plane_stride, out_image_stride, d_occ_ptr, occ_pitch,
                        occ_stride, d_valid_ptr, valid_pitch, valid_stride, d_stats_ptr)
        self._check(self._L.dfx_warp_device(self._h, C.byref(d)))

    def _warp_images(self, images, layout_code, what="images"):
        """A uint8 array of images as the warp takes it: (array, channels).  (n, H, W), (n, H, W, 3) or — channels first —
        (n, 3, H, W)."""
        a = np.asarray(images)
        H, W = self.height, self.width
        if a.dtype != np.uint8:
            raise ValueError(f"{what} must be uint8")
        if a.ndim == 3 and a.shape[1:] == (H, W):
            return np.ascontiguousarray(a), 1
        if a.ndim == 4 and a.shape[1:] == ((3, H, W) if layout_code else (H, W, 3)):
            return np.ascontiguousarray(a), 3
        raise ValueError(f"{what} must be (n, H, W), (n, H, W, 3) or, with layout=\"chw\", (n, 3, H, W)")

    def _warp_flows(self, flows, n):
        return _np_flows(flows, self.height, self.width, lead="n", n=n, tail=", one flow per image")

    def warp(self, images, flows, border: str = "zero", dtype=np.uint8, layout: str = "hwc", ref=None, occ=None,
             want_valid: bool = False, want_stats: bool = False):
        """Image i sampled bilinearly at p + flows[i](p) (dfx_warp_device): the warped images in the images' shape, as
        np.uint8 (rounded to nearest even), np.float32, np.float16 or "bfloat16" (np.uint16 bit patterns).

        images: uint8, (n, H, W), (n, H, W, 3) or, with layout="chw", (n, 3, H, W).  flows: (n, 2, H, W) float32.
        border "zero": 0 where the target leaves the frame; "clamp": the sample at the nearest edge position.
        occ: optional (n, H, W) uint8 occlusion masks (0 = visible) as fb_check gives them.  ref: optional images of the
        same shape the warp is compared with.  want_valid: also return the (n, H, W) uint8 mask of the pixels whose target
        stays in the frame (and is not occluded); want_stats (needs ref): also return the (n, 2) uint64 {count, sad} over
        those pixels, sad the sum over channels of |ref - round(warp)|.  Returns out, or (out[, valid][, stats])."""
        code, np_dt = _warp_dtype(dtype)
        b, l = _warp_border(border), _warp_layout(layout)
        img, ch = self._warp_images(images, l)
        n = img.shape[0]
        H, W = self.height, self.width
        fl = self._warp_flows(flows, n)
        if want_stats and ref is None:
            raise ValueError("want_stats needs ref")
        if ref is not None:
            ref, _ = self._warp_images(ref, l, "ref")
            if ref.shape != img.shape:
                raise ValueError("ref must have the shape of images")
        occ = _np_planes(occ, n, H, W, np.uint8, "occ", "n")
        out = np.empty(img.shape, np_dt)
        valid = np.empty((n, H, W), np.uint8) if want_valid else None
        stats = np.zeros((n, 2), np.uint64) if want_stats else None
        if n:
            planes = ch == 3 and l == 1
            pitch = W * (1 if ch == 1 or planes else 3)
            plane = H * W if planes else 0
            image = ch * H * W
            with self._staged((img, fl, ref, occ), (out, valid, stats)) as (d_img, d_fl, d_ref, d_occ, d_out, d_valid, d_stats):
                self.warp_device(d_img, ch, l if ch == 3 else 0, pitch, plane, image, d_fl, W, H * W, 2 * H * W, n, b, code,
                                 d_out, pitch, plane, image, d_ref, d_occ, W, H * W, d_valid, W, H * W, d_stats)
        res = (out,) + ((valid,) if want_valid else ()) + ((stats,) if want_stats else ())
        return res if len(res) > 1 else out

    def warp_error(self, frames, flows, step: int, occ=None):
        """The photometric error of the flows of a FlowBuffer: flow i of `step` is a -> b (for step > 0 frames i -> i + step,
        for step < 0 frames i - step -> i: the pair rule of calc_optflows), frame b is warped back by it and compared with
        frame a.  Returns the float64 array of the M = max(N - |step|, 0) mean absolute errors in grey levels, sad / (count *
        channels) over the pixels whose target stays in the frame (and, with occ — (M, H, W) uint8, 0 = visible — is not
        occluded); NaN where no pixel counts.  frames: N uint8 frames (H, W) or (H, W, 3); flows: (M, 2, H, W) float32.
        Only the statistics are computed on the device (no warped image is stored)."""
        step = int(step)
        if step == 0:
            raise ValueError("step must not be 0")
        H, W = self.height, self.width
        fr = np.asarray(frames)
        if fr.dtype != np.uint8 or fr.ndim not in (3, 4) or fr.shape[1:3] != (H, W) or (fr.ndim == 4 and fr.shape[3] != 3):
            raise ValueError("frames must be N uint8 frames of (H, W) or (H, W, 3)")
        fr = np.ascontiguousarray(fr)
        ch = 1 if fr.ndim == 3 else 3
        m = max(fr.shape[0] - abs(step), 0)
        fl = self._warp_flows(flows, m)
        occ = _np_planes(occ, m, H, W, np.uint8, "occ")
        stats = np.zeros((m, 2), np.uint64)
        if m:
            fb = ch * H * W
            with self._staged((fr, fl, occ), (stats,)) as (d_fr, d_fl, d_occ, d_stats):
                first_a, first_b = (0, step) if step > 0 else (-step, 0)  # flow 0 is frame first_a -> frame first_b
                self.warp_device(d_fr.value + first_b * fb, ch, 0, W * ch, 0, fb, d_fl, W, H * W, 2 * H * W, m,
                                 d_ref_ptr=d_fr.value + first_a * fb, d_occ_ptr=d_occ, occ_pitch=W, occ_stride=H * W,
                                 d_stats_ptr=d_stats)
        cnt, sad = stats[:, 0].astype(np.float64), stats[:, 1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(cnt > 0, sad / (cnt * ch), np.nan)

    def _warp_tensor_images(self, t, layout, what):
        """A torch uint8 / output tensor of images as the warp takes it, read from its shape and strides: (channels, layout
        code of how it lies in MEMORY, row pitch, plane stride, image stride, whether the SHAPE is channels-first), strides in
        elements.  The shape is (n, H, W), (n, 3, H, W) or (n, H, W, 3); memory may be interleaved or planar under either shape
        (a permuted view is read where it lies)."""
        H, W = self.height, self.width
        n = t.shape[0] if t.dim() else 0
        st = t.stride()
        if t.dim() == 3 and tuple(t.shape[1:]) == (H, W):
            pitch, image = _plane_geometry(t, n, H, W, t.dtype, what, noun="images")
            return 1, 0, pitch, 0, image, False
        chw, hwc = tuple(t.shape[1:]) == (3, H, W), tuple(t.shape[1:]) == (H, W, 3)
        if t.dim() != 4 or not (chw or hwc):
            raise ValueError(f"{what} must be (n, H, W), (n, 3, H, W) or (n, H, W, 3)")
        if chw and hwc:  # H = W = 3: the shape does not say
            if layout is None:
                raise ValueError(f'{what}: H = W = 3, say layout="chw" or "hwc"')
            chw = _warp_layout(layout) == 1
        sc, sy, sx = (st[1], st[2], st[3]) if chw else (st[3], st[1], st[2])  # strides of channel, row, pixel
        if sc == 1 and (sx == 3 or W == 1):  # interleaved pixels
            pitch = sy if H > 1 else 3 * W
            image = st[0] if n > 1 else H * pitch
            if pitch < 3 * W or image < H * pitch:
                raise ValueError(f"{what}: rows and images must not overlap")
            return 3, 0, pitch, 0, image, chw
        if sx == 1 or W == 1:  # three planes
            pitch = sy if H > 1 else W
            plane = sc
            image = st[0] if n > 1 else 3 * plane
            if pitch < W or plane < H * pitch or image < 3 * plane:
                raise ValueError(f"{what}: rows, planes and images must not overlap")
            return 3, 1, pitch, plane, image, chw
        raise ValueError(f"{what}: pixels must be interleaved (channel stride 1, pixel stride 3) or planar (pixel stride 1)")

    def warp_tensor(self, images, flows, border: str = "zero", dtype=None, layout: str | None = None, ref=None, occ=None,
                    want_valid: bool = False, want_stats: bool = False, out=None):
        """warp for torch tensors on this handle's device, read and written where they lie.

        images: torch.uint8, (n, H, W), (n, 3, H, W) or (n, H, W, 3); the memory layout — interleaved or three planes — and
        every stride are taken from the tensor, so the NCHW view of an NHWC batch or a slice of a larger tensor is read
        without a copy (layout is needed only for H = W = 3, where the shape does not say which it is).  flows: (n, 2, H, W)
        torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns.  dtype: torch.uint8 (default),
        torch.float32, torch.float16 or torch.bfloat16.  out: optional tensor of that dtype and the images' shape whose
        memory layout is the images' (interleaved or planar); otherwise the result is allocated in the images' memory
        layout and returned in the images' shape.  ref: optional uint8 tensor of the images' shape (copied only if its
        strides differ from the images'); occ: optional (n, H, W) uint8 masks (0 = visible).  want_valid / want_stats as
        warp: valid is an (n, H, W) uint8 tensor, stats an (n, 2) torch.int64 tensor {count, sad}.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong dtype, device, shape or stride."""
        import torch

        codes = {torch.uint8: WARP_U8, torch.float32: PLANAR_F32, torch.float16: PLANAR_F16, torch.bfloat16: PLANAR_BF16}
        tdt = torch.uint8 if dtype is None else dtype
        if tdt not in codes:
            raise ValueError("dtype must be torch.uint8, torch.float32, torch.float16 or torch.bfloat16")
        b = _warp_border(border)
        if layout is not None:
            _warp_layout(layout)
        if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
            raise ValueError("images must be a torch.uint8 tensor")
        H, W = self.height, self.width
        ch, mem, pitch, plane, image, chw = self._warp_tensor_images(images, layout, "images")
        n = images.shape[0]
        dev = images.device
        row_pitch, flow_plane, flow_stride = _flow_geometry(flows, H, W, "flows", "n", n, ", one flow per image")
        if want_stats and ref is None:
            raise ValueError("want_stats needs ref")
        if ref is not None:
            if not isinstance(ref, torch.Tensor) or ref.dtype != torch.uint8 or ref.shape != images.shape:
                raise ValueError("ref must be a torch.uint8 tensor of the images' shape")
        occ_pitch = occ_stride = 0
        if occ is not None:
            occ_pitch, occ_stride = _plane_geometry(occ, n, H, W, torch.uint8, "occ", "n")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != tdt or out.shape != images.shape:
                raise ValueError(f"out must be a {tdt} tensor of the images' shape")
            och, omem, out_pitch, out_plane, out_image, _ = self._warp_tensor_images(out, layout, "out")
            if (och, omem) != (ch, mem):
                raise ValueError("out must lie in memory as the images do (interleaved or planar)")
        self._check_devices(images, "images must be on this handle's device", (flows, ref, occ, out),
                            "flows, ref, occ and out must be on the images' device")
        if out is None:
            if ch == 3 and mem == 0:  # interleaved memory, whatever the shape's order
                base = torch.empty((n, H, W, 3), dtype=tdt, device=dev)
                out = base.permute(0, 3, 1, 2) if chw else base
                out_pitch, out_plane, out_image = 3 * W, 0, 3 * H * W
            elif ch == 3:
                base = torch.empty((n, 3, H, W), dtype=tdt, device=dev)
                out = base if chw else base.permute(0, 2, 3, 1)
                out_pitch, out_plane, out_image = W, H * W, 3 * H * W
            else:
                out = torch.empty((n, H, W), dtype=tdt, device=dev)
                out_pitch, out_plane, out_image = W, 0, H * W
        if ref is not None and n and ref.stride() != images.stride():
            ref = torch.empty_strided(images.shape, images.stride(), dtype=torch.uint8, device=dev).copy_(ref)
        valid = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_valid else None
        stats = torch.zeros((n, 2), dtype=torch.int64, device=dev) if want_stats else None
        torch.cuda.current_stream(dev).synchronize()
        if n:
            self.warp_device(images.data_ptr(), ch, mem, pitch, plane, image, flows.data_ptr(), row_pitch, flow_plane,
                             flow_stride, n, b, codes[tdt], out.data_ptr(), out_pitch, out_plane, out_image,
                             ref.data_ptr() if ref is not None else None, occ.data_ptr() if occ is not None else None,
                             occ_pitch, occ_stride, valid.data_ptr() if want_valid else None, W, H * W,
                             stats.data_ptr() if want_stats else None)
        res = (out,) + ((valid,) if want_valid else ()) + ((stats,) if want_stats else ())
        return res if len(res) > 1 else out

    # -- the backward warp of float, half and label planes by a flow (dfx_warp_planes_device) ----
    def warp_planes_device(self, d_src_ptr: int, src_dtype: int, channels: int, layout: int, src_pitch: int,
                           src_plane_stride: int, src_image_stride: int, d_flow_ptr: int, row_pitch_floats: int,
                           plane_stride_floats: int, flow_stride_floats: int, n: int, border: int = 0, sample: int = 0,
                           invalid: int = 0, out_dtype: int = PLANAR_F32, d_out_ptr: int | None = None, out_pitch: int = 0,
                           out_plane_stride: int = 0, out_image_stride: int = 0, d_occ_ptr: int | None = None,
                           occ_pitch: int = 0, occ_stride: int = 0, d_valid_ptr: int | None = None, valid_pitch: int = 0,
                           valid_stride: int = 0):
        """n sources of `channels` planes that are already in device memory, sampled at the positions n planar float32 flows
        name: the fields of dfx_warp_planes_desc (include/dfx.h) as arguments, codes and raw pointers as the header gives
        them."""
        d = DfxWarpPlanesDesc(d_src_ptr, int(src_dtype), int(channels), int(layout), src_pitch, src_plane_stride,
                              src_image_stride, d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n),
                              int(border), int(sample), int(invalid), int(out_dtype), d_out_ptr, out_pitch, out_plane_stride,
                              out_image_stride, d_occ_ptr, occ_pitch, occ_stride, d_valid_ptr, valid_pitch, valid_stride)
        self._check(self._L.dfx_warp_planes_device(self._h, C.byref(d)))

    def warp_planes(self, planes, flows, sample: str = "bilinear", border: str = "zero", invalid: str = "zero", dtype=None,
                    layout: str = "chw", occ=None, return_valid: bool = False, out=None):
        """Source i sampled at p + flows[i](p) (dfx_warp_planes_device): labels, a depth plane, a soft mask or a feature map
        of frame 1 at the pixels of frame 0.

        planes: (n, C, H, W), or with layout="hwc" (n, H, W, C).  sample "bilinear": float32, float16 or uint16 holding
        bfloat16 bit patterns; the result is np.float32, np.float16 or "bfloat16" (np.uint16 bit patterns) as dtype says
        (None: as the source).  sample "nearest": any 1-, 2- or 4-byte integer or float dtype, the element at the rounded
        position (ties to even) copied as a bit pattern; the result has the source's dtype.  flows: (n, 2, H, W) float32.
        border "zero" / "clamp" as warp.  occ: optional (n, H, W) uint8 occlusion masks (0 = visible).  invalid "zero": every
        pixel is written, zero bits where the target leaves the frame; "keep": only the pixels whose target stays in the
        frame (and is not occluded) are written and the others of `out` — required then, a contiguous array of the result's
        shape and dtype — stay as they are (a background, an ignore index, an earlier warp).  return_valid: also return the
        (n, H, W) uint8 mask of those pixels.  Returns out, or (out, valid)."""
        smp, b, inv = _warp_planes_settings(sample, border, invalid)
        l = _warp_layout(layout)
        a = np.asarray(planes)
        H, W = self.height, self.width
        if a.ndim != 4 or (a.shape[2:] != (H, W) if l else a.shape[1:3] != (H, W)) or a.shape[1 if l else 3] < 1:
            raise ValueError('planes must be (n, C, H, W) or, with layout="hwc", (n, H, W, C)')
        src_code, out_code, np_dt = _warp_planes_np_dtypes(a.dtype, smp, dtype)
        a = np.ascontiguousarray(a)
        n, ch = a.shape[0], a.shape[1 if l else 3]
        fl = self._warp_flows(flows, n)
        occ = _np_planes(occ, n, H, W, np.uint8, "occ", "n")
        if out is not None:
            if not isinstance(out, np.ndarray) or out.dtype != np_dt or out.shape != a.shape or not out.flags.c_contiguous:
                raise ValueError(f"out must be a contiguous {np_dt.name} array of the planes' shape")
        elif inv:
            raise ValueError('invalid="keep" needs out: the array whose other pixels are kept')
        else:
            out = np.empty(a.shape, np_dt)
        valid = np.empty((n, H, W), np.uint8) if return_valid else None
        if n:
            pitch = W if l else W * ch
            plane = H * W if l and ch > 1 else 0
            image = ch * H * W
            keep_in, fresh = (out, None) if inv else (None, out)  # a kept output goes up first and comes back by hand
            with self._staged((a, fl, occ, keep_in), (fresh, valid)) as (d_src, d_fl, d_occ, d_keep, d_fresh, d_valid):
                d_out = d_keep if inv else d_fresh
                self.warp_planes_device(d_src, src_code, ch, l, pitch, plane, image, d_fl, W, H * W, 2 * H * W, n, b, smp, inv,
                                        out_code, d_out, pitch, plane, image, d_occ, W, H * W, d_valid, W, H * W)
                if inv:
                    self._check(self._L.dfx_memcpy_d2h(self._h, out.ctypes.data, d_out, out.nbytes))
        return (out, valid) if return_valid else out

    def _planes_tensor_geometry(self, t, chw, what):
        """A torch tensor of planes as the warp takes it, read from its shape — (n, C, H, W), or (n, H, W, C) where not chw —
        and its strides: (channels, layout code of how it lies in MEMORY, row pitch, plane stride, image stride), in
        elements.  Memory may be channels-last or channels-first under either shape (a permuted view is read where it lies)."""
        H, W = self.height, self.width
        if t.dim() != 4 or tuple(t.shape[2:] if chw else t.shape[1:3]) != (H, W) or t.shape[1 if chw else 3] < 1:
            raise ValueError(f'{what} must be (n, C, H, W) or, with layout="hwc", (n, H, W, C)')
        n, ch = t.shape[0], t.shape[1 if chw else 3]
        st = t.stride()
        sc, sy, sx = (st[1], st[2], st[3]) if chw else (st[3], st[1], st[2])  # strides of channel, row, pixel
        if (sx == 1 or W == 1) and (ch == 1 or sc != 1 or (H == 1 and W == 1)):  # channels-first memory: C planes
            pitch = sy if H > 1 else W
            plane = sc if ch > 1 else H * pitch
            image = st[0] if n > 1 else ch * plane
            if pitch < W or plane < H * pitch or image < ch * plane:
                raise ValueError(f"{what}: rows, planes and images must not overlap")
            return ch, 1, pitch, (plane if ch > 1 else 0), image
        if (sc == 1 or ch == 1) and (sx == ch or W == 1):  # channels-last memory: C elements per pixel
            pitch = sy if H > 1 else ch * W
            image = st[0] if n > 1 else H * pitch
            if pitch < ch * W or image < H * pitch:
                raise ValueError(f"{what}: rows and images must not overlap")
            return ch, 0, pitch, 0, image
        raise ValueError(f"{what}: pixels must be channels-last (channel stride 1, pixel stride C) or channels-first (pixel stride 1)")

    def warp_planes_tensor(self, planes, flows, sample: str = "bilinear", border: str = "zero", invalid: str = "zero",
                           dtype=None, layout: str = "chw", occ=None, return_valid: bool = False, out=None):
        """warp_planes for torch tensors on this handle's device, read and written where they lie.

        planes: (n, C, H, W), or with layout="hwc" (n, H, W, C); torch.float32, torch.float16 or torch.bfloat16, and for
        sample="nearest" also torch.uint8, torch.int16 or torch.int32 (label maps, copied as bit patterns).  The memory
        layout — channels-first or channels-last — and every stride are taken from the tensor, so a channels_last tensor,
        the NCHW view of an NHWC batch or a slice of a larger tensor is read without a copy.  flows: (n, 2, H, W)
        torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns.  dtype: the result's, for
        bilinear any of the three float types whatever the source is (None: the source's); for nearest the source's.  out:
        optional tensor of that dtype and the planes' shape that lies in memory as the planes do, not `planes` itself;
        required for invalid="keep", whose other pixels it keeps; otherwise the result is allocated in the planes' memory
        layout and returned in the planes' shape.  occ: optional (n, H, W) uint8 masks (0 = visible).  return_valid: also
        return the (n, H, W) uint8 tensor of the pixels whose target stays in the frame (and is not occluded).

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        smp, b, inv = _warp_planes_settings(sample, border, invalid)
        chw = _warp_layout(layout) == 1
        codes = {torch.float32: PLANAR_F32, torch.float16: PLANAR_F16, torch.bfloat16: PLANAR_BF16}
        if smp:
            codes.update({torch.uint8: WARP_U8, torch.int16: PLANAR_F16, torch.int32: PLANAR_F32})
        if not isinstance(planes, torch.Tensor) or planes.dtype not in codes:
            raise ValueError("planes must be a torch.float32, torch.float16 or torch.bfloat16 tensor" +
                             (", or torch.uint8, torch.int16 or torch.int32" if smp else
                              ' (torch.uint8, torch.int16 and torch.int32 take sample="nearest")'))
        tdt = planes.dtype if dtype is None else dtype
        if smp and tdt != planes.dtype:
            raise ValueError('sample="nearest" copies elements: dtype must be None or the planes\' dtype')
        if tdt not in codes:
            raise ValueError("dtype must be torch.float32, torch.float16 or torch.bfloat16")
        H, W = self.height, self.width
        ch, mem, pitch, plane, image = self._planes_tensor_geometry(planes, chw, "planes")
        n, dev = planes.shape[0], planes.device
        fgeom = _flow_geometry(flows, H, W, "flows", "n", n, ", one flow per image")
        ogeom = (0, 0)
        if occ is not None:
            ogeom = _plane_geometry(occ, n, H, W, torch.uint8, "occ", "n")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != tdt or out.shape != planes.shape:
                raise ValueError(f"out must be a {tdt} tensor of the planes' shape")
            och, omem, out_pitch, out_plane, out_image = self._planes_tensor_geometry(out, chw, "out")
            if omem != mem and ch > 1:
                raise ValueError("out must lie in memory as the planes do (channels-last or channels-first)")
            if omem != mem:  # one channel: the two layouts name the same memory
                out_pitch, out_plane, out_image = (out_pitch, 0, out_image)
            if out.data_ptr() == planes.data_ptr() and n:
                raise ValueError("out must not be planes: a warp cannot run in place")
        elif inv:
            raise ValueError('invalid="keep" needs out: the tensor whose other pixels are kept')
        self._check_devices(planes, "planes must be on this handle's device", (flows, occ, out),
                            "flows, occ and out must be on the planes' device")
        if out is None:
            if mem == 0:  # channels-last memory, whatever the shape's order
                base = torch.empty((n, H, W, ch), dtype=tdt, device=dev)
                out = base.permute(0, 3, 1, 2) if chw else base
                out_pitch, out_plane, out_image = ch * W, 0, ch * H * W
            else:
                base = torch.empty((n, ch, H, W), dtype=tdt, device=dev)
                out = base if chw else base.permute(0, 2, 3, 1)
                out_pitch, out_plane, out_image = W, (H * W if ch > 1 else 0), ch * H * W
        valid = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if return_valid else None
        torch.cuda.current_stream(dev).synchronize()
        if n:
            self.warp_planes_device(planes.data_ptr(), codes[planes.dtype], ch, mem, pitch, plane, image, flows.data_ptr(),
                                    *fgeom, n, b, smp, inv, codes[tdt], out.data_ptr(), out_pitch, out_plane, out_image,
                                    occ.data_ptr() if occ is not None else None, ogeom[0], ogeom[1],
                                    valid.data_ptr() if return_valid else None, W, H * W)
        return (out, valid) if return_valid else out

    # -- the global (camera) motion of a flow: robust fit, removal, moving mask (dfx_global_motion_device) ----
    def global_motion_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                             n: int, d_result_ptr: int, model: int = 1, rounds: int = 5, thr: float = 0.5, growth: float = 2.0,
                             d_mask_ptr: int | None = None, mask_pitch: int = 0, mask_stride: int = 0,
                             d_out_ptr: int | None = None, out_row_pitch_floats: int = 0, out_plane_stride_floats: int = 0,
                             out_flow_stride_floats: int = 0, d_moving_ptr: int | None = None, moving_pitch: int = 0,
                             moving_stride: int = 0):
        """n planar float32 flows that are already in device memory: the fields of dfx_gm_desc (include/dfx.h) as arguments,
        codes and raw pointers as the header gives them; d_result_ptr: n dfx_gm_result records (DfxGmResult) in device memory."""
        d = DfxGmDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), int(model), int(rounds),
                      float(thr), float(growth), d_mask_ptr, mask_pitch, mask_stride, d_out_ptr, out_row_pitch_floats,
                      out_plane_stride_floats, out_flow_stride_floats, d_moving_ptr, moving_pitch, moving_stride, d_result_ptr)
        self._check(self._L.dfx_global_motion_device(self._h, C.byref(d)))

    def global_motion(self, flows, mask=None, model: str = "affine", rounds: int = 5, thr: float = 0.5, growth: float = 2.0):
        """How much of each flow is the camera, and what the flow is without it (dfx_global_motion_device).

        flows: (M, 2, H, W) float32.  mask: optional (M, H, W) uint8, nonzero = excluded from the fit (an occlusion mask as
        fb_check gives it).  model "translation" or "affine"; rounds 1 .. 8 of re-fitting on the pixels within the previous
        model (1 = plain least squares); thr: the inlier radius of the last round in pixels, each earlier round's `growth`
        times wider.  Returns (params, compensated, moving, info): params (M, 6) float64 with u_cam = a0 + a1 x + a2 y,
        v_cam = a3 + a4 x + a5 y in pixel coordinates; compensated (M, 2, H, W) float32, the flows minus that model;
        moving (M, H, W) uint8, 1 where a pixel does not follow the model within thr (or is excluded); info: a dict of
        "valid" (M,), "inliers" (M, 8), "status" (M,: bit k set = round k was degenerate and kept the model before it) and
        "rounds"."""
        code, rounds, thr, growth = _gm_settings(model, rounds, thr, growth)
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W)
        m = fl.shape[0]
        mask = _np_planes(mask, m, H, W, np.uint8, "mask")
        out, moving = np.empty_like(fl), np.empty((m, H, W), np.uint8)
        rec = np.zeros(m, GM_RESULT_DTYPE)
        if m:
            with self._staged((fl, mask), (out, moving, rec)) as (d_fl, d_mask, d_out, d_moving, d_rec):
                self.global_motion_device(d_fl, W, H * W, 2 * H * W, m, d_rec, code, rounds, thr, growth, d_mask, W, H * W,
                                          d_out, W, H * W, 2 * H * W, d_moving, W, H * W)
        return rec["a"].copy(), out, moving, _gm_info(rec)

    def global_motion_tensor(self, flows, mask=None, model: str = "affine", rounds: int = 5, thr: float = 0.5,
                             growth: float = 2.0, out=None, want_moving: bool = True):
        """global_motion for torch tensors on this handle's device, read and written where they lie.

        flows: (M, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  mask: optional (M, H, W) torch.uint8.
        out: optional (M, 2, H, W) float32 tensor for the compensated flows; it may be `flows` itself (in place).  Returns
        (params, compensated, moving, info): params an (M, 6) float64 tensor, moving an (M, H, W) uint8 tensor (None with
        want_moving=False), info a dict of host tensors "valid", "inliers", "status", "rounds" as global_motion's
        (the n records are copied to the host once; the counts are int64).

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        code, rounds, thr, growth = _gm_settings(model, rounds, thr, growth)
        H, W = self.height, self.width
        row_pitch, flow_plane, flow_stride = _flow_geometry(flows, H, W, "flows")
        m, dev = flows.shape[0], flows.device
        mask_pitch = mask_stride = 0
        if mask is not None:
            mask_pitch, mask_stride = _plane_geometry(mask, m, H, W, torch.uint8, "mask")
        if out is not None:
            out_pitch, out_plane, out_stride = _flow_geometry(out, H, W, "out")
            if out.shape[0] != m:
                raise ValueError("out must be an (M, 2, H, W) torch.float32 tensor")
            if out.data_ptr() == flows.data_ptr() and (out_pitch, out_plane, out_stride) != (row_pitch, flow_plane, flow_stride):
                raise ValueError("out: in place needs the strides of flows")
        self._check_devices(flows, "flows must be on this handle's device", (mask, out), "mask and out must be on the flows' device")
        if out is None:
            out = torch.empty((m, 2, H, W), dtype=torch.float32, device=dev)
            out_pitch, out_plane, out_stride = W, H * W, 2 * H * W
        moving = torch.empty((m, H, W), dtype=torch.uint8, device=dev) if want_moving else None
        rec = torch.zeros((m, C.sizeof(DfxGmResult) // 8), dtype=torch.int64, device=dev)  # 8-byte aligned records
        torch.cuda.current_stream(dev).synchronize()
        if m:
            self.global_motion_device(flows.data_ptr(), row_pitch, flow_plane, flow_stride, m, rec.data_ptr(), code, rounds, thr,
                                      growth, mask.data_ptr() if mask is not None else None, mask_pitch, mask_stride,
                                      out.data_ptr(), out_pitch, out_plane, out_stride,
                                      moving.data_ptr() if want_moving else None, W, H * W)
        host = rec.cpu().numpy().view(np.uint8).reshape(m, -1).copy().view(GM_RESULT_DTYPE).reshape(m)
        info = {k: torch.from_numpy(v.astype(np.int64) if v.dtype.kind == "u" else v) for k, v in _gm_info(host).items()}
        return torch.from_numpy(host["a"].copy()).to(dev), out, moving, info

    # -- median filter and occlusion fill of flows, mask-aware (dfx_flow_median_device) ----
    def flow_median_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                           n: int, d_out_ptr: int, out_row_pitch_floats: int, out_plane_stride_floats: int,
                           out_flow_stride_floats: int, ksize: int = 5, mode: int = 0, d_mask_ptr: int | None = None,
                           mask_pitch: int = 0, mask_stride: int = 0, d_mask_out_ptr: int | None = None,
                           mask_out_pitch: int = 0, mask_out_stride: int = 0):
        """n planar float32 flows that are already in device memory: the fields of dfx_median_desc (include/dfx.h) as
        arguments, codes and raw pointers as the header gives them."""
        d = DfxMedianDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), int(ksize), int(mode),
                          d_mask_ptr, mask_pitch, mask_stride, d_out_ptr, out_row_pitch_floats, out_plane_stride_floats,
                          out_flow_stride_floats, d_mask_out_ptr, mask_out_pitch, mask_out_stride)
        self._check(self._L.dfx_flow_median_device(self._h, C.byref(d)))

    def flow_median(self, flows, ksize: int = 5, mask=None, mode: str = "all", passes: int = 1):
        """The ksize x ksize median of each flow plane on the keys of the samples' bit patterns, mask-aware
        (dfx_flow_median_device).

        flows: (M, 2, H, W) float32.  mask: optional (M, H, W) uint8, nonzero = the sample is not used (an occlusion mask as
        fb_check gives it).  mode "all": every pixel takes the median of the unmasked samples of its window; "fill" (needs a
        mask): only masked pixels do, unmasked flow is returned bit for bit.  passes > 1 repeats the call on its own output
        with the returned mask as the mask, which grows a fill inward by ksize // 2 pixels per pass; in "fill" mode the passes
        stop once the returned mask is all zero.  Returns (out, mask_out): (M, 2, H, W) float32 and (M, H, W) uint8 with 1
        where a pixel had no unmasked sample in its window (it keeps its input), None without a mask."""
        ksize, code, passes = _median_settings(ksize, mode, passes, mask is not None)
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W)
        m = fl.shape[0]
        mask = _np_planes(mask, m, H, W, np.uint8, "mask")
        out = np.empty_like(fl)
        mask_out = np.empty((m, H, W), np.uint8) if mask is not None else None
        if m:
            # the passes alternate between two flow buffers and two mask buffers, so the results are fetched by hand from
            # whichever the last pass wrote
            spare = [fl.nbytes, mask.nbytes if mask is not None else 0]
            with self._staged((fl, mask), (), spare) as (src, msrc, dst, mdst):
                if mask is None:
                    mdst = None  # (no mask planes either way)
                for k in range(passes):
                    self.flow_median_device(src, W, H * W, 2 * H * W, m, dst, W, H * W, 2 * H * W, ksize, code, msrc, W, H * W,
                                            mdst, W, H * W)
                    src, dst, msrc, mdst = dst, src, mdst, msrc
                    if mask is not None and code == MEDIAN_MODES["fill"] and k + 1 < passes:
                        self._check(self._L.dfx_memcpy_d2h(self._h, mask_out.ctypes.data, msrc, mask.nbytes))
                        if not mask_out.any():
                            break
                self._check(self._L.dfx_memcpy_d2h(self._h, out.ctypes.data, src, out.nbytes))
                if mask is not None:
                    self._check(self._L.dfx_memcpy_d2h(self._h, mask_out.ctypes.data, msrc, mask.nbytes))
        return out, mask_out

    def flow_median_tensor(self, flows, ksize: int = 5, mask=None, mode: str = "all", passes: int = 1, out=None):
        """flow_median for torch tensors on this handle's device, read and written where they lie.

        flows: (M, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  mask: optional (M, H, W) torch.uint8.
        out: optional (M, 2, H, W) float32 tensor for the result, not `flows` itself (a stencil cannot run in place).  Returns
        (out, mask_out): mask_out an (M, H, W) uint8 tensor, None without a mask.  passes > 1 alternates between `out` and
        one temporary torch allocation (and two mask tensors); the result is copied into `out` where the last pass did not
        write it there.  In "fill" mode the passes stop once a returned mask is all zero (one host read per pass).

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        ksize, code, passes = _median_settings(ksize, mode, passes, mask is not None)
        H, W = self.height, self.width
        geom = _flow_geometry(flows, H, W, "flows")
        m, dev = flows.shape[0], flows.device
        mgeom = _plane_geometry(mask, m, H, W, torch.uint8, "mask") if mask is not None else (0, 0)
        if out is not None:
            ogeom = _flow_geometry(out, H, W, "out")
            if out.shape[0] != m:
                raise ValueError("out must be an (M, 2, H, W) torch.float32 tensor")
            if out.data_ptr() == flows.data_ptr() and m:
                raise ValueError("out must not be flows: a stencil cannot run in place")
        self._check_devices(flows, "flows must be on this handle's device", (mask, out), "mask and out must be on the flows' device")
        dense, mdense = (W, H * W, 2 * H * W), (W, H * W)
        if out is None:
            out = torch.empty((m, 2, H, W), dtype=torch.float32, device=dev)
            ogeom = dense
        torch.cuda.current_stream(dev).synchronize()
        if not m:
            return out, (torch.empty((0, H, W), dtype=torch.uint8, device=dev) if mask is not None else None)
        src, sgeom, msrc, msgeom = flows, geom, mask, mgeom
        tmp = None
        masks = [torch.empty((m, H, W), dtype=torch.uint8, device=dev) for _ in range(min(passes, 2))] if mask is not None else []
        for k in range(passes):
            if k % 2 == 0:
                dst, dgeom = out, ogeom
            else:
                if tmp is None:
                    tmp = torch.empty((m, 2, H, W), dtype=torch.float32, device=dev)
                dst, dgeom = tmp, dense
            mdst = masks[k % 2] if mask is not None else None
            self.flow_median_device(src.data_ptr(), *sgeom, m, dst.data_ptr(), *dgeom, ksize, code,
                                    msrc.data_ptr() if mask is not None else None, *msgeom,
                                    mdst.data_ptr() if mask is not None else None, *mdense)
            src, sgeom, msrc, msgeom = dst, dgeom, mdst, mdense
            if mask is not None and code == MEDIAN_MODES["fill"] and k + 1 < passes and not bool(mdst.any()):
                break
        if src is not out:
            out.copy_(src)
            torch.cuda.current_stream(dev).synchronize()
        return out, msrc if mask is not None else None

    # -- adjacent flows chained into long-range flows and dense trajectories (dfx_flow_chain_device) ----
    def flow_chain_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                          n: int, d_out_ptr: int, out_row_pitch_floats: int, out_plane_stride_floats: int,
                          out_flow_stride_floats: int, length: int, first: int = 0, hop: int = 1, anchors: int = 1,
                          anchor_step: int = 1, emit: int = 0, border: int = 0, d_occ_ptr: int | None = None,
                          occ_pitch: int = 0, occ_stride: int = 0, d_valid_ptr: int | None = None, valid_pitch: int = 0,
                          valid_stride: int = 0):
        """n planar float32 flows that are already in device memory: the fields of dfx_chain_desc (include/dfx.h) as
        arguments, codes and raw pointers as the header gives them."""
        d = DfxChainDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), int(first), int(hop),
                         int(length), int(anchors), int(anchor_step), int(emit), int(border), d_occ_ptr, occ_pitch, occ_stride,
                         d_out_ptr, out_row_pitch_floats, out_plane_stride_floats, out_flow_stride_floats, d_valid_ptr,
                         valid_pitch, valid_stride)
        self._check(self._L.dfx_flow_chain_device(self._h, C.byref(d)))

    def flow_chain(self, flows, length: int, first: int = 0, hop: int = 1, anchors: int | None = None, anchor_step: int = 1,
                   emit: str = "last", border: str = "zero", occ=None):
        """Adjacent flows composed into long-range flows: A_0 = 0, A_{k+1}(p) = A_k(p) + F_k(p + A_k(p)), bilinear samples
        (dfx_flow_chain_device).

        flows: (N, 2, H, W) float32, flows of adjacent frames.  Link k of anchor j reads flow first + j * anchor_step + k * hop
        (hop -1 walks a list of backward flows down the clip); anchors None: as many chains as fit.  emit "last": the flow over
        all `length` links per anchor; "all": the flow after every link, anchor by anchor (p + A_k(p) is the trajectory of pixel
        p).  border "zero": a chain that leaves the frame is frozen; "clamp": it goes on from the nearest edge position.  occ:
        optional (N, H, W) uint8 masks, one per flow, nonzero = occluded (as fb_check gives them).  Returns (out, valid):
        (m * E, 2, H, W) float32 and (m * E, H, W) uint8, E = length for "all" and 1 otherwise; valid is 1 where every link so
        far was sampled inside the frame from unoccluded taps."""
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W, lead="N")
        n = fl.shape[0]
        length, first, hop, m, anchor_step, ecode, bcode = _chain_settings(n, length, first, hop, anchors, anchor_step, emit, border)
        occ = _np_planes(occ, n, H, W, np.uint8, "occ", "N")
        e = length if ecode else 1
        out = np.empty((m * e, 2, H, W), np.float32)
        valid = np.empty((m * e, H, W), np.uint8)
        if m:
            with self._staged((fl, occ), (out, valid)) as (src, docc, dst, dval):
                self.flow_chain_device(src, W, H * W, 2 * H * W, n, dst, W, H * W, 2 * H * W, length, first, hop, m, anchor_step,
                                       ecode, bcode, docc, W, H * W, dval, W, H * W)
        return out, valid

    def flow_chain_tensor(self, flows, length: int, first: int = 0, hop: int = 1, anchors: int | None = None,
                          anchor_step: int = 1, emit: str = "last", border: str = "zero", occ=None, out=None):
        """flow_chain for torch tensors on this handle's device, read and written where they lie.

        flows: (N, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  occ: optional (N, H, W) torch.uint8.
        out: optional (m * E, 2, H, W) float32 tensor for the result, not `flows` itself.  Returns (out, valid): valid an
        (m * E, H, W) uint8 tensor.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        H, W = self.height, self.width
        geom = _flow_geometry(flows, H, W, "flows", "N")
        n, dev = flows.shape[0], flows.device
        length, first, hop, m, anchor_step, ecode, bcode = _chain_settings(n, length, first, hop, anchors, anchor_step, emit, border)
        e = length if ecode else 1
        ogeom_occ = _plane_geometry(occ, n, H, W, torch.uint8, "occ", "N") if occ is not None else (0, 0)
        if out is not None:
            ogeom = _flow_geometry(out, H, W, "out", "N")
            if out.shape[0] != m * e:
                raise ValueError("out must be an (m * E, 2, H, W) torch.float32 tensor")
            if out.data_ptr() == flows.data_ptr() and m and n:
                raise ValueError("out must not be flows: a chain cannot run in place")
        self._check_devices(flows, "flows must be on this handle's device", (occ, out), "occ and out must be on the flows' device")
        if out is None:
            out = torch.empty((m * e, 2, H, W), dtype=torch.float32, device=dev)
            ogeom = (W, H * W, 2 * H * W)
        valid = torch.empty((m * e, H, W), dtype=torch.uint8, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if m:
            self.flow_chain_device(flows.data_ptr(), *geom, n, out.data_ptr(), *ogeom, length, first, hop, m, anchor_step, ecode,
                                   bcode, occ.data_ptr() if occ is not None else None, *ogeom_occ, valid.data_ptr(), W, H * W)
        return out, valid

    # -- forward projection of flows: inverse and time-t flows, holes marked (dfx_flow_project_device) ----
    def flow_project_work_bytes(self) -> int:
        """The bytes of workspace one flow of this handle's size needs (dfx_flow_project_work_bytes)."""
        return int(self._L.dfx_flow_project_work_bytes(self._h))

    def flow_project_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                            n: int, d_work_ptr: int, work_bytes: int, t: float = 1.0, scale: float = -1.0,
                            min_weight: float = 0.25, d_out_ptr: int | None = None, out_row_pitch_floats: int = 0,
                            out_plane_stride_floats: int = 0, out_flow_stride_floats: int = 0, d_hole_ptr: int | None = None,
                            hole_pitch: int = 0, hole_stride: int = 0, d_coverage_ptr: int | None = None,
                            coverage_pitch_floats: int = 0, coverage_stride_floats: int = 0,
                            d_importance_ptr: int | None = None, importance_pitch_floats: int = 0,
                            importance_stride_floats: int = 0, d_occ_ptr: int | None = None, occ_pitch: int = 0,
                            occ_stride: int = 0):
        """n planar float32 flows that are already in device memory: the fields of dfx_project_desc (include/dfx.h) as
        arguments, raw pointers as the header gives them."""
        d = DfxProjectDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), t, scale, min_weight,
                           d_importance_ptr, importance_pitch_floats, importance_stride_floats, d_occ_ptr, occ_pitch, occ_stride,
                           d_out_ptr, out_row_pitch_floats, out_plane_stride_floats, out_flow_stride_floats, d_hole_ptr,
                           hole_pitch, hole_stride, d_coverage_ptr, coverage_pitch_floats, coverage_stride_floats, d_work_ptr,
                           work_bytes)
        self._check(self._L.dfx_flow_project_device(self._h, C.byref(d)))

    def flow_project(self, flows, t: float = 1.0, scale: float | None = None, importance=None, occ=None,
                     min_weight: float = 0.25, coverage: bool = False):
        """Flows carried forward along themselves to time t and written where they land, times `scale`
        (dfx_flow_project_device): scale None is -t, the flow from time t back to the first frame; 1 - t the flow on to the
        second; t = 1 with scale -1 the inverse flow.

        flows: (N, 2, H, W) float32.  importance: optional (N, H, W) float32, > 0 counts, how much a source weighs against the
        others landing on the same pixel.  occ: optional (N, H, W) uint8, nonzero = the source pixel is skipped.  min_weight:
        the share of one full-weight source below which a target is a hole (0.25: a choice, see include/dfx.h).  Returns
        (out, hole[, coverage]): (N, 2, H, W) float32 with +0 in the holes, (N, H, W) uint8 with 1 in the holes (the polarity
        flow_median's fill and flow_chain's occ take), and with coverage=True (N, H, W) float32, the summed weight in
        full-weight sources."""
        t, scale, min_weight = _project_settings(t, scale, min_weight)
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W, lead="N")
        n = fl.shape[0]
        importance = _np_planes(importance, n, H, W, np.float32, "importance", "N")
        occ = _np_planes(occ, n, H, W, np.uint8, "occ", "N")
        out = np.empty((n, 2, H, W), np.float32)
        hole = np.empty((n, H, W), np.uint8)
        cov = np.empty((n, H, W), np.float32) if coverage else None
        if n:
            wb = self.flow_project_work_bytes() * min(n, 8)
            with self._staged((fl, importance, occ), (out, hole, cov), [wb]) as (src, dimp, docc, dst, dhole, dcov, work):
                self.flow_project_device(src, W, H * W, 2 * H * W, n, work, wb, t, scale, min_weight, dst, W, H * W, 2 * H * W,
                                         dhole, W, H * W, dcov, W, H * W, dimp, W, H * W, docc, W, H * W)
        return (out, hole, cov) if coverage else (out, hole)

    def flow_invert(self, flows, **kw):
        """The inverse flow by forward projection: flow_project(flows, t=1, scale=-1, **kw)."""
        return self.flow_project(flows, t=1.0, scale=-1.0, **kw)

    def flow_project_tensor(self, flows, t: float = 1.0, scale: float | None = None, importance=None, occ=None,
                            min_weight: float = 0.25, coverage: bool = False, out=None, work=None):
        """flow_project for torch tensors on this handle's device, read and written where they lie.

        flows: (N, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  importance: optional (N, H, W)
        torch.float32; occ: optional (N, H, W) torch.uint8.  out: optional (N, 2, H, W) float32 tensor for the result, not
        `flows` itself.  work: optional contiguous tensor of any dtype to use as the workspace, 8-byte aligned and at least
        flow_project_work_bytes() large (more takes more flows per wave of launches); without it one for min(N, 8) flows is
        allocated through torch.  Returns (out, hole[, coverage]): hole an (N, H, W) uint8 tensor, coverage an (N, H, W)
        float32 tensor.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        t, scale, min_weight = _project_settings(t, scale, min_weight)
        H, W = self.height, self.width
        geom = _flow_geometry(flows, H, W, "flows", "N")
        n, dev = flows.shape[0], flows.device
        igeom = cgeom = (0, 0)
        if importance is not None:
            igeom = _plane_geometry(importance, n, H, W, torch.float32, "importance", "N", "planes")
        if occ is not None:
            cgeom = _plane_geometry(occ, n, H, W, torch.uint8, "occ", "N", "planes")
        if out is not None:
            ogeom = _flow_geometry(out, H, W, "out", "N")
            if out.shape[0] != n:
                raise ValueError("out must be an (N, 2, H, W) torch.float32 tensor")
            if out.data_ptr() == flows.data_ptr() and n:
                raise ValueError("out must not be flows: a projection cannot run in place")
        per = PROJECT_WORDS * 8 * H * W
        if work is not None:
            if not isinstance(work, torch.Tensor) or not work.is_contiguous():
                raise ValueError("work must be a contiguous torch tensor")
            work_bytes = work.numel() * work.element_size()
            if work_bytes < per:
                raise ValueError(f"work must hold at least {per} bytes (flow_project_work_bytes)")
        self._check_devices(flows, "flows must be on this handle's device", (importance, occ, out, work),
                            "importance, occ, out and work must be on the flows' device")
        if work is not None and work.data_ptr() % 8 != 0:
            raise ValueError("work must be 8-byte aligned")
        if out is None:
            out = torch.empty((n, 2, H, W), dtype=torch.float32, device=dev)
            ogeom = (W, H * W, 2 * H * W)
        hole = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        cov = torch.empty((n, H, W), dtype=torch.float32, device=dev) if coverage else None
        if n:
            if work is None:
                work = torch.empty((per * min(n, 8) // 8,), dtype=torch.int64, device=dev)
                work_bytes = work.numel() * 8
            torch.cuda.current_stream(dev).synchronize()
            self.flow_project_device(flows.data_ptr(), *geom, n, work.data_ptr(), work_bytes, t, scale, min_weight,
                                     out.data_ptr(), *ogeom, hole.data_ptr(), W, H * W,
                                     cov.data_ptr() if coverage else None, W, H * W,
                                     importance.data_ptr() if importance is not None else None, *igeom,
                                     occ.data_ptr() if occ is not None else None, *cgeom)
        return (out, hole, cov) if coverage else (out, hole)

    # -- forward warp (splat) of images and float payloads along a flow (dfx_splat_device) ----
    def splat_work_bytes(self, channels: int) -> int:
        """The bytes of workspace one image of `channels` channels of this handle's size needs (dfx_splat_work_bytes)."""
        return int(self._L.dfx_splat_work_bytes(self._h, int(channels)))

    def splat_device(self, d_src_ptr: int, src_dtype: int, channels: int, layout: int, src_pitch: int, src_plane_stride: int,
                     src_image_stride: int, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int,
                     flow_stride_floats: int, n: int, d_work_ptr: int, work_bytes: int, t: float = 1.0,
                     min_weight: float = 0.25, mode: int = 0, hole_mode: int = 0, out_dtype: int = PLANAR_F32,
                     d_out_ptr: int | None = None, out_pitch: int = 0, out_plane_stride: int = 0, out_image_stride: int = 0,
                     d_hole_ptr: int | None = None, hole_pitch: int = 0, hole_stride: int = 0,
                     d_coverage_ptr: int | None = None, coverage_pitch_floats: int = 0, coverage_stride_floats: int = 0,
                     d_importance_ptr: int | None = None, importance_pitch_floats: int = 0,
                     importance_stride_floats: int = 0, d_occ_ptr: int | None = None, occ_pitch: int = 0,
                     occ_stride: int = 0):
        """n sources and n planar float32 flows that are already in device memory: the fields of dfx_splat_desc
        (include/dfx.h) as arguments, codes and raw pointers as the header gives them."""
        d = DfxSplatDesc(d_src_ptr, int(src_dtype), int(channels), int(layout), src_pitch, src_plane_stride, src_image_stride,
                         d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), t, min_weight,
                         int(mode), int(hole_mode), int(out_dtype), d_importance_ptr, importance_pitch_floats,
                         importance_stride_floats, d_occ_ptr, occ_pitch, occ_stride, d_out_ptr, out_pitch, out_plane_stride,
                         out_image_stride, d_hole_ptr, hole_pitch, hole_stride, d_coverage_ptr, coverage_pitch_floats,
                         coverage_stride_floats, d_work_ptr, work_bytes)
        self._check(self._L.dfx_splat_device(self._h, C.byref(d)))

    def _splat_images(self, images, layout_code):
        """A numpy array of sources as the splat takes it: (array, channels, whether it is 8-bit).  uint8 as the warp takes
        images; float32 (n, C, H, W) with C = 1 .. 4."""
        a = np.asarray(images)
        H, W = self.height, self.width
        if a.dtype == np.float32:
            if a.ndim != 4 or a.shape[2:] != (H, W) or not 1 <= a.shape[1] <= SPLAT_MAX_CHANNELS:
                raise ValueError("float32 images must be (n, C, H, W) with C = 1 .. 4")
            return np.ascontiguousarray(a), a.shape[1], False
        if a.dtype != np.uint8:
            raise ValueError("images must be uint8 or float32")
        return self._warp_images(a, layout_code) + (True,)

    def splat(self, images, flows, t: float = 1.0, importance=None, occ=None, mode: str = "mean", holes: str = "zero",
              min_weight: float = 0.25, dtype=None, layout: str = "hwc", return_hole: bool = False,
              return_coverage: bool = False, out=None):
        """Image i carried forward along flows[i] to time t and written where it lands (dfx_splat_device): the forward warp.
        Frame 0 with F_{0->1} gives frame 0 as seen at time t; a float32 payload (labels, depth, features) travels the same
        way.

        images: uint8, (n, H, W), (n, H, W, 3) or, with layout="chw", (n, 3, H, W); or float32 (n, C, H, W), C = 1 .. 4
        (|v| <= 32768; a pixel with a larger or non-finite value is skipped).  flows: (n, 2, H, W) float32.  importance:
        optional (n, H, W) float32, > 0 counts, how much a source weighs against the others landing on the same pixel (the
        exp(alpha * z) of softmax splatting is the caller's).  occ: optional (n, H, W) uint8, nonzero = the source pixel is
        skipped.  mode "mean": the weighted mean of what lands; "sum": the weighted sum in full-weight sources (float32
        only; the caller normalises).  min_weight: the share of one full-weight source below which a target is a hole
        (0.25: a choice, see include/dfx.h).  holes "zero": holes are 0; "keep": the hole pixels of `out` — required then,
        an array of the result's shape and dtype — stay as they are (a background, or an earlier splat).  dtype: np.uint8
        (the default for uint8 images in "mean") or np.float32.  Returns out, or (out[, hole][, coverage]): hole (n, H, W)
        uint8 with 1 in the holes, coverage (n, H, W) float32, the summed weight in full-weight sources."""
        l = _warp_layout(layout)
        img, ch, src_u8 = self._splat_images(images, l)
        if dtype is None:
            dtype = np.uint8 if src_u8 and mode == "mean" else np.float32
        code, np_dt = _warp_dtype(dtype)
        if code not in (WARP_U8, PLANAR_F32):
            raise ValueError("dtype must be np.uint8 or np.float32")
        t, min_weight, m, hm = _splat_settings(t, min_weight, mode, holes, src_u8, code == WARP_U8)
        n = img.shape[0]
        H, W = self.height, self.width
        fl = self._warp_flows(flows, n)
        importance = _np_planes(importance, n, H, W, np.float32, "importance", "n")
        occ = _np_planes(occ, n, H, W, np.uint8, "occ", "n")
        if out is not None:
            if not isinstance(out, np.ndarray) or out.dtype != np_dt or out.shape != img.shape or not out.flags.c_contiguous:
                raise ValueError(f"out must be a contiguous {np_dt.name} array of the images' shape")
        elif hm:
            raise ValueError('holes="keep" needs out: the array whose hole pixels are kept')
        else:
            out = np.empty(img.shape, np_dt)
        hole = np.empty((n, H, W), np.uint8) if return_hole else None
        cov = np.empty((n, H, W), np.float32) if return_coverage else None
        if n:
            planes = ch > 1 and (l == 1 or not src_u8)
            pitch = W * (1 if ch == 1 or planes else 3)
            plane = H * W if planes else 0
            image = ch * H * W
            wb = self.splat_work_bytes(ch) * min(n, 8)
            keep_in, fresh = (out, None) if hm else (None, out)  # a kept output goes up first and comes back by hand
            with self._staged((img, fl, importance, occ, keep_in), (fresh, hole, cov), [wb]) as \
                    (d_img, d_fl, d_imp, d_occ, d_keep, d_fresh, d_hole, d_cov, work):
                d_out = d_keep if hm else d_fresh
                self.splat_device(d_img, WARP_U8 if src_u8 else PLANAR_F32, ch, 1 if planes else 0, pitch, plane, image,
                                  d_fl, W, H * W, 2 * H * W, n, work, wb, t, min_weight, m, hm, code, d_out, pitch, plane,
                                  image, d_hole, W, H * W, d_cov, W, H * W, d_imp, W, H * W, d_occ, W, H * W)
                if hm:
                    self._check(self._L.dfx_memcpy_d2h(self._h, out.ctypes.data, d_out, out.nbytes))
        res = (out,) + ((hole,) if return_hole else ()) + ((cov,) if return_coverage else ())
        return res if len(res) > 1 else out

    def _splat_tensor_payload(self, t, what):
        """(channels, row pitch, plane stride, image stride), in floats, of a torch.float32 tensor of payload planes
        (n, C, H, W), C = 1 .. 4, read from its strides."""
        H, W = self.height, self.width
        if t.dim() != 4 or tuple(t.shape[2:]) != (H, W) or not 1 <= t.shape[1] <= SPLAT_MAX_CHANNELS:
            raise ValueError(f"{what}: float32 must be (n, C, H, W) with C = 1 .. 4")
        n, ch = t.shape[0], t.shape[1]
        if ch == 2:
            return (2,) + _flow_geometry(t, H, W, what, "n")
        st = t.stride()
        pitch = st[2] if H > 1 else W
        plane = st[1] if ch > 1 else H * pitch
        image = st[0] if n > 1 else ch * plane
        if (st[3] != 1 and W > 1) or pitch < W or plane < H * pitch or image < ch * plane:
            raise ValueError(f"{what}: the innermost dimension must be contiguous and rows, planes and images must not overlap")
        return ch, pitch, (plane if ch > 1 else 0), image

    def splat_tensor(self, images, flows, t: float = 1.0, importance=None, occ=None, mode: str = "mean", holes: str = "zero",
                     min_weight: float = 0.25, dtype=None, layout: str | None = None, return_hole: bool = False,
                     return_coverage: bool = False, out=None, work=None):
        """splat for torch tensors on this handle's device, read and written where they lie.

        images: torch.uint8, (n, H, W), (n, 3, H, W) or (n, H, W, 3) — the memory layout, interleaved or three planes, and
        every stride are taken from the tensor, so the NCHW view of an NHWC batch or a slice of a larger tensor is read
        without a copy (layout is needed only for H = W = 3) — or torch.float32 (n, C, H, W), C = 1 .. 4, with a contiguous
        innermost dimension.  flows: (n, 2, H, W) torch.float32.  importance: optional (n, H, W) torch.float32; occ: optional
        (n, H, W) torch.uint8.  dtype: torch.uint8 (the default for uint8 images in "mean") or torch.float32.  out: optional
        tensor of that dtype and the images' shape that lies in memory as the images do, not `images` itself; required for
        holes="keep", whose hole pixels it keeps.  work: optional contiguous tensor of any dtype to use as the workspace,
        8-byte aligned and at least splat_work_bytes(C) large (more takes more images per wave of launches); without it one
        for min(n, 8) images is allocated through torch.  Returns out, or (out[, hole][, coverage]).

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        if layout is not None:
            _warp_layout(layout)
        if not isinstance(images, torch.Tensor) or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError("images must be a torch.uint8 or torch.float32 tensor")
        src_u8 = images.dtype == torch.uint8
        tdt = (torch.uint8 if src_u8 and mode == "mean" else torch.float32) if dtype is None else dtype
        if tdt not in (torch.uint8, torch.float32):
            raise ValueError("dtype must be torch.uint8 or torch.float32")
        t, min_weight, m, hm = _splat_settings(t, min_weight, mode, holes, src_u8, tdt == torch.uint8)
        H, W = self.height, self.width

        def geometry(x, what):
            if src_u8:
                return self._warp_tensor_images(x, layout, what)
            ch, pitch, plane, image = self._splat_tensor_payload(x, what)
            return ch, (1 if ch > 1 else 0), pitch, plane, image, True

        ch, mem, pitch, plane, image, chw = geometry(images, "images")
        n, dev = images.shape[0], images.device
        fgeom = _flow_geometry(flows, H, W, "flows", "n", n, ", one flow per image")
        igeom = cgeom = (0, 0)
        if importance is not None:
            igeom = _plane_geometry(importance, n, H, W, torch.float32, "importance", "n", "planes")
        if occ is not None:
            cgeom = _plane_geometry(occ, n, H, W, torch.uint8, "occ", "n", "planes")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != tdt or out.shape != images.shape:
                raise ValueError(f"out must be a {tdt} tensor of the images' shape")
            och, omem, out_pitch, out_plane, out_image, _ = geometry(out, "out")
            if (och, omem) != (ch, mem):
                raise ValueError("out must lie in memory as the images do (interleaved or planar)")
            if out.data_ptr() == images.data_ptr() and n:
                raise ValueError("out must not be images: a splat cannot run in place")
        elif hm:
            raise ValueError('holes="keep" needs out: the tensor whose hole pixels are kept')
        per = (1 + ch) * 8 * H * W
        if work is not None:
            if not isinstance(work, torch.Tensor) or not work.is_contiguous():
                raise ValueError("work must be a contiguous torch tensor")
            work_bytes = work.numel() * work.element_size()
            if work_bytes < per:
                raise ValueError(f"work must hold at least {per} bytes (splat_work_bytes)")
        self._check_devices(images, "images must be on this handle's device", (flows, importance, occ, out, work),
                            "flows, importance, occ, out and work must be on the images' device")
        if work is not None and work.data_ptr() % 8 != 0:
            raise ValueError("work must be 8-byte aligned")
        if out is None:
            if ch == 3 and mem == 0:  # interleaved memory, whatever the shape's order
                base = torch.empty((n, H, W, 3), dtype=tdt, device=dev)
                out = base.permute(0, 3, 1, 2) if chw else base
                out_pitch, out_plane, out_image = 3 * W, 0, 3 * H * W
            elif src_u8 and ch == 3:
                base = torch.empty((n, 3, H, W), dtype=tdt, device=dev)
                out = base if chw else base.permute(0, 2, 3, 1)
                out_pitch, out_plane, out_image = W, H * W, 3 * H * W
            else:
                out = torch.empty(tuple(images.shape), dtype=tdt, device=dev)
                out_pitch, out_plane, out_image = W, (H * W if ch > 1 else 0), ch * H * W
        hole = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if return_hole else None
        cov = torch.empty((n, H, W), dtype=torch.float32, device=dev) if return_coverage else None
        if n:
            if work is None:
                work = torch.empty((per * min(n, 8) // 8,), dtype=torch.int64, device=dev)
                work_bytes = work.numel() * 8
            torch.cuda.current_stream(dev).synchronize()
            self.splat_device(images.data_ptr(), WARP_U8 if src_u8 else PLANAR_F32, ch, mem, pitch, plane, image,
                              flows.data_ptr(), *fgeom, n, work.data_ptr(), work_bytes, t, min_weight, m, hm,
                              WARP_U8 if tdt == torch.uint8 else PLANAR_F32, out.data_ptr(), out_pitch, out_plane, out_image,
                              hole.data_ptr() if return_hole else None, W, H * W,
                              cov.data_ptr() if return_coverage else None, W, H * W,
                              importance.data_ptr() if importance is not None else None, *igeom,
                              occ.data_ptr() if occ is not None else None, *cgeom)
        res = (out,) + ((hole,) if return_hole else ()) + ((cov,) if return_coverage else ())
        return res if len(res) > 1 else out

    # -- frame interpolation at time t from two frames and their flows (dfx_interpolate_device) ----
    def interpolate_work_bytes(self, fill_passes: int = 3) -> int:
        """The bytes of workspace one pair of this handle's size needs with that many fill passes
        (dfx_interpolate_work_bytes; 0 for fill_passes outside 0 .. 16)."""
        d = DfxInterpDesc()
        d.fill_passes = int(fill_passes)
        return int(self._L.dfx_interpolate_work_bytes(self._h, C.byref(d)))

    def interpolate_device(self, d_img0_ptr: int, d_img1_ptr: int, channels: int, layout: int, img_pitch: int,
                           img_plane_stride: int, img_image_stride: int, d_fwd_ptr: int, d_bwd_ptr: int | None,
                           row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int, n: int, d_work_ptr: int,
                           work_bytes: int, t: float = 0.5, min_weight: float = 0.25, fill_passes: int = 3, ksize: int = 3,
                           d_occ_fwd_ptr: int | None = None, d_occ_bwd_ptr: int | None = None, occ_pitch: int = 0,
                           occ_stride: int = 0, out_dtype: int = WARP_U8, d_out_ptr: int | None = None, out_pitch: int = 0,
                           out_plane_stride: int = 0, out_image_stride: int = 0, d_source_ptr: int | None = None,
                           source_pitch: int = 0, source_stride: int = 0):
        """n pairs of 8-bit images and their planar float32 flows that are already in device memory: the fields of
        dfx_interp_desc (include/dfx.h) as arguments, codes and raw pointers as the header gives them."""
        d = DfxInterpDesc(d_img0_ptr, d_img1_ptr, int(channels), int(layout), img_pitch, img_plane_stride, img_image_stride,
                          d_fwd_ptr, d_bwd_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), t,
                          min_weight, int(fill_passes), int(ksize), d_occ_fwd_ptr, d_occ_bwd_ptr, occ_pitch, occ_stride,
                          int(out_dtype), d_out_ptr, out_pitch, out_plane_stride, out_image_stride, d_source_ptr, source_pitch,
                          source_stride, d_work_ptr, work_bytes)
        self._check(self._L.dfx_interpolate_device(self._h, C.byref(d)))

    def interpolate(self, img0, img1, fwd, bwd=None, t: float = 0.5, occ_fwd=None, occ_bwd=None, fill_passes: int = 3,
                    ksize: int = 3, min_weight: float = 0.25, layout: str = "hwc", dtype=np.uint8, want_source: bool = False):
        """The frames at time t between img0[i] (time 0) and img1[i] (time 1), from the frames and their flows
        (dfx_interpolate_device): the forward flow is projected to time t, the holes of the projection are filled, both
        frames are warped to time t and blended, each pixel from the frames in which it is visible.

        img0, img1: uint8, (n, H, W), (n, H, W, 3) or, with layout="chw", (n, 3, H, W).  fwd: (n, 2, H, W) float32, the flows
        img0 -> img1; bwd: optionally the flows img1 -> img0.  occ_fwd / occ_bwd: optional (n, H, W) uint8 occlusion masks
        of those flows as fb_check gives them (occ_bwd needs bwd).  fill_passes (0 .. 16), ksize (3 or 5) and min_weight
        are choices (3, 3 and 0.25 by default: see include/dfx.h).  dtype: np.uint8 (rounded to nearest even) or np.float32.
        want_source: also return the (n, H, W) uint8 plane that says where each pixel came from: 0 both frames, 1 frame 0
        only, 2 frame 1 only, 3 neither (the plain blend of the pixel's own bytes), + 4 where only the filled flows reached
        it.  Returns out in the images' shape, or (out, source)."""
        t, min_weight, fill_passes, ksize = _interp_settings(t, min_weight, fill_passes, ksize)
        l = _warp_layout(layout)
        code, np_dt = _warp_dtype(dtype)
        if code not in (WARP_U8, PLANAR_F32):
            raise ValueError("dtype must be np.uint8 or np.float32")
        a0, ch = self._warp_images(img0, l, "img0")
        a1, _ = self._warp_images(img1, l, "img1")
        if a1.shape != a0.shape:
            raise ValueError("img1 must have the shape of img0")
        n = a0.shape[0]
        H, W = self.height, self.width
        fwd = _np_flows(fwd, H, W, "fwd", "n", n, ", one flow per pair")
        bwd = _np_flows(bwd, H, W, "bwd", "n", n, ", one flow per pair") if bwd is not None else None
        if occ_bwd is not None and bwd is None:
            raise ValueError("occ_bwd needs bwd")
        occ_fwd = _np_planes(occ_fwd, n, H, W, np.uint8, "occ_fwd", "n")
        occ_bwd = _np_planes(occ_bwd, n, H, W, np.uint8, "occ_bwd", "n")
        out = np.empty(a0.shape, np_dt)
        source = np.empty((n, H, W), np.uint8) if want_source else None
        if n:
            planes = ch == 3 and l == 1
            pitch = W * (1 if ch == 1 or planes else 3)
            plane = H * W if planes else 0
            image = ch * H * W
            wb = _interp_work_bytes(W, H, fill_passes) * min(n, 8)
            with self._staged((a0, a1, fwd, bwd, occ_fwd, occ_bwd), (out, source), [wb]) as \
                    (d_a0, d_a1, d_fwd, d_bwd, d_occ_fwd, d_occ_bwd, d_out, d_source, d_work):
                self.interpolate_device(d_a0, d_a1, ch, l if ch == 3 else 0, pitch, plane, image, d_fwd, d_bwd, W, H * W,
                                        2 * H * W, n, d_work, wb, t, min_weight, fill_passes, ksize, d_occ_fwd, d_occ_bwd, W,
                                        H * W, code, d_out, pitch, plane, image, d_source, W, H * W)
        return (out, source) if want_source else out

    def interpolate_tensor(self, img0, img1, fwd, bwd=None, t: float = 0.5, occ_fwd=None, occ_bwd=None, fill_passes: int = 3,
                           ksize: int = 3, min_weight: float = 0.25, layout: str | None = None, dtype=None,
                           want_source: bool = False, out=None, work=None):
        """interpolate for torch tensors on this handle's device, read and written where they lie.

        img0, img1: torch.uint8 tensors of equal shape and strides, (n, H, W), (n, 3, H, W) or (n, H, W, 3); the memory layout
        and every stride are taken from img0 as warp_tensor takes them, so frames[:-s] and frames[s:] of one clip are read
        without a copy.  fwd, bwd: (n, 2, H, W) torch.float32 with equal strides and a contiguous innermost dimension, e.g.
        what flow_tensor_bidir returns; occ_fwd, occ_bwd: (n, H, W) torch.uint8 with equal strides.  dtype: torch.uint8
        (default) or torch.float32.  out: optional tensor of that dtype and the images' shape and memory layout.  work:
        optional contiguous tensor of any dtype to use as the workspace, 8-byte aligned and at least
        interpolate_work_bytes(fill_passes) large (more takes more pairs per wave of launches); without it one for min(n, 8)
        pairs is allocated through torch.  Returns out, or (out, source) with want_source, source an (n, H, W) uint8 tensor.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        t, min_weight, fill_passes, ksize = _interp_settings(t, min_weight, fill_passes, ksize)
        codes = {torch.uint8: WARP_U8, torch.float32: PLANAR_F32}
        tdt = torch.uint8 if dtype is None else dtype
        if tdt not in codes:
            raise ValueError("dtype must be torch.uint8 or torch.float32")
        if layout is not None:
            _warp_layout(layout)
        for x, what in ((img0, "img0"), (img1, "img1")):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
                raise ValueError(f"{what} must be a torch.uint8 tensor")
        H, W = self.height, self.width
        ch, mem, pitch, plane, image, chw = self._warp_tensor_images(img0, layout, "img0")
        n, dev = img0.shape[0], img0.device
        if img1.shape != img0.shape or (n and img1.stride() != img0.stride()):
            raise ValueError("img1 must have the shape and the strides of img0")
        geom = _flow_geometry(fwd, H, W, "fwd", "n", n, ", one flow per pair")
        if bwd is not None and _flow_geometry(bwd, H, W, "bwd", "n", n, ", one flow per pair") != geom:
            raise ValueError("bwd must have the strides of fwd")
        if occ_bwd is not None and bwd is None:
            raise ValueError("occ_bwd needs bwd")
        ogeom = (0, 0)
        if occ_fwd is not None:
            ogeom = _plane_geometry(occ_fwd, n, H, W, torch.uint8, "occ_fwd", "n")
        if occ_bwd is not None:
            g = _plane_geometry(occ_bwd, n, H, W, torch.uint8, "occ_bwd", "n")
            if occ_fwd is not None and g != ogeom:
                raise ValueError("occ_bwd must have the strides of occ_fwd")
            ogeom = g
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != tdt or out.shape != img0.shape:
                raise ValueError(f"out must be a {tdt} tensor of the images' shape")
            och, omem, out_pitch, out_plane, out_image, _ = self._warp_tensor_images(out, layout, "out")
            if (och, omem) != (ch, mem):
                raise ValueError("out must lie in memory as the images do (interleaved or planar)")
        per = _interp_work_bytes(W, H, fill_passes)
        if work is not None:
            if not isinstance(work, torch.Tensor) or not work.is_contiguous():
                raise ValueError("work must be a contiguous torch tensor")
            work_bytes = work.numel() * work.element_size()
            if work_bytes < per:
                raise ValueError(f"work must hold at least {per} bytes (interpolate_work_bytes)")
        self._check_devices(img0, "img0 must be on this handle's device", (img1, fwd, bwd, occ_fwd, occ_bwd, out, work),
                            "img1, the flows, the masks, out and work must be on img0's device")
        if work is not None and work.data_ptr() % 8 != 0:
            raise ValueError("work must be 8-byte aligned")
        if out is None:
            if ch == 3 and mem == 0:  # interleaved memory, whatever the shape's order
                base = torch.empty((n, H, W, 3), dtype=tdt, device=dev)
                out = base.permute(0, 3, 1, 2) if chw else base
                out_pitch, out_plane, out_image = 3 * W, 0, 3 * H * W
            elif ch == 3:
                base = torch.empty((n, 3, H, W), dtype=tdt, device=dev)
                out = base if chw else base.permute(0, 2, 3, 1)
                out_pitch, out_plane, out_image = W, H * W, 3 * H * W
            else:
                out = torch.empty((n, H, W), dtype=tdt, device=dev)
                out_pitch, out_plane, out_image = W, 0, H * W
        source = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_source else None
        if n:
            if work is None:
                work = torch.empty(((per * min(n, 8) + 7) // 8,), dtype=torch.int64, device=dev)
                work_bytes = work.numel() * 8
            torch.cuda.current_stream(dev).synchronize()
            ptr = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
            self.interpolate_device(img0.data_ptr(), img1.data_ptr(), ch, mem, pitch, plane, image, fwd.data_ptr(), ptr(bwd),
                                    *geom, n, work.data_ptr(), work_bytes, t, min_weight, fill_passes, ksize, ptr(occ_fwd),
                                    ptr(occ_bwd), *ogeom, codes[tdt], out.data_ptr(), out_pitch, out_plane, out_image,
                                    ptr(source), W, H * W)
        return (out, source) if want_source else out

    def interpolate_frames(self, frames, step: int = 1, ts=(0.5,), fill_passes: int = 3, ksize: int = 3,
                           min_weight: float = 0.25, alpha1: float = 0.01, alpha2: float = 0.5):
        """The in-between frames of a clip of gray frames: for every pair (i, i + step) of calc_optflows' pair rule, the
        frames at the times `ts` between frame i (time 0) and frame i + step (time 1).  One calc_optflows_bidir with the
        forward-backward masks, then one interpolate per t.  frames: N uint8 frames (H, W); step >= 1.  Returns an
        (M, len(ts), H, W) uint8 array, M = max(N - step, 0)."""
        step = int(step)
        if step < 1:
            raise ValueError("step must be >= 1")
        ts = tuple(ts)
        for t in ts:
            _interp_settings(t, min_weight, fill_passes, ksize)
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        if any(f.shape != self._frame_shape() for f in frames):
            raise ValueError("frame shape does not match the engine")
        H, W = self.height, self.width
        m = max(len(frames) - step, 0)
        res = np.empty((m, len(ts), H, W), np.uint8)
        if m == 0 or not ts:
            return res
        fwd, bwd, occ_f, occ_b = self.calc_optflows_bidir(frames, step, True, alpha1, alpha2)
        clip = np.stack(frames)
        for k, t in enumerate(ts):
            res[:, k] = self.interpolate(clip[:m], clip[step:], fwd, bwd, t, occ_f, occ_b, fill_passes, ksize, min_weight)
        return res

    # -- motion descriptors of flows: HOF and MBH cell histograms (dfx_flow_hist_device) ----
    def flow_hist_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                         n: int, kinds: int, cell: int, bins: int, still_thr: float, norm: int = 0,
                         d_sums_ptr: int | None = None, sums_stride: int = 0, d_out_ptr: int | None = None,
                         out_slot_stride_floats: int = 0, out_col_stride_floats: int = 0, out_row_stride_floats: int = 0,
                         out_flow_stride_floats: int = 0, d_mask_ptr: int | None = None, mask_pitch: int = 0,
                         mask_stride: int = 0):
        """n planar float32 flows that are already in device memory, as cell histograms: the fields of dfx_hist_desc
        (include/dfx.h) as arguments, codes and raw pointers as the header gives them."""
        d = DfxHistDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), d_mask_ptr, mask_pitch,
                        mask_stride, int(kinds), int(cell), int(bins), float(still_thr), int(norm), d_sums_ptr, sums_stride,
                        d_out_ptr, out_slot_stride_floats, out_col_stride_floats, out_row_stride_floats,
                        out_flow_stride_floats)
        self._check(self._L.dfx_flow_hist_device(self._h, C.byref(d)))

    def flow_hist(self, flows, kinds=("hof", "mbhx", "mbhy"), cell: int = 8, bins: int = 8, still_thr: float = 0.4,
                  norm: str = "none", mask=None, want_sums: bool = False):
        """Motion descriptors of flows (dfx_flow_hist_device): per cell x cell pixels the orientation histogram of the flow
        (HOF, with a slot for still pixels) and of the spatial derivatives of u and v (MBHx, MBHy), Dalal et al. 2006 and the
        descriptors of dense trajectories.

        flows: (n, 2, H, W) float32.  kinds: a name or names of "hof", "mbhx", "mbhy"; the channels lie in that order.  bins
        2 .. 16 orientation slots per channel, bin 0 centred on +x, counter-clockwise with y down; cell 4, 8, 16 or 32.
        still_thr: a HOF magnitude at or below it counts into the still slot (iDT's 0.4 by default; negative: never).  norm
        "none": weights in pixels times magnitude; "l1", "l1_sqrt", "l2": per cell and channel.  mask: optional (n, H, W)
        uint8, nonzero = not here; masked, NaN, infinite and huge (> 1e9) pixels add nothing, and neither does an MBH pixel
        with such a neighbour.  Returns (n, D, CH, CW) float32 with CH = ceil(H / cell), CW = ceil(W / cell), the slots named
        by flow_hist_slots(kinds, bins); with want_sums also the integer sums (n, CH, CW, D) int64 (weights times 256)."""
        code, cell, bins, thr, ncode, D = _hist_settings(kinds, cell, bins, still_thr, norm)
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W, lead="n")
        n = fl.shape[0]
        mask = _np_planes(mask, n, H, W, np.uint8, "mask", "n")
        CH, CW = -(-H // cell), -(-W // cell)
        out = np.zeros((n, D, CH, CW), np.float32)
        sums = np.zeros((n, CH, CW, D), np.int64) if want_sums else None
        if n:
            with self._staged((fl, mask), (out, sums)) as (d_fl, d_mask, d_out, d_sums):
                self.flow_hist_device(d_fl, W, H * W, 2 * H * W, n, code, cell, bins, thr, ncode, d_sums, CH * CW * D, d_out,
                                      CH * CW, 1, CW, D * CH * CW, d_mask, W, H * W)
        return (out, sums) if want_sums else out

    def flow_hist_tensor(self, flows, kinds=("hof", "mbhx", "mbhy"), cell: int = 8, bins: int = 8, still_thr: float = 0.4,
                         norm: str = "none", mask=None, want_sums: bool = False, layout: str = "chw", out=None):
        """flow_hist for torch tensors on this handle's device, read and written where they lie.

        flows: (n, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  mask: optional (n, H, W) torch.uint8.
        layout "chw": the result is (n, D, CH, CW); "hwc": (n, CH, CW, D).  out: optional torch.float32 tensor of that shape
        with any strides (a slice of a larger tensor is written in place); otherwise the result is allocated contiguous.
        want_sums: also return the integer sums as an (n, CH, CW, D) torch.int64 tensor.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        code, cell, bins, thr, ncode, D = _hist_settings(kinds, cell, bins, still_thr, norm)
        lay = _warp_layout(layout)
        H, W = self.height, self.width
        row_pitch, flow_plane, flow_stride = _flow_geometry(flows, H, W, "flows", "n")
        n, dev = flows.shape[0], flows.device
        mask_pitch = mask_stride = 0
        if mask is not None:
            mask_pitch, mask_stride = _plane_geometry(mask, n, H, W, torch.uint8, "mask", "n")
        CH, CW = -(-H // cell), -(-W // cell)
        shape = (n, D, CH, CW) if lay else (n, CH, CW, D)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != shape):
            raise ValueError(f"out must be a torch.float32 tensor of shape {shape}")
        self._check_devices(flows, "flows must be on this handle's device", (mask, out),
                            "mask and out must be on the flows' device")
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=dev)
        so = out.stride()
        s_flow, (s_slot, s_row, s_col) = so[0], ((so[1], so[2], so[3]) if lay else (so[3], so[1], so[2]))
        if min(so) < 0:
            raise ValueError("out: strides must not be negative")
        sums = torch.empty((n, CH, CW, D), dtype=torch.int64, device=dev) if want_sums else None
        torch.cuda.current_stream(dev).synchronize()
        if n:
            self.flow_hist_device(flows.data_ptr(), row_pitch, flow_plane, flow_stride, n, code, cell, bins, thr, ncode,
                                  sums.data_ptr() if want_sums else None, CH * CW * D, out.data_ptr(), s_slot, s_col, s_row,
                                  s_flow, mask.data_ptr() if mask is not None else None, mask_pitch, mask_stride)
        return (out, sums) if want_sums else out

    # -- flows as colour images: the Middlebury wheel, unknown pixels marked (dfx_flow_colour_device) ----
    def flow_colour_device(self, d_flow_ptr: int, row_pitch_floats: int, plane_stride_floats: int, flow_stride_floats: int,
                           n: int, d_out_ptr: int, out_pitch: int, out_plane_stride: int, out_image_stride: int,
                           norm: int = 1, max_rad: float = 0.0, d_max2_ptr: int | None = None, order: int = 1,
                           layout: int = 0, unknown=(0, 0, 0), d_mask_ptr: int | None = None, mask_pitch: int = 0,
                           mask_stride: int = 0, d_frame_ptr: int | None = None, frame_channels: int = 0,
                           frame_layout: int = 0, frame_pitch: int = 0, frame_plane_stride: int = 0,
                           frame_image_stride: int = 0, alpha256: int = 256):
        """n planar float32 flows that are already in device memory, as colour images: the fields of dfx_colour_desc
        (include/dfx.h) as arguments, codes and raw pointers as the header gives them."""
        d = DfxColourDesc(d_flow_ptr, row_pitch_floats, plane_stride_floats, flow_stride_floats, int(n), d_mask_ptr, mask_pitch,
                          mask_stride, int(norm), float(max_rad), d_max2_ptr, int(order), int(layout), d_out_ptr, out_pitch,
                          out_plane_stride, out_image_stride, (C.c_uint8 * 3)(*[int(c) for c in unknown]), d_frame_ptr,
                          int(frame_channels), int(frame_layout), frame_pitch, frame_plane_stride, frame_image_stride,
                          int(alpha256))
        self._check(self._L.dfx_flow_colour_device(self._h, C.byref(d)))

    def flow_colour(self, flows, norm: str = "flow", max_rad: float | None = None, mask=None, order: str = "rgb",
                    layout: str = "hwc", unknown=(0, 0, 0), frame=None, alpha: float = 0.5, return_max: bool = False):
        """Flows as colour images on the Middlebury wheel (Baker et al. 2011; dfx_flow_colour_device): hue from the direction,
        saturation from the magnitude over a radius R.

        flows: (n, 2, H, W) float32.  norm "flow": R is the largest magnitude of the known pixels of each flow; "batch": of
        all n flows (torchvision's flow_to_image rule); "fixed": R = max_rad, longer vectors are darkened.  mask: optional
        (n, H, W) uint8, nonzero = unknown (an occlusion mask, a hole plane, a mask_out).  Unknown pixels — masked, NaN,
        infinite or beyond 1e9 — get the colour `unknown` (in the output's channel order) and do not enter R.  order "rgb" or
        "bgr"; layout "hwc": (n, H, W, 3) uint8, "chw": (n, 3, H, W).  frame: optional uint8 frames to blend over, (n, H, W)
        gray or 3 channels in the output's order and layout; alpha is the weight of the colours, alpha256 =
        int(round(alpha * 256)).  return_max: also return the radii sqrt(M2) as an (n,) float32 array and sqrt(MB2)."""
        code, rad, ocode, lay, unk, a256 = _colour_settings(norm, max_rad, order, layout, unknown, alpha)
        H, W = self.height, self.width
        fl = _np_flows(flows, H, W, lead="n")
        n = fl.shape[0]
        mask = _np_planes(mask, n, H, W, np.uint8, "mask", "n")
        fch = 0
        if frame is not None:
            frame = np.asarray(frame)
            if frame.dtype != np.uint8 or frame.shape not in ((n, H, W), (n, 3, H, W) if lay else (n, H, W, 3)):
                raise ValueError("frame must be uint8, (n, H, W) or the images' shape")
            frame = np.ascontiguousarray(frame)
            fch = 1 if frame.ndim == 3 else 3
        out = np.empty((n, 3, H, W) if lay else (n, H, W, 3), np.uint8)
        m2 = np.zeros(n + 1, np.float32)
        if n:
            want_max = code != 0 or return_max
            with self._staged((fl, mask, frame), (out, m2 if want_max else None)) as (d_fl, d_mask, d_frame, d_out, d_m2):
                geom = (W, H * W, 3 * H * W) if lay else (3 * W, 0, 3 * H * W)
                fgeom = (W, 0, H * W) if fch == 1 else geom
                self.flow_colour_device(d_fl, W, H * W, 2 * H * W, n, d_out, *geom, code, rad, d_m2, ocode, lay, unk, d_mask, W,
                                        H * W, d_frame, fch, lay, *fgeom, a256)
        if return_max:
            r = np.sqrt(m2)
            return out, r[:n], r[n]
        return out

    def flow_colour_tensor(self, flows, norm: str = "flow", max_rad: float | None = None, mask=None, order: str = "rgb",
                           layout: str = "hwc", unknown=(0, 0, 0), frame=None, alpha: float = 0.5, return_max: bool = False,
                           out=None):
        """flow_colour for torch tensors on this handle's device, read and written where they lie.

        flows: (n, 2, H, W) torch.float32 with a contiguous innermost dimension, e.g. what flow_tensor returns; every stride is
        taken from the tensor, so a slice of a larger tensor is read without a copy.  mask: optional (n, H, W) torch.uint8.
        frame: optional torch.uint8, (n, H, W), (n, 3, H, W) or (n, H, W, 3), interleaved or planar in memory under either
        shape, channels in the output's order.  out: optional torch.uint8 tensor of shape (n, H, W, 3) (layout "hwc") or
        (n, 3, H, W) ("chw"), interleaved or planar in memory; otherwise the images are allocated contiguous in that shape.
        return_max: also return the radii sqrt(M2) as an (n,) float32 tensor and sqrt(MB2) as a 0-d tensor.
        norm="batch", order="rgb", layout="chw" is torchvision's flow_to_image up to the unknown-pixel rule and the
        polynomial angle.

        Torch's current stream on that device is synchronised before the call; the call returns with its device work
        complete.  Raises ValueError before the library is reached for a wrong setting, dtype, device, shape or stride."""
        import torch

        code, rad, ocode, lay, unk, a256 = _colour_settings(norm, max_rad, order, layout, unknown, alpha)
        H, W = self.height, self.width
        row_pitch, flow_plane, flow_stride = _flow_geometry(flows, H, W, "flows", "n")
        n, dev = flows.shape[0], flows.device
        mask_pitch = mask_stride = 0
        if mask is not None:
            mask_pitch, mask_stride = _plane_geometry(mask, n, H, W, torch.uint8, "mask", "n")
        fch, fmem, fgeom = 0, 0, (0, 0, 0)
        if frame is not None:
            if not isinstance(frame, torch.Tensor) or frame.dtype != torch.uint8 or frame.dim() < 3 or frame.shape[0] != n:
                raise ValueError("frame must be a torch.uint8 tensor, (n, H, W), (n, 3, H, W) or (n, H, W, 3)")
            fch, fmem, fp, fpl, fim, _ = self._warp_tensor_images(frame, layout, "frame")
            fgeom = (fp, fpl, fim)
        shape = (n, 3, H, W) if lay else (n, H, W, 3)
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape:
                raise ValueError(f"out must be a torch.uint8 tensor of shape {shape}")
            _, omem, op, opl, oim, _ = self._warp_tensor_images(out, layout, "out")
        self._check_devices(flows, "flows must be on this handle's device", (mask, frame, out),
                            "mask, frame and out must be on the flows' device")
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=dev)
            omem, op, opl, oim = (1, W, H * W, 3 * H * W) if lay else (0, 3 * W, 0, 3 * H * W)
        want_max = code != 0 or return_max
        m2 = torch.zeros(n + 1, dtype=torch.float32, device=dev) if want_max else None
        torch.cuda.current_stream(dev).synchronize()
        if n:
            self.flow_colour_device(flows.data_ptr(), row_pitch, flow_plane, flow_stride, n, out.data_ptr(), op, opl, oim,
                                    code, rad, m2.data_ptr() if want_max else None, ocode, omem, unk,
                                    mask.data_ptr() if mask is not None else None, mask_pitch, mask_stride,
                                    frame.data_ptr() if frame is not None else None, fch, fmem, *fgeom, a256)
        if return_max:
            r = torch.sqrt(m2)
            return out, r[:n], r[n]
        return out

    def flow_colour_key(self, size: int):
        """The usual legend disc as a (size, size, 3) uint8 RGB image: flow_colour of the radial flow u = x - c, v = y - c
        with c = (size - 1) / 2, everything outside the disc of radius c masked (black).  The handle's own size does not
        matter: a size x size handle of the same algorithm and device is used for the call where it differs."""
        if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
            raise ValueError("size must be a positive integer")
        size = int(size)
        c = np.float32(size - 1) / np.float32(2)
        d = np.arange(size, dtype=np.float32) - c
        u, v = np.broadcast_to(d[None, :], (size, size)), np.broadcast_to(d[:, None], (size, size))
        flow = np.stack([u, v]).astype(np.float32)[None]
        mask = ((u * u + v * v) > c * c).astype(np.uint8)[None]
        if (self.width, self.height) == (size, size):
            return self.flow_colour(flow, mask=mask)[0]
        with FlowEngine(size, size, self.algorithm, device=self._device) as eng:
            return eng.flow_colour(flow, mask=mask)[0]

    def flow_tensor_bidir(self, frames, step: int, check: bool = True, alpha1: float = 0.01, alpha2: float = 0.5, out=None):
        """flow_tensor for both directions and the occlusion masks: (fwd, bwd, occ_fwd, occ_bwd) as torch tensors on the
        frames' device — two (M, 2, H, W) float32 tensors of raw flow values (fwd: flow_tensor's for `step`, bwd: for -step)
        and two (M, H, W) uint8 masks of the forward-backward check, None with check=False.  Every frame is built once.

        frames: as flow_tensor takes them, strides read from the tensor.  out: optional 4-tuple (fwd, bwd, occ_fwd, occ_bwd)
        to write into (the masks None with check=False): fwd and bwd float32 with equal strides, the two masks uint8 with
        equal strides, innermost dimension contiguous, rows, planes and flows not overlapping.  Torch's current stream on
        that device is synchronised before the call; the call returns with its device work complete."""
        import torch

        n, pitch, frame_stride, layout = self._tensor_frames(frames)
        dev = frames.device
        m = self._peek_pairs(n, step)
        H, W = self.height, self.width
        if out is None:
            out = (torch.empty((m, 2, H, W), dtype=torch.float32, device=dev),
                   torch.empty((m, 2, H, W), dtype=torch.float32, device=dev),
                   torch.empty((m, H, W), dtype=torch.uint8, device=dev) if check else None,
                   torch.empty((m, H, W), dtype=torch.uint8, device=dev) if check else None)
        if len(out) != 4:
            raise ValueError("out must be a 4-tuple (fwd, bwd, occ_fwd, occ_bwd)")
        fwd, bwd, of, ob = out
        for t in (fwd, bwd):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (m, 2, H, W):
                raise ValueError(f"out: fwd and bwd must be float32 tensors of shape {(m, 2, H, W)} on the frames' device")
        if fwd.stride() != bwd.stride():
            raise ValueError("out: fwd and bwd must have equal strides")
        so = fwd.stride()
        row_pitch = so[2] if H > 1 else W
        plane_stride, flow_stride = so[1], (so[0] if m > 1 else 2 * so[1])
        if so[3] != 1 or row_pitch < W or plane_stride < H * row_pitch or flow_stride < 2 * plane_stride:
            raise ValueError("out: the innermost dimension must be contiguous and rows, planes and flows must not overlap")
        occ_pitch = occ_stride = 0
        if check:
            for t in (of, ob):
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != dev or tuple(t.shape) != (m, H, W):
                    raise ValueError(f"out: the masks must be uint8 tensors of shape {(m, H, W)} on the frames' device")
            if of.stride() != ob.stride():
                raise ValueError("out: the two masks must have equal strides")
            sm = of.stride()
            occ_pitch = sm[1] if H > 1 else W
            occ_stride = sm[0] if m > 1 else occ_pitch * H
            if sm[2] != 1 or occ_pitch < W or occ_stride < H * occ_pitch:
                raise ValueError("out: the masks' innermost dimension must be contiguous and rows and planes must not overlap")
        elif of is not None or ob is not None:
            raise ValueError("out: the masks must be None with check=False")
        self._check_devices(frames, "frames must be on this handle's device")
        self._num_pairs(n, step)
        torch.cuda.current_stream(dev).synchronize()

        def call():
            self._arm()
            self._check(self._L.dfx_calc_batch_bidir_device(
                self._h, frames.data_ptr() if n else None, pitch, frame_stride, n, int(step),
                fwd.data_ptr() if m else None, bwd.data_ptr() if m else None, row_pitch, plane_stride, flow_stride,
                float(alpha1), float(alpha2), of.data_ptr() if check and m else None,
                ob.data_ptr() if check and m else None, occ_pitch, occ_stride))
            return fwd, bwd, (of if check else None), (ob if check else None)

        if m == 0 and check:  # (an empty tensor's data_ptr is 0: one mask pointer alone would be refused; there is nothing to do)
            self._armed_seg = self._armed_src = None
            return fwd, bwd, of, ob
        if layout is not None:  # how THIS tensor lies in memory, declared for this call only
            self._set_call_layout(*layout)
            try:
                return call()
            finally:
                self._set_call_layout(1, 0)
        return call()

    def _tensor_frames(self, frames):
        """A torch frames tensor as the device-resident calls take it: (n, row pitch, frame stride, layout), in bytes and read
        from the tensor's strides; layout is None, or the (layout, plane stride) to declare for the one call that reads a
        tensor lying otherwise than the declared source format.  ValueError for a wrong type, rank or shape, a non-contiguous
        innermost dimension, overlapping rows, planes or frames."""
        import torch

        if not isinstance(frames, torch.Tensor):
            raise ValueError("frames must be a torch tensor")
        if frames.dtype != torch.uint8:
            raise ValueError("frames must be torch.uint8")
        shape = self._frame_shape()
        chw = bool(getattr(self, "_src_chw", False))
        if frames.dim() != 1 + len(shape) or tuple(frames.shape[1:]) != tuple(shape):
            raise ValueError(f"frames must be (N,) + {tuple(shape)}")
        st = frames.stride()
        # a channels-first SHAPE over interleaved memory — the permuted view of an NHWC batch, torch's channels_last — is read
        # as the interleaved frames it is
        nhwc_view = chw and st[3] == 3 and st[1] == 1
        if not nhwc_view and (st[-1] != 1 or (len(shape) == 3 and not chw and st[2] != 3)):
            raise ValueError("the innermost dimension of frames must be contiguous")
        n = int(frames.shape[0])
        plane_stride = 0
        if nhwc_view:
            rows, row_bytes = shape[1], shape[2] * 3
            pitch = st[2] if rows > 1 else row_bytes
            span = pitch * rows
        elif chw:
            rows, row_bytes = shape[1], shape[2]
            pitch = st[2] if rows > 1 else row_bytes  # (the stride of a dimension of size 1 means nothing)
            plane_stride = st[1]
            if pitch < row_bytes or plane_stride < pitch * rows:
                raise ValueError("frames: rows or planes overlap")
            span = 2 * plane_stride + pitch * rows
        else:
            rows, row_bytes = shape[0], shape[1] * (3 if len(shape) == 3 else 1)
            pitch = st[1] if rows > 1 else row_bytes
            span = pitch * rows
        frame_stride = st[0] if n > 1 else span
        if pitch < row_bytes or frame_stride < span:
            raise ValueError("frames: rows or frames overlap")
        layout = None
        if nhwc_view or (chw and plane_stride != pitch * rows):
            layout = (0 if nhwc_view else 1, plane_stride)
        return n, pitch, frame_stride, layout

    # -- flow bounding on the device (reference: convertFlowToImage, src/common.cpp:4-16) ------
    def calc_optflows_u8(self, frames_gray, step: int, bound: float, lower: float | None = None):
        """calc_optflows followed by encodeFlowMap's bounding (src/common.cpp:48-64), all on the device.

        Returns (img_x, img_y): two lists of M (H, W) uint8 planes.  The reference bounds to
        [-bound, bound]; pass `lower` for an asymmetric interval [lower, bound]."""
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        img_x = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        img_y = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        if m == 0:
            return img_x, img_y
        self._check_shapes(frames)
        lo = -float(bound) if lower is None else float(lower)
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        xp = (C.c_void_p * m)(*[f.ctypes.data for f in img_x])
        yp = (C.c_void_p * m)(*[f.ctypes.data for f in img_y])
        self._arm()
        self._check(self._L.dfx_calc_batch_u8(self._h, fp, self._host_pitch(frames[0]), n, int(step), lo, float(bound), xp,
                                              yp, self.width))
        return img_x, img_y

    # -- the -st=png scheme on the device (reference: convertFlowToPngImage, src/common.cpp:18-46) ------
    def calc_optflows_png(self, frames_gray, step: int, submit: bool = False):
        """calc_optflows followed by convertFlowToPngImage's arithmetic on the device: per flow the adaptive bounds
        (minMaxLoc, the ceil(.../4)*4 rule with its `% 8 == 0 -> += 4` step) and the two convertTo(CV_8U) planes.

        Returns (img_x, img_y, bounds): two lists of M (H, W) uint8 planes and an (M, 2) float64 array of
        (bound_x, bound_y).  png_bgr() assembles the reference's 3-channel image from them.  submit=True goes through
        dfx_submit_batch_png + dfx_wait (the host shell's form)."""
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        img_x = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        img_y = [np.empty((self.height, self.width), dtype=np.uint8) for _ in range(m)]
        bounds = np.zeros((m, 2), np.float64)
        if m == 0:
            return img_x, img_y, bounds
        self._check_shapes(frames)
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        xp = (C.c_void_p * m)(*[f.ctypes.data for f in img_x])
        yp = (C.c_void_p * m)(*[f.ctypes.data for f in img_y])
        bp = bounds.ctypes.data_as(C.POINTER(C.c_double))
        self._arm()
        if submit:
            t = C.c_uint64(0)
            self._check(self._L.dfx_submit_batch_png(self._h, fp, self._host_pitch(frames[0]), n, int(step), xp, yp, self.width,
                                                     bp, C.byref(t)))
            self._check(self._L.dfx_wait(self._h, t.value))
        else:
            self._check(self._L.dfx_calc_batch_png(self._h, fp, self._host_pitch(frames[0]), n, int(step), xp, yp, self.width, bp))
        return img_x, img_y, bounds

    def calc_optflows_png_device(self, d_frames_ptr: int, pitch: int, frame_stride: int, n_frames: int, step: int,
                                 d_img_x_ptr: int, d_img_y_ptr: int, img_pitch: int, img_stride: int, d_bounds_ptr: int):
        self._num_pairs(n_frames, step)
        self._arm()
        self._check(self._L.dfx_calc_batch_png_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step),
                                                      d_img_x_ptr, d_img_y_ptr, img_pitch, img_stride, d_bounds_ptr))

    def flow_to_png_device(self, d_flows_ptr: int, flow_stride_floats: int, n: int, d_img_x_ptr: int, d_img_y_ptr: int,
                           img_pitch: int, img_stride: int, d_bounds_ptr: int):
        self._check(self._L.dfx_flow_to_png_device(self._h, d_flows_ptr, flow_stride_floats, n, d_img_x_ptr, d_img_y_ptr,
                                                   img_pitch, img_stride, d_bounds_ptr))

    @staticmethod
    def png_bgr(img_x: np.ndarray, img_y: np.ndarray, bound_x: float, bound_y: float) -> np.ndarray:
        """The reference's 3-channel PNG image (src/common.cpp:41-45) from the device's planes and bounds: channel 2 is
        bound_x / 4 on rows 0 .. int(H / 2) (rectangle's inclusive box, Point's truncation) and bound_y / 4 below."""
        h, w = img_x.shape
        out = np.empty((h, w, 3), np.uint8)
        out[..., 0], out[..., 1] = img_x, img_y
        half = int(h / 2)
        sat = lambda v: int(min(255, max(0, np.rint(v))))  # noqa: E731 — saturate_cast<uchar>(double): cvRound, clamp
        out[: half + 1, :, 2] = sat(bound_x / 4)
        out[half + 1:, :, 2] = sat(bound_y / 4)
        return out

    def calc_optflows_jpeg(self, frames_gray, step: int, bound: float, quality: int = 95):
        """encodeFlowMap of every flow of the FlowBuffer on the device (src/common.cpp:48-64): returns two lists of
        `bytes`, the flow_x and flow_y JPEG files (bounded to [-bound, bound], quality like cv::imencode)."""
        frames = self._frames_in(frames_gray)
        n = len(frames)
        m = self._num_pairs(n, step)
        if m == 0:
            return [], []
        self._check_shapes(frames)
        cap = int(self._L.dfx_jpeg_capacity(self._h))
        bx = [np.empty(cap, np.uint8) for _ in range(m)]
        by = [np.empty(cap, np.uint8) for _ in range(m)]
        sx, sy = (C.c_uint32 * m)(), (C.c_uint32 * m)()
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in frames])
        self._arm()
        self._check(self._L.dfx_calc_batch_jpeg(self._h, fp, self._host_pitch(frames[0]), n, int(step), -float(bound),
                                                float(bound), int(quality), (C.c_void_p * m)(*[b.ctypes.data for b in bx]),
                                                (C.c_void_p * m)(*[b.ctypes.data for b in by]), cap, sx, sy))
        return ([bx[i][:sx[i]].tobytes() for i in range(m)], [by[i][:sy[i]].tobytes() for i in range(m)])

    def encode_jpeg(self, planes, quality: int = 95):
        """imencode(".jpg") of (H, W) uint8 planes on the device: a list of `bytes`."""
        ps = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
        n = len(ps)
        if n == 0:
            return []
        if any(p.shape != (self.height, self.width) for p in ps):
            raise ValueError("plane shape does not match the engine")
        cap = int(self._L.dfx_jpeg_capacity(self._h))
        bufs = [np.empty(cap, np.uint8) for _ in range(n)]
        sizes = (C.c_uint32 * n)()
        self._check(self._L.dfx_encode_jpeg(self._h, (C.c_void_p * n)(*[p.ctypes.data for p in ps]), self.width, n,
                                            int(quality), (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), cap, sizes))
        return [bufs[i][:sizes[i]].tobytes() for i in range(n)]

    # -- colour frame extraction (reference: extract_frames_only, src/denseflow_gpu.cpp:82-105) ------------
    def _bgr(self, frames):
        fs = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        if fs and (any(f.shape != fs[0].shape for f in fs) or len(fs[0].shape) != 3 or fs[0].shape[2] != 3):
            raise ValueError("frames must share one (h, w, 3) shape")
        return fs

    def prepare_frames_bgr(self, frames):
        """cv::resize(INTER_LINEAR) of (h, w, 3) uint8 BGR frames to the engine's size, every channel on its own."""
        src = self._bgr(frames)
        n = len(src)
        out = [np.empty((self.height, self.width, 3), np.uint8) for _ in range(n)]
        if n == 0:
            return out
        sh, sw = src[0].shape[:2]
        sp = (C.c_void_p * n)(*[f.ctypes.data for f in src])
        op = (C.c_void_p * n)(*[f.ctypes.data for f in out])
        self._check(self._L.dfx_prepare_frames_bgr(self._h, sp, sw * 3, sw, sh, n, op, self.width * 3))
        return out

    def prepare_frames_bgr_device(self, d_src_ptr: int, src_pitch: int, src_frame_stride: int, src_width: int,
                                  src_height: int, n: int, d_dst_ptr: int, dst_pitch: int, dst_frame_stride: int):
        self._check(self._L.dfx_prepare_frames_bgr_device(self._h, d_src_ptr, src_pitch, src_frame_stride, int(src_width),
                                                          int(src_height), int(n), d_dst_ptr, dst_pitch, dst_frame_stride))

    def encode_jpeg_bgr(self, frames, quality: int = 95):
        """imencode(".jpg", bgr) of (H, W, 3) uint8 BGR frames on the device (YCbCr 4:2:0): a list of `bytes`."""
        fs = self._bgr(frames)
        if fs and fs[0].shape[:2] != (self.height, self.width):
            raise ValueError("frame shape does not match the engine")
        return self.extract_frames(fs, quality)

    def extract_frames(self, frames, quality: int = 95, submit: bool = False):
        """The -s=0 mode for one buffer of (h, w, 3) uint8 BGR source frames: resize to the engine's size and encode,
        all on the device.  Returns a list of `bytes`.  submit=True goes through dfx_submit_extract_frames + dfx_wait."""
        fs = self._bgr(frames)
        n = len(fs)
        if n == 0:
            return []
        sh, sw = fs[0].shape[:2]
        cap = int(self._L.dfx_jpeg_capacity_bgr(self._h))
        bufs = [np.empty(cap, np.uint8) for _ in range(n)]
        sizes = (C.c_uint32 * n)()
        fp = (C.c_void_p * n)(*[f.ctypes.data for f in fs])
        bp = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
        if submit:
            t = C.c_uint64(0)
            self._check(self._L.dfx_submit_extract_frames(self._h, fp, sw * 3, sw, sh, n, int(quality), bp, cap, sizes,
                                                          C.byref(t)))
            self._check(self._L.dfx_wait(self._h, t.value))
        else:
            self._check(self._L.dfx_extract_frames(self._h, fp, sw * 3, sw, sh, n, int(quality), bp, cap, sizes))
        return [bufs[i][:sizes[i]].tobytes() for i in range(n)]

    def frames_device_bytes(self) -> int:
        """Device memory held by the colour extraction state of this handle."""
        return int(self._L.dfx_frames_device_bytes(self._h))

    def calc_optflows_u8_device(self, d_frames_ptr: int, pitch: int, frame_stride: int, n_frames: int, step: int,
                                lower: float, upper: float, d_img_x_ptr: int, d_img_y_ptr: int, img_pitch: int,
                                img_stride: int):
        """Frames and bounded planes resident in HBM (raw device pointers)."""
        self._check(self._L.dfx_calc_batch_u8_device(self._h, d_frames_ptr, pitch, frame_stride, n_frames, int(step),
                                                     float(lower), float(upper), d_img_x_ptr, d_img_y_ptr,
                                                     img_pitch, img_stride))

    def flow_to_u8_device(self, d_flows_ptr: int, flow_stride_floats: int, n: int, lower: float, upper: float,
                          d_img_x_ptr: int, d_img_y_ptr: int, img_pitch: int, img_stride: int):
        """Bound n flows that are already in device memory."""
        self._check(self._L.dfx_flow_to_u8_device(self._h, d_flows_ptr, flow_stride_floats, int(n), float(lower),
                                                  float(upper), d_img_x_ptr, d_img_y_ptr, img_pitch, img_stride))

    def stats(self) -> DfxStats:
        s = DfxStats()
        self._check(self._L.dfx_get_stats(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        self._L.dfx_reset_stats(self._h)

    def tvl1_batch_tables(self):
        """dfxi_tvl1_batch_tables (test hook): for every pair of the last device batch, in pair order, the executed inner
        iterations as a [levels][DFX_MAX_WARPS] table (the layout of DfxStats.iters_table) and the convergence sums
        evaluated per level.  Returns (tables, checks)."""
        st = self.stats()
        cap = max(int(st.batch), 1)
        iters = (C.c_int * (cap * DFX_MAX_LEVELS * DFX_MAX_WARPS))()
        checks = (C.c_int * (cap * DFX_MAX_LEVELS))()
        n = self._L.dfxi_tvl1_batch_tables(self._h, cap, iters, checks)
        if n < 0:
            raise DfxError(-n, f"dfxi_tvl1_batch_tables failed with status {-n}")
        it = np.ctypeslib.as_array(iters).reshape(cap, DFX_MAX_LEVELS, DFX_MAX_WARPS)
        ck = np.ctypeslib.as_array(checks).reshape(cap, DFX_MAX_LEVELS)
        return ([it[b, :st.levels].tolist() for b in range(n)], [ck[b, :st.levels].tolist() for b in range(n)])
