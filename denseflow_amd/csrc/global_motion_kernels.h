// global_motion_kernels.h — launcher of the robust parametric fit of a flow's dominant (camera) motion and of its removal
// (global_motion_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dfx.h"

enum : int { GM_TRANSLATION = 0, GM_AFFINE = 1 }; // = DFX_GM_TRANSLATION / DFX_GM_AFFINE of include/dfx.h
enum : int { GM_MAX_ROUNDS = 8 };                 // = the length of dfx_gm_result.inliers
enum : int { GM_BAND_ROWS = 32 };                 // rows of a flow one workgroup of the accumulate kernel walks
enum : int { GM_SUMS = 12 };                      // S1 Sx Sy Sxx Sxy Syy Su Sxu Syu Sv Sxv Syv
enum : int { GM_MAX_SIDE = 8192 };                // W, H at most this: the bound of the integer sums (include/dfx.h)

static_assert(sizeof(dfx_gm_result) == 352 && offsetof(dfx_gm_result, work) == 248, "dfx_gm_result is a documented layout");

// n planar float32 flows of w x h pixels.  Flow i: u plane at flow + i * flow_stride, v plane plane_stride behind it, rows
// row_pitch apart (floats).  mask (may be nullptr), moving (may be nullptr): byte planes, plane i at + i * stride, pitch bytes
// per row.  out (may be nullptr; may be flow with flow's strides) lies as flow does with strides of its own.  result: n
// records, 8-byte aligned.
struct GmArgs {
    const float *flow;
    const unsigned char *mask;
    float *out;
    unsigned char *moving;
    dfx_gm_result *result;
    int n, w, h;
    int model, rounds;
    float thr, growth;
    long long row_pitch, plane_stride, flow_stride; // floats
    long long mask_pitch, mask_stride;              // bytes
    long long out_pitch, out_plane, out_stride;     // floats
    long long moving_pitch, moving_stride;          // bytes
};

// Enqueues on s: the zeroing of the n records, `rounds` accumulate launches (the last workgroup of a flow closes its round:
// no host synchronisation in between) and, where out or moving is asked for, the apply launch.  Nothing for n <= 0.  Every
// bound of include/dfx.h's dfx_global_motion_device is the caller's to check.
void gm_launch(hipStream_t s, const GmArgs &a);
