// flow_median_kernels.h — launcher of the mask-aware median filter and occlusion fill of planar flows
// (flow_median_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "dfx.h"

enum : int { FM_ALL = 0, FM_FILL = 1 };  // = DFX_MEDIAN_ALL / DFX_MEDIAN_FILL of include/dfx.h
enum : int { FM_TILE_W = 64 };           // columns of a flow one workgroup owns (16 lanes of 4 pixels)
enum : int { FM_TILE_H = 16 };           // rows of a flow one workgroup owns (16 lane rows)

// n planar float32 flows of w x h pixels.  Flow i: u plane at flow + i * flow_stride, v plane plane_stride behind it, rows
// row_pitch apart (floats); out lies likewise with strides of its own and must not be flow.  mask (may be nullptr),
// mask_out (may be nullptr; needs mask): byte planes, plane i at + i * stride, pitch bytes per row.
struct FmArgs {
    const float *flow;
    const unsigned char *mask;
    float *out;
    unsigned char *mask_out;
    int n, w, h;
    int ksize, mode;
    long long row_pitch, plane_stride, flow_stride; // floats
    long long mask_pitch, mask_stride;              // bytes
    long long out_pitch, out_plane, out_stride;     // floats
    long long mask_out_pitch, mask_out_stride;      // bytes
};

// Enqueues on s one launch per 65535 flows.  Nothing for n <= 0.  Every bound of include/dfx.h's dfx_flow_median_device
// is the caller's to check.
void fm_launch(hipStream_t s, const FmArgs &a);
