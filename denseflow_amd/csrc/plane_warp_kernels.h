// plane_warp_kernels.h — launcher of the backward warp of float, half and label planes by a flow (plane_warp_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

enum : int { PW_BORDER_ZERO = 0, PW_BORDER_CLAMP = 1 };     // = DFX_WARP_BORDER_* of include/dfx.h
enum : int { PW_SAMPLE_BILINEAR = 0, PW_SAMPLE_NEAREST = 1 }; // = DFX_SAMPLE_*
enum : int { PW_INVALID_ZERO = 0, PW_INVALID_KEEP = 1 };    // = DFX_WARP_INVALID_*
enum : int { PW_ELEM_U8 = 3 };                              // = DFX_WARP_U8; 0 .. 2 are DFX_ELEM_F32 / _F16 / _BF16

// n images of w x h pixels and `channels` elements per pixel, sampled at the positions n planar float32 flows name.  Image
// i is at src + i * src_image; planar: channel c is a plane at c * src_plane, rows src_pitch apart; interleaved: pixel
// (x, y) channel c at y * src_pitch + channels * x + c.  All of these in elements of src_dtype.  Flow i: u plane at flow +
// i * flow_stride, v plane plane_stride behind it, rows row_pitch apart (floats).  out (may be nullptr) lies as src does with
// strides of its own, in elements of out_dtype.  occ (may be nullptr) and valid (may be nullptr) are byte planes, plane i at
// + i * stride, pitch bytes per row.
struct PwArgs {
    const void *src;
    const float *flow;
    void *out;
    const unsigned char *occ;
    unsigned char *valid;
    int n, w, h;
    int channels, planar, border, sample, keep, src_dtype, out_dtype;
    long long src_pitch, src_plane, src_image;      // elements of src_dtype
    long long row_pitch, plane_stride, flow_stride; // floats
    long long out_pitch, out_plane, out_image;      // elements of out_dtype
    long long occ_pitch, occ_stride;                // bytes
    long long valid_pitch, valid_stride;            // bytes
};

// Enqueues the warp on s (nothing for n <= 0).  Every bound of include/dfx.h's dfx_warp_planes_device is the caller's to
// check.
void pw_launch(hipStream_t s, const PwArgs &a);
