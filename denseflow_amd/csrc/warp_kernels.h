// warp_kernels.h — launcher of the backward warp of 8-bit images by a flow, with its photometric statistics
// (warp_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

enum : int { WARP_BORDER_ZERO = 0, WARP_BORDER_CLAMP = 1 }; // = DFX_WARP_BORDER_* of include/dfx.h
enum : int { WARP_OUT_U8 = 3 };                             // = DFX_WARP_U8; 0 .. 2 are DFX_ELEM_F32 / _F16 / _BF16
enum : int { WARP_STATS_ROWS = 32 };                        // rows of an image one workgroup of the statistics form covers

// n images of w x h pixels and `channels` (1 or 3) bytes per pixel, sampled at the positions n planar float32 flows name.
// Image i is at src + i * src_image; interleaved (channels == 3 && !planar): pixel (x, y) channel c at y * src_pitch + 3 * x
// + c; otherwise channel c is a plane at c * src_plane, rows src_pitch apart (bytes).  ref (may be nullptr) lies as src does.
// Flow i: u plane at flow + i * flow_stride, v plane plane_stride behind it, rows row_pitch apart (floats).  out (may be
// nullptr) lies as src does with strides of its own, in elements of out_dtype.  occ (may be nullptr) and valid (may be
// nullptr) are byte planes, plane i at + i * stride, pitch bytes per row.  stats (may be nullptr; needs ref): {count, sad} of
// image i at stats[2 * i], stats[2 * i + 1].
struct WarpArgs {
    const unsigned char *src, *ref;
    const float *flow;
    void *out;
    const unsigned char *occ;
    unsigned char *valid;
    unsigned long long *stats;
    int n, w, h;
    int channels, planar, border, out_dtype;
    long long src_pitch, src_plane, src_image;      // bytes
    long long row_pitch, plane_stride, flow_stride; // floats
    long long out_pitch, out_plane, out_image;      // elements of out_dtype
    long long occ_pitch, occ_stride;                // bytes
    long long valid_pitch, valid_stride;            // bytes
};

// Enqueues on s: the zeroing of the n statistics pairs (where asked for), then the warp (nothing for n <= 0).  Every bound
// of include/dfx.h's dfx_warp_device is the caller's to check.
void warp_launch(hipStream_t s, const WarpArgs &a);
