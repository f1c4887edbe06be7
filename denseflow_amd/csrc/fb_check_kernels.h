// fb_check_kernels.h — launcher of the forward-backward consistency check (fb_check_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

// One direction of a launch: n planar float32 flows F and the n flows B they are checked against, the n mask planes and
// (optionally) the n err planes the check writes.  Flow i of either array is a u plane at + i * flow_stride and a v plane
// plane_stride behind it, rows row_pitch apart (floats: the layout of dfx_calc_batch_planar_device); mask plane i is at
// occ + i * occ_stride, occ_pitch bytes per row; err plane i at err + i * err_stride, err_pitch floats per row.
struct FbCheckDir {
    const float *f, *b;
    unsigned char *occ;
    float *err; // may be nullptr: no err plane
};

// A launch covers dirs x n flows: direction 0 checks (F, B), direction 1 — the bidirectional entry point's second half —
// whatever its own four pointers name (there: (B, F) into the backward mask).  The strides are common to both.
struct FbCheckArgs {
    FbCheckDir dir[2];
    int dirs; // 1 or 2
    int n, w, h;
    long long row_pitch, plane_stride, flow_stride; // floats
    long long occ_pitch, occ_stride;                // bytes
    long long err_pitch, err_stride;                // floats
    float alpha1, alpha2;
};

// Enqueues the check on s (nothing for n <= 0).  Every bound of include/dfx.h's dfx_fb_check_device is the caller's to check.
void fb_check_launch(hipStream_t s, const FbCheckArgs &a);
