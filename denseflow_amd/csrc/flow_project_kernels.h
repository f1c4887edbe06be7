// flow_project_kernels.h — launcher of the forward projection (splat) of planar flows with integer sums
// (flow_project_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

enum : int { FP_WORDS = 3 }; // 64-bit words per pixel of the workspace: Wsum, Su, Sv, in that order, pixel after pixel

// Planar float32 flows of w x h pixels.  Flow i: u plane at flow + i * flow_stride, v plane plane_stride behind it, rows
// row_pitch apart (floats).  imp (may be nullptr): one float plane per flow; occ (may be nullptr): one byte plane per flow.
// out (may be nullptr) is laid out as the flows are with strides of its own; hole (bytes) and cov (floats) are one plane per
// flow, each may be nullptr.  work: FP_WORDS * w * h words per flow of a wave, flows_per_wave flows; 8-byte aligned.
struct FpArgs {
    const float *flow;
    const float *imp;
    const unsigned char *occ;
    float *out;
    unsigned char *hole;
    float *cov;
    unsigned long long *work;
    int n, w, h;
    float t;                 // px = x + t * fu
    double sc;               // (double)scale / 256.0
    unsigned long long wmin; // hole = Wsum < wmin; >= 1
    long long row_pitch, plane_stride, flow_stride; // floats
    long long imp_pitch, imp_stride;                // floats
    long long occ_pitch, occ_stride;                // bytes
    long long out_pitch, out_plane, out_stride;     // floats
    long long hole_pitch, hole_stride;              // bytes
    long long cov_pitch, cov_stride;                // floats
};

// FpArgs::wmin of a min_weight: max(1, llrint(min_weight * 2^24)), at most 2^63 (a min_weight no sum can reach makes every
// pixel a hole).
inline unsigned long long fp_wmin(float min_weight) {
    const double m = (double)min_weight * 16777216.0;
    return m >= 9223372036854775808.0 ? (1ull << 63) : std::max<unsigned long long>(1ull, (unsigned long long)std::llrint(m));
}

// Enqueues on s, per wave of min(flows_per_wave, 65535) flows: zero the wave's words, scatter, normalise.  Nothing for
// n <= 0.  Every bound of include/dfx.h's dfx_flow_project_device is the caller's to check.
void fp_launch(hipStream_t s, const FpArgs &a, long long flows_per_wave);

// Enqueues on s the normalising pass alone, over the sums a preceding fp_launch of the same flows left in work: the same
// projection under another scale (sc) into other planes.  That fp_launch must have taken its n <= 65535 flows as one wave.
void fp_renormalise(hipStream_t s, const FpArgs &a);
