// flow_project_kernels.h — launcher of the forward projection (splat) of planar flows with integer sums
// (flow_project_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "flow_scatter.h"

enum : int { FP_WORDS = 3 }; // 64-bit words per pixel of the workspace: Wsum, Su, Sv, in that order, pixel after pixel

// The flows, imp, occ, hole, cov and work of FsSource (flow_scatter.h; work: FP_WORDS * w * h words per flow of a wave,
// flows_per_wave flows), and out (may be nullptr), laid out as the flows are with strides of its own.
struct FpArgs : FsSource {
    float *out;
    double sc;                                  // (double)scale / 256.0
    long long out_pitch, out_plane, out_stride; // floats
};

// Enqueues on s, per wave of min(flows_per_wave, 65535) flows: zero the wave's words, scatter, normalise.  Nothing for
// n <= 0.  Every bound of include/dfx.h's dfx_flow_project_device is the caller's to check.
void fp_launch(hipStream_t s, const FpArgs &a, long long flows_per_wave);

// Enqueues on s the normalising pass alone, over the sums a preceding fp_launch of the same flows left in work: the same
// projection under another scale (sc) into other planes.  That fp_launch must have taken its n <= 65535 flows as one wave.
void fp_renormalise(hipStream_t s, const FpArgs &a);
