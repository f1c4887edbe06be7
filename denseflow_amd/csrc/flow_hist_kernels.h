// flow_hist_kernels.h — launcher of the motion descriptors of flows: HOF / MBHx / MBHy cell histograms (flow_hist_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

enum : int { FH_KIND_HOF = 1, FH_KIND_MBHX = 2, FH_KIND_MBHY = 4 };                 // = DFX_HIST_* of include/dfx.h
enum : int { FH_NORM_NONE = 0, FH_NORM_L1 = 1, FH_NORM_L1_SQRT = 2, FH_NORM_L2 = 3 }; // = DFX_HIST_NORM_* of include/dfx.h
enum : int { FH_MAX_BINS = 16, FH_MAX_SLOTS = 3 * FH_MAX_BINS + 1 };                  // 49 slots: HOF's still slot is the one more

// slots of a cell under `kinds` and `bins`: HOF bins + 1, MBHX bins, MBHY bins, in that order
static inline int fh_slots(int kinds, int bins) {
    return ((kinds & FH_KIND_HOF) ? bins + 1 : 0) + ((kinds & FH_KIND_MBHX) ? bins : 0) + ((kinds & FH_KIND_MBHY) ? bins : 0);
}

// n planar float32 flows (flow i: a u plane at flow + i * flow_stride, its v plane plane_stride behind it, rows row_pitch
// apart, in floats: the layout of dfx_calc_batch_planar_device), optionally n mask planes (mask i at mask + i * mask_stride,
// mask_pitch bytes per row; nonzero = not here), and one or both outputs: the integer sums, dense (CH, CW, D) per flow and
// sums_stride words between flows, and the float values, element (flow i, slot b, cell row cy, cell column cx) at
// out + i * out_flow + b * out_slot + cy * out_row + cx * out_col.
struct FhArgs {
    const float *flow;
    const unsigned char *mask; // may be nullptr
    long long *sums;           // may be nullptr
    float *out;                // may be nullptr (not both)
    int n, w, h;
    int i0;                    // the launch's first flow (set by the launcher: grid.z holds at most 65535 of them)
    long long row_pitch, plane_stride, flow_stride;     // floats
    long long mask_pitch, mask_stride;                  // bytes
    long long sums_stride;                              // 64-bit words
    long long out_slot, out_col, out_row, out_flow;     // floats
    int kinds;                 // FH_KIND_* bits, 1 .. 7
    int bins;                  // 2 .. 16
    int cell;                  // 4, 8, 16 or 32
    int norm;                  // FH_NORM_*
    float still_thr;           // HOF: m <= still_thr goes to the still slot; negative: never
    // set by the launcher
    int cell_log2, cw, ch, d, bands;
    int wide_flow, wide_mask;  // a lane's 4 elements in one access
};

// Enqueues on s (nothing for n <= 0): one launch per 65535 flows does everything.  Every bound of include/dfx.h's
// dfx_flow_hist_device is the caller's to check.
void fh_launch(hipStream_t s, const FhArgs &a);
