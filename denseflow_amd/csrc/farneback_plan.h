// farneback_plan.h — pure host logic of the -a=farn launches (no HIP): how the row-stream iteration kernel's column
// strips are cut into segments of rows.  Plain C++ so that the CPU tests compile the very function the launcher uses
// (tests/plan_harness.cpp, tests/test_plan_logic.py).
#pragma once

#include <algorithm>

#ifndef FARN_STREAM_GENERATIONS
#define FARN_STREAM_GENERATIONS 16
#endif

constexpr int kFarnStreamStripCols = 64; // output columns per workgroup
constexpr int kFarnStreamStepRows = 6;   // rows a workgroup advances per step
constexpr int kFarnStreamMinSegRows = 48; // the floor for the reference's window (half-width 6)
constexpr int kFarnStreamSlots = 256 * 4; // workgroups the machine holds at once: 256 CUs x 4
// box half-widths (winSize / 2) the row-stream kernel is built for: winSize 7 .. 21.  Its work split puts one step's
// updateMatrices items, 6 x (32 + half) column pairs, and one vertical-sum column per lane on 256 lanes: half <= 10.
constexpr int kFarnStreamHalfMin = 3, kFarnStreamHalfMax = 10;
inline bool farn_stream_has_half(int half) { return half >= kFarnStreamHalfMin && half <= kFarnStreamHalfMax; }

// The Gaussian update window (dfx_params.farn_window = DFX_FARN_WINDOW_GAUSSIAN): the non-negative half of
// getGaussianKernel(winSize, (winSize / 2) * 0.3f), g[0] the centre (farn_window_taps, engine_plan.h).  Handed to the
// iteration kernels by value: the taps are uniform and live in scalar registers.  16 = half-widths up to 15 (winSize 31).
struct FarnWinTaps {
    float g[16];
};

// The shortest segment worth its warm-up: a segment recomputes the 2 * half rows above and below it (its window's
// first rows, and the rows its last outputs need), so the floor is four times that, in whole steps — 48 rows at half 6.
inline int farn_stream_min_seg_rows(int half) {
    return (8 * half + kFarnStreamStepRows - 1) / kFarnStreamStepRows * kFarnStreamStepRows;
}

// Rows per segment: whole 6-row steps, and enough segments that a launch is many generations of workgroups — a workgroup
// walks its whole segment, so with few generations the last, nearly empty one costs a full segment time (one segment per
// column at 1080p is 3.02 generations: measured 1130 us per launch against 1000 with >= 8).  Each segment pays 2 * half
// warm-up rows (12 at the reference's window), hence the floor of farn_stream_min_seg_rows(half) rows (48).  The
// segments [k * rows, min((k + 1) * rows, h)) partition the level's rows.
inline int farn_stream_seg_rows(int w, int h, int n_pairs, int half = 6) {
    const long long cols = (w + kFarnStreamStripCols - 1) / kFarnStreamStripCols;
    const long long wgs_per_seg = std::max<long long>(cols * std::max(n_pairs, 1), 1);
    long long nseg = ((long long)FARN_STREAM_GENERATIONS * kFarnStreamSlots + wgs_per_seg - 1) / wgs_per_seg;
    nseg = std::max<long long>(1, std::min<long long>(nseg, h / farn_stream_min_seg_rows(half))); // no segment under the floor
    const int rows = (int)((h + nseg - 1) / nseg);
    return (rows + kFarnStreamStepRows - 1) / kFarnStreamStepRows * kFarnStreamStepRows;
}
