// farn_window_taps_harness.cpp — the engine's own Gaussian-window taps (farn_window_taps, denseflow_amd/csrc/engine_plan.h:
// pure host arithmetic) behind a C entry point, for tests/test_farneback_window_ref.py.
#include "../denseflow_amd/csrc/engine_plan.h"

extern "C" int fwt_window_taps(int win_size, float *out16) {
    FarnWinTaps t;
    if (!farn_window_taps(win_size, t))
        return -1;
    for (int i = 0; i < 16; ++i)
        out16[i] = t.g[i];
    return 0;
}
