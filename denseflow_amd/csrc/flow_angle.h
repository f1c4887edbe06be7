// flow_angle.h — the one angle of a flow vector: atan2(y, x) / pi in half-turns by the polynomial of section (0.5.1) of
// include/dfx.h, shared by the colour coding (flow_colour_kernels.hip) and the orientation histograms (flow_hist_kernels.hip).
// Plain C++, float32, every operation rounded on its own (the build's -ffp-contract=off): tests/flow_angle_harness.cpp compiles
// this very text on the CPU and tests/test_flow_angle_cpu.py holds it bit for bit against tests/flow_colour_ref.py's
// atan2_turns, the NumPy reference the kernels are tested with.
#pragma once

#include "dfx_device.h"

// atan2(y, x) / pi in half-turns: the polynomial of the text, signs from the sign bits so that +-0 behave as in IEEE atan2
DFX_HD float fv_atan2_turns(float y, float x) {
    const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
    const float mx = __builtin_fmaxf(ax, ay), mn = __builtin_fminf(ax, ay);
    const float t = mx > 0.0f ? mn / mx : 0.0f;
    const float s = t * t;
    float p = -0x1.81b21cp-7f;
    p = p * s + 0x1.b0bae2p-5f;
    p = p * s + -0x1.ddcd90p-4f;
    p = p * s + 0x1.8ca306p-3f;
    p = p * s + -0x1.54a3a4p-2f;
    p = p * s + 0x1.fffd5cp-1f;
    float r = t * p;
    if (ay > ax)
        r = 1.5707964f - r;
    if (__builtin_bit_cast(unsigned, x) >> 31)
        r = 3.1415927f - r;
    if (__builtin_bit_cast(unsigned, y) >> 31)
        r = -r;
    return r * 0.31830987f;
}
