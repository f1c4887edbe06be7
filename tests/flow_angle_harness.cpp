// tests/flow_angle_harness.cpp — the angle of the colour coding and of the orientation histograms
// (denseflow_amd/csrc/flow_angle.h: fv_atan2_turns) compiled as plain C++ with -ffp-contract=off, the very text the kernels
// compile.  A stand-alone program, so that it also runs under -fsanitize=undefined with no preload.  Driven by
// tests/test_flow_angle_cpu.py.
//
// stdin:  binary, pairs of float32 (y, x) until the end of input
// stdout: binary, one float32 per pair: fv_atan2_turns(y, x)
#include <cstdio>
#include <vector>

#include "../denseflow_amd/csrc/flow_angle.h"

int main() {
    std::vector<float> in(1 << 16), out(1 << 15);
    for (;;) {
        const size_t got = std::fread(in.data(), 2 * sizeof(float), in.size() / 2, stdin);
        if (got == 0)
            break;
        for (size_t i = 0; i < got; ++i)
            out[i] = fv_atan2_turns(in[2 * i], in[2 * i + 1]);
        if (std::fwrite(out.data(), sizeof(float), got, stdout) != got)
            return 2;
    }
    return 0;
}
