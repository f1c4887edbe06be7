// tests/flow_quad_harness.cpp — the bilinear tap of the flow post-processing kernels (denseflow_amd/csrc/flow_quad.h: fq_tap,
// fq_lerp, fq_sample_f32, fq_sample_u8) compiled as plain C++ with -ffp-contract=off, the very text the kernels compile.  A
// stand-alone program, so that it also runs under -fsanitize=undefined,address with no preload: the float to int casts of
// fq_tap and the tap addresses (every probe buffer is a heap block of exactly its size) are what the sanitizers guard.
// Driven by tests/test_flow_quad_cpu.py.
//
// stdin:  w h border
//         w * h * 3 bytes (decimal): a probe image, interleaved
//         2 * w * h float32 bit patterns (hex): two probe planes
//         then positions until the end of input, one per line: the bit patterns (hex) of px and py
// stdout: per position one line: inside take x0 x1 y0 y1 ax ay | the samples of the image as gray (channel 0 alone), interleaved
//         (3) and planar (3) | the samples of the two float planes; floats as hex bit patterns, samples 0 without take, as
//         in the kernels
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../denseflow_amd/csrc/flow_quad.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
static uint32_t bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

int main() {
    int w, h, border;
    if (std::scanf("%d %d %d", &w, &h, &border) != 3 || w <= 0 || h <= 0)
        return 2;
    const size_t hw = (size_t)w * h;
    std::vector<unsigned char> il(hw * 3), planar(hw * 3), gray(hw);
    for (size_t i = 0; i < hw * 3; ++i) {
        unsigned v;
        if (std::scanf("%u", &v) != 1)
            return 2;
        il[i] = (unsigned char)v;
        planar[(i % 3) * hw + i / 3] = (unsigned char)v;
        if (i % 3 == 0)
            gray[i / 3] = (unsigned char)v;
    }
    std::vector<float> planes(2 * hw);
    for (size_t i = 0; i < 2 * hw; ++i) {
        unsigned b;
        if (std::scanf("%x", &b) != 1)
            return 2;
        planes[i] = from_bits(b);
    }
    unsigned bx, by;
    while (std::scanf("%x %x", &bx, &by) == 2) {
        const FqTap t = fq_tap(from_bits(bx), from_bits(by), w, h, border);
        float g[1] = {0.0f}, si[3] = {0.0f, 0.0f, 0.0f}, sp[3] = {0.0f, 0.0f, 0.0f}, su = 0.0f, sv = 0.0f;
        if (t.take) {
            fq_sample_u8<1, false>(gray.data(), w, 0, t, g);
            fq_sample_u8<3, true>(il.data(), 3LL * w, 0, t, si);
            fq_sample_u8<3, false>(planar.data(), w, (long long)hw, t, sp);
            su = fq_sample_f32(planes.data(), w, t);
            sv = fq_sample_f32(planes.data() + hw, w, t);
        }
        std::printf("%d %d %d %d %d %d %08x %08x | %08x %08x %08x %08x %08x %08x %08x | %08x %08x\n", (int)t.inside, (int)t.take,
                    t.x0, t.x1, t.y0, t.y1, bits(t.ax), bits(t.ay), bits(g[0]), bits(si[0]), bits(si[1]), bits(si[2]), bits(sp[0]),
                    bits(sp[1]), bits(sp[2]), bits(su), bits(sv));
    }
    return 0;
}
