// tests/plane_warp_harness.cpp — the helpers denseflow_amd/csrc/flow_quad.h gained for the warp of typed planes (fq_nearest,
// fq_f16_to_f32, fq_bf16_to_f32, fq_load_elem, fq_sample_elem) compiled as plain C++ with -ffp-contract=off, the very text the
// kernels compile.  A stand-alone program, so that it also runs under -fsanitize=undefined,address with no preload: the float
// to int casts of fq_nearest and the tap addresses (the probe plane is a heap block of exactly its size) are what the
// sanitizers guard.  Driven by tests/test_plane_warp_cpu.py.  Everything is binary, in the machine's byte order.
//
// argv[1] = "half":    stdout: 65536 float32, fq_f16_to_f32 of every pattern, then 65536 float32, fq_bf16_to_f32 of every pattern
// argv[1] = "nearest": stdin: int32 w h border count, then count x {float32 px, py}
//                      stdout: count x int32 {inside, take, xn, yn}
// argv[1] = "sample":  stdin: int32 w h border elem count, then the w * h elements of a plane (DFX_ELEM_* elem), then
//                      count x {float32 px, py};  stdout: count x float32, fq_sample_elem where take and 0 elsewhere
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../denseflow_amd/csrc/flow_quad.h"

template <class T>
static bool get(std::vector<T> &v) {
    return v.empty() || std::fread(v.data(), sizeof(T), v.size(), stdin) == v.size();
}
template <class T>
static bool put(const std::vector<T> &v) {
    return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), stdout) == v.size();
}

template <int ELEM>
static void sample_all(const void *plane, int w, int h, int border, const std::vector<float> &pos, std::vector<float> &out) {
    for (size_t i = 0; i < out.size(); ++i) {
        const FqTap t = fq_tap(pos[2 * i], pos[2 * i + 1], w, h, border);
        out[i] = t.take ? fq_sample_elem<ELEM>(plane, w, t) : 0.0f;
    }
}

int main(int argc, char **argv) {
    if (argc != 2)
        return 2;
    if (!std::strcmp(argv[1], "half")) {
        std::vector<float> out(2 * 65536);
        for (unsigned b = 0; b < 65536; ++b) {
            out[b] = fq_f16_to_f32((unsigned short)b);
            out[65536 + b] = fq_bf16_to_f32((unsigned short)b);
        }
        return put(out) ? 0 : 2;
    }
    const bool near = !std::strcmp(argv[1], "nearest");
    if (!near && std::strcmp(argv[1], "sample"))
        return 2;
    std::vector<int32_t> head(near ? 4 : 5);
    if (!get(head) || head[0] <= 0 || head[1] <= 0 || head.back() < 0)
        return 2;
    const int w = head[0], h = head[1], border = head[2];
    const size_t count = (size_t)head.back();
    if (near) {
        std::vector<float> pos(2 * count);
        if (!get(pos))
            return 2;
        std::vector<int32_t> out(4 * count);
        for (size_t i = 0; i < count; ++i) {
            const FqNear t = fq_nearest(pos[2 * i], pos[2 * i + 1], w, h, border);
            out[4 * i] = t.inside, out[4 * i + 1] = t.take, out[4 * i + 2] = t.xn, out[4 * i + 3] = t.yn;
        }
        return put(out) ? 0 : 2;
    }
    const int elem = head[3];
    std::vector<unsigned char> plane((size_t)w * h * dfx_elem_bytes(elem));
    std::vector<float> pos(2 * count), out(count);
    if (!get(plane) || !get(pos))
        return 2;
    if (elem == DFX_ELEM_F32)
        sample_all<DFX_ELEM_F32>(plane.data(), w, h, border, pos, out);
    else if (elem == DFX_ELEM_F16)
        sample_all<DFX_ELEM_F16>(plane.data(), w, h, border, pos, out);
    else if (elem == DFX_ELEM_BF16)
        sample_all<DFX_ELEM_BF16>(plane.data(), w, h, border, pos, out);
    else
        return 2;
    return put(out) ? 0 : 2;
}
