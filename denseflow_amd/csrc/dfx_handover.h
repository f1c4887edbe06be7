// dfx_handover.h — the hand-over of one device batch to the caller's buffers: rows from a page-locked bounce block to the
// caller's flows / planes, and entropy-coded segments from a landing buffer to JPEG files.  Pure C++ (no HIP): compiled
// into dfx_pipeline.cpp, dfx_frames.cpp and dfx_api.cpp and, for the CPU suite, into tests/handover_harness.cpp
// (tests/test_handover_cpu.py).  The blocking path, the handle's helper thread and the deferred tails all run
// dfx_hand_over on a DfxHandover, which owns copies of that batch's destination pointers: the caller's pointer arrays
// need not outlive a submit call.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dfx.h"

// jpeg_host.cpp (declared in jpeg_kernels.h, which needs HIP): header + byte-stuffed segment + EOI; 0 = does not fit
size_t jpeg_assemble(const std::vector<unsigned char> &header, const unsigned char *src, unsigned long long bits,
                     unsigned char *dst, size_t capacity);

struct DfxCodedPlane { // what the device reports per coded plane / frame
    unsigned long long bits, base; // bits of the entropy-coded segment, its first byte in the landing buffer
};

struct DfxHandover {
    // rows: dst_a.size() pairs in `block` (null: none).  Float: pair j is H rows of W (u, v) pairs at j * W * H * 8 -> dst_a[j].
    // Two u8 planes: x plane j at j * W * H -> dst_a[j], y plane j at (pairs + j) * W * H -> dst_b[j].
    // Float planes: u plane of pair j at j * W * H * 2 * elem_bytes -> dst_a[j], its v plane W * H * elem_bytes behind ->
    // dst_b[j] (elem_bytes: 4, or 2 for float16 / bfloat16 planes).
    const unsigned char *block = nullptr;
    bool two_planes = false, float_planes = false;
    size_t elem_bytes = 4;
    int W = 0, H = 0;
    size_t pitch = 0; // bytes per destination row
    std::vector<void *> dst_a, dst_b;
    // files: coded[j] of `landing` becomes file j in jpg[j] (capacity bytes each), its size in *size[j]
    std::vector<unsigned char> header;
    const unsigned char *landing = nullptr;
    std::vector<DfxCodedPlane> coded;
    std::vector<unsigned char *> jpg;
    std::vector<uint32_t *> size;
    size_t capacity = 0;
    const char *too_small = "JPEG: jpg_capacity is too small for an encoded plane"; // the text of that failure
};

// A file that could exceed the capacity if every byte of its segment had to be stuffed (above 4 bits per pixel against
// dfx_jpeg_capacity: noise).  Such a batch is handed over synchronously: "does not fit" is then DFX_ERR_UNSUPPORTED from
// the submit call — the status that means "encode this on the host" — and never an error of a deferred tail, which the
// host shell could only treat as fatal.
inline bool dfx_may_not_fit(const DfxHandover &h) {
    for (const DfxCodedPlane &p : h.coded)
        if (h.header.size() + 2 * (size_t)((p.bits >> 3) + 1) + 2 > h.capacity)
            return true;
    return false;
}

inline void dfx_copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t row_bytes, int rows) {
    if (dpitch == row_bytes && spitch == row_bytes)
        std::memcpy(dst, src, row_bytes * rows);
    else
        for (int y = 0; y < rows; ++y)
            std::memcpy((char *)dst + (size_t)y * dpitch, (const char *)src + (size_t)y * spitch, row_bytes);
}

inline int dfx_hand_over(const DfxHandover &h, std::string *err) {
    const size_t plane = (size_t)h.W * h.H, nb = h.dst_a.size();
    for (size_t j = 0; h.block && j < nb; ++j) {
        if (h.float_planes) {
            const size_t e = h.elem_bytes, rb = (size_t)h.W * e;
            dfx_copy_rows(h.dst_a[j], h.pitch, h.block + j * plane * 2 * e, rb, rb, h.H);
            dfx_copy_rows(h.dst_b[j], h.pitch, h.block + j * plane * 2 * e + plane * e, rb, rb, h.H);
        } else if (h.two_planes) {
            dfx_copy_rows(h.dst_a[j], h.pitch, h.block + j * plane, (size_t)h.W, (size_t)h.W, h.H);
            dfx_copy_rows(h.dst_b[j], h.pitch, h.block + (nb + j) * plane, (size_t)h.W, (size_t)h.W, h.H);
        } else {
            dfx_copy_rows(h.dst_a[j], h.pitch, h.block + j * plane * 8, (size_t)h.W * 8, (size_t)h.W * 8, h.H);
        }
    }
    for (size_t j = 0; j < h.coded.size(); ++j) {
        const size_t n = jpeg_assemble(h.header, h.landing + h.coded[j].base, h.coded[j].bits, h.jpg[j], h.capacity);
        if (n == 0) {
            *err = h.too_small;
            return DFX_ERR_UNSUPPORTED;
        }
        *h.size[j] = (uint32_t)n;
    }
    return DFX_OK;
}
