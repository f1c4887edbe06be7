// tests/handover_harness.cpp — TEST INFRASTRUCTURE: C wrappers around denseflow_amd/csrc/dfx_handover.h (the HIP-free
// hand-over of a device batch to the caller's buffers, which the blocking path, the helper thread and the deferred
// tails of libdfx all run) so that tests/test_handover_cpu.py can drive it on the CPU.  Linked with jpeg_host.cpp.
#include <cstdio>

#include "../denseflow_amd/csrc/dfx_handover.h"

extern "C" {

// rows of `nb` pairs out of `block` into dst_a[j] (and dst_b[j] for two u8 planes), `pitch` bytes per destination row
int hh_rows(const unsigned char *block, int two_planes, int w, int h, size_t pitch, int nb, void **dst_a, void **dst_b) {
    DfxHandover d;
    d.block = block, d.two_planes = two_planes != 0, d.W = w, d.H = h, d.pitch = pitch;
    d.dst_a.assign(dst_a, dst_a + nb);
    if (two_planes)
        d.dst_b.assign(dst_b, dst_b + nb);
    std::string err;
    return dfx_hand_over(d, &err);
}

static DfxHandover files(const unsigned char *header, size_t header_len, const unsigned char *landing, int n,
                         const unsigned long long *bits, const unsigned long long *base, unsigned char **jpg,
                         uint32_t *sizes, size_t capacity) {
    DfxHandover d;
    d.header.assign(header, header + header_len);
    d.landing = landing, d.capacity = capacity;
    for (int j = 0; j < n; ++j) {
        d.coded.push_back({bits[j], base[j]});
        d.jpg.push_back(jpg ? jpg[j] : nullptr);
        d.size.push_back(sizes + j);
    }
    return d;
}

// n files out of `landing`; returns the status, the failure's text in msg
int hh_files(const unsigned char *header, size_t header_len, const unsigned char *landing, int n,
             const unsigned long long *bits, const unsigned long long *base, unsigned char **jpg, uint32_t *sizes,
             size_t capacity, char *msg, size_t msg_len) {
    std::string err;
    const int rc = dfx_hand_over(files(header, header_len, landing, n, bits, base, jpg, sizes, capacity), &err);
    snprintf(msg, msg_len, "%s", err.c_str());
    return rc;
}

int hh_may_not_fit(size_t header_len, int n, const unsigned long long *bits, size_t capacity) {
    const std::vector<unsigned char> header(header_len);
    std::vector<unsigned long long> base(n, 0);
    std::vector<uint32_t> sizes(n);
    return dfx_may_not_fit(files(header.data(), header_len, nullptr, n, bits, base.data(), nullptr, sizes.data(), capacity));
}

// jpeg_assemble called directly: what every file of hh_files must equal
size_t hh_assemble(const unsigned char *header, size_t header_len, const unsigned char *src, unsigned long long bits,
                   unsigned char *dst, size_t capacity) {
    return jpeg_assemble(std::vector<unsigned char>(header, header + header_len), src, bits, dst, capacity);
}
}
