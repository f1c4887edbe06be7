// flow_scatter.hip — the zero pass of the integer scatter (flow_scatter.h): the words of a wave of items, before its adds.
#include <hip/hip_runtime.h>

#include "flow_scatter.h"

namespace {

__global__ __launch_bounds__(256) void k_fs_zero(fs_u64 *work, long long words) {
    // head: one word where the base is 8 mod 16; then pairs; then at most one trailing word
    const long long head = (((size_t)work & 15) != 0 && words > 0) ? 1 : 0;
    const long long pairs = (words - head) / 2;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    ulonglong2 *q = reinterpret_cast<ulonglong2 *>(work + head);
    for (long long i = tid; i < pairs; i += step)
        q[i] = make_ulonglong2(0ull, 0ull);
    if (tid == 0) {
        if (head)
            work[0] = 0ull;
        if (head + 2 * pairs < words)
            work[words - 1] = 0ull;
    }
}

} // namespace

void fs_zero(hipStream_t s, fs_u64 *work, long long words) {
    const unsigned blocks = (unsigned)std::min<long long>((words / 2 + 255) / 256 + 1, 8192);
    hipLaunchKernelGGL(k_fs_zero, dim3(blocks), dim3(256), 0, s, work, words);
}
