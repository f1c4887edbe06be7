// jpeg_device_common.h — the parts of the device JPEG encoder that the gray form (jpeg_kernels.hip) and the colour form
// (jpeg_colour_kernels.hip) share: the bit emitter, the per-stream scan of block bit counts, the layout of the streams in
// the shared buffer and its zero-fill.  Device code only; included by those two files.
#pragma once

#include <hip/hip_runtime.h>

#include "jpeg_kernels.h"

namespace {

__device__ __forceinline__ int bit_length(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }

struct Emitter { // MSB-first bit string appended at an arbitrary bit position of a zeroed big-endian word stream
    unsigned *words;
    unsigned long long acc; // pending bits, left-aligned
    int nacc;               // number of pending bits (< 32 between puts)
    __device__ __forceinline__ void begin(unsigned *stream, unsigned long long bitpos) {
        words = stream + (bitpos >> 5);
        nacc = (int)(bitpos & 31); // the first word is shared with the previous block: its leading bits stay zero here
        acc = 0;
    }
    __device__ __forceinline__ void put(unsigned code, int len) { // len <= 27
        acc |= (unsigned long long)(code & ((1u << len) - 1u)) << (64 - nacc - len);
        nacc += len;
        if (nacc >= 32) {
            atomicOr(words, __builtin_bswap32((unsigned)(acc >> 32)));
            ++words;
            acc <<= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void end() {
        if (nacc > 0)
            atomicOr(words, __builtin_bswap32((unsigned)(acc >> 32)));
    }
};

// Blocks of one stream (a gray plane / a colour frame) and, in a colour frame's MCU order (Y00 Y01 Y10 Y11 Cb Cr per
// MCU), the block that holds the DC predictor of block b: the previous block of the same component (-1: predictor 0).
__device__ __forceinline__ int jpeg_stream_blocks(const JpegCtx &c) { return c.bw * c.bh; }
__device__ __forceinline__ int jpeg_stream_blocks(const JpegColourCtx &c) { return c.mcus_x * c.mcus_y * 6; }
__device__ __forceinline__ int jpeg_colour_pred_block(int b) {
    const int k = b % 6;
    if (k >= 1 && k <= 3)
        return b - 1;
    if (b < 6)
        return -1;
    return k == 0 ? b - 3 : b - 6;
}

// One workgroup per stream: bits of every block (DC difference code + AC codes) and their exclusive prefix sum.
template <class Ctx, bool COLOUR>
__global__ __launch_bounds__(1024) void k_jpeg_scan(Ctx c) {
    __shared__ unsigned wave_sum[16];
    __shared__ unsigned long long running;
    const int plane = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nblk = jpeg_stream_blocks(c);
    const short *dc = c.dc + (long long)plane * nblk;
    unsigned *bits = c.bits + (long long)plane * nblk;
    if (tid == 0)
        running = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nblk; b0 += 1024) {
        const int b = b0 + tid;
        unsigned v = 0;
        if (b < nblk) {
            const int pb = COLOUR ? jpeg_colour_pred_block(b) : b - 1;
            const JpegTables &T = c.tab[COLOUR && b % 6 >= 4 ? 1 : 0];
            const int diff = (int)dc[b] - (pb >= 0 ? (int)dc[pb] : 0);
            const int nb = bit_length(diff < 0 ? -diff : diff);
            v = (unsigned)T.dc_len[nb] + (unsigned)nb + bits[b];
        }
        unsigned incl = v; // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned o = __shfl_up(incl, off, 64);
            if (lane >= off)
                incl += o;
        }
        if (lane == 63)
            wave_sum[wave] = incl;
        __syncthreads();
        unsigned before = 0;
        for (int i = 0; i < wave; ++i)
            before += wave_sum[i];
        const unsigned long long base = running;
        if (b < nblk) {
            const unsigned long long off = base + before + incl - v;
            bits[b] = (unsigned)off; // < 2^32: a stream's segment is at most blocks x 1728 bits
        }
        __syncthreads();
        if (tid == 1023)
            running = base + before + incl;
        __syncthreads();
    }
    if (tid == 0)
        c.plane_bits[plane] = running;
}

// One thread: where every stream starts (4-byte aligned: the emit pass ORs whole words), totals for the host.
template <class Ctx>
__global__ void k_jpeg_layout(Ctx c) {
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    const int n = c.n_planes;
    unsigned long long at = 0;
    for (int p = 0; p < n; ++p) {
        const unsigned long long bits = c.plane_bits[p];
        c.plane_base[p] = at;
        c.info[2 + 2 * p] = bits;
        c.info[2 + 2 * p + 1] = at;
        at += ((bits + 31) >> 5) << 2;
    }
    c.hdr[0] = c.info[0] = at;
    c.hdr[1] = c.info[1] = at > c.capacity_bytes ? 1ull : 0ull;
    __threadfence_system();
}

// Zero the part of the shared buffer the emit pass will OR into.
template <class Ctx>
__global__ __launch_bounds__(256) void k_jpeg_zero(Ctx c) {
    if (c.hdr[1] != 0)
        return;
    const unsigned long long words = c.hdr[0] >> 2;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < words; i += (unsigned long long)gridDim.x * 256)
        c.stream[i] = 0u;
}

} // namespace
