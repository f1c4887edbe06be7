// jpeg_colour_kernels.hip — baseline JPEG of BGR frames on the device: YCbCr 4:2:0, one interleaved scan.
//
// Replaces the reference's colour frame extraction, `imencode(".jpg", frame)` of every BGR frame in
// DenseFlow::extract_frames_only (/root/reference/src/denseflow_gpu.cpp:82-105, the -s=0 mode).  Output is byte-identical
// to libjpeg(-turbo)'s — the library behind cv::imencode — and to the shell's host encoder (src/image_io.cpp:
// imencodeJpegColour); pinned in tests/test_jpeg_colour_pin.py and tests/test_extract_frames_gpu.py.
//
// The three-pass shape of the gray encoder (jpeg_kernels.hip: count -> scan -> layout -> zero -> emit), with the colour
// front end fused into the transform pass so that no YCbCr plane goes to HBM:
//   k_jpeg_colour_blocks   one workgroup takes up to 32 consecutive MCUs (16 x 16 pixels each) of one MCU row.
//     stage 1: the strip's BGR rows are read as aligned dwords (4 pixels = 3 dwords), converted with libjpeg's jccolor.c
//              fixed-point sums; Y goes to LDS at full resolution, Cb / Cr through h2v2_downsample (jcsample.c: four
//              samples + bias 1, 2, 1, 2 ... along the row, >> 2).  libjpeg's edge rules: the right column is replicated
//              up to the padded width BEFORE downsampling; an odd last row is replicated to a row pair; below the image
//              the DOWNSAMPLED last row is repeated (jcprepct.c pads the output of the downsampler, not its input).
//     stage 2: one thread per block (6 per MCU: Y00 Y01 Y10 Y11 Cb Cr), JDCT_ISLOW + reciprocal quantisation with the
//              component's table, then the gray encoder's count / emit code with the component's Huffman pair.
//              A Y block that lies wholly outside the image is one of libjpeg's dummy blocks (jccoefct.c:
//              compress_data): no AC, and the DC of the block before it in the MCU — a zero difference + EOB.
//   k_jpeg_scan<., true>   DC differences against the previous block OF THE SAME COMPONENT in MCU order, prefix sum.
#include <hip/hip_runtime.h>

#include "../../include/dfx_jpeg_tables.h"
#include "jpeg_device_common.h"
#include "jpeg_kernels.h"

namespace {

constexpr int CJ_MCUS = 32;              // MCUs per workgroup
constexpr int CJ_THREADS = CJ_MCUS * 6;  // one thread per block: 3 waves

// Four consecutive BGR pixels of a row starting at pixel x (a multiple of 4; the row is 4-byte aligned), each packed as
// B | G << 8 | R << 16.  Inside the image: three dwords.  At the right edge: bytes, the last column replicated.
__device__ __forceinline__ void load4_bgr(const unsigned char *row, int x, int w, unsigned p[4]) {
    if (x + 4 <= w) {
        const unsigned *d = reinterpret_cast<const unsigned *>(row + 3 * x);
        const unsigned d0 = d[0], d1 = d[1], d2 = d[2];
        p[0] = d0 & 0xFFFFFFu;
        p[1] = (d0 >> 24) | ((d1 & 0xFFFFu) << 8);
        p[2] = (d1 >> 16) | ((d2 & 0xFFu) << 16);
        p[3] = d2 >> 8;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned char *q = row + 3 * min(x + i, w - 1);
            p[i] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
        }
    }
}
__device__ __forceinline__ int px_b(unsigned p) { return (int)(p & 255u); }
__device__ __forceinline__ int px_g(unsigned p) { return (int)((p >> 8) & 255u); }
__device__ __forceinline__ int px_r(unsigned p) { return (int)((p >> 16) & 255u); }

__device__ __forceinline__ unsigned y4(const unsigned p[4]) { // four Y samples, packed little-endian
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        v |= (unsigned)DFX_JPEG_YCC_Y(px_r(p[i]), px_g(p[i]), px_b(p[i])) << (8 * i);
    return v;
}
// h2v2_downsample of pixels (a, b) of the upper and lower row
__device__ __forceinline__ int cb2(unsigned a0, unsigned a1, unsigned b0, unsigned b1, int bias) {
    return (DFX_JPEG_YCC_CB(px_r(a0), px_g(a0), px_b(a0)) + DFX_JPEG_YCC_CB(px_r(a1), px_g(a1), px_b(a1)) +
            DFX_JPEG_YCC_CB(px_r(b0), px_g(b0), px_b(b0)) + DFX_JPEG_YCC_CB(px_r(b1), px_g(b1), px_b(b1)) + bias) >> 2;
}
__device__ __forceinline__ int cr2(unsigned a0, unsigned a1, unsigned b0, unsigned b1, int bias) {
    return (DFX_JPEG_YCC_CR(px_r(a0), px_g(a0), px_b(a0)) + DFX_JPEG_YCC_CR(px_r(a1), px_g(a1), px_b(a1)) +
            DFX_JPEG_YCC_CR(px_r(b0), px_g(b0), px_b(b0)) + DFX_JPEG_YCC_CR(px_r(b1), px_g(b1), px_b(b1)) + bias) >> 2;
}

template <bool EMIT>
__global__ __launch_bounds__(CJ_THREADS) void k_jpeg_colour_blocks(JpegColourCtx c) {
    __shared__ unsigned ys[16][CJ_MCUS * 4];          // Y of the strip, 16 rows x 512 samples, four samples per word
    __shared__ unsigned short cs[2][8][CJ_MCUS * 4];  // Cb, Cr: 8 rows x 256 samples, two samples per element
    __shared__ short zz[64][CJ_THREADS];              // [zig-zag position][thread]: the entropy loop indexes dynamically
    __shared__ short dcs[CJ_THREADS];                 // quantised DC of every block of the strip (dummy blocks copy one)
    const int tid = threadIdx.x;
    const int frame = blockIdx.z, my = blockIdx.y, mx0 = blockIdx.x * CJ_MCUS;
    if (EMIT && c.hdr[1] != 0) // the streams do not fit the shared buffer (k_jpeg_layout): nothing is written
        return;
    const int nmcu = min(CJ_MCUS, c.mcus_x - mx0);
    const unsigned char *F = c.bgr + (long long)frame * c.frame_stride;
    const int ch = (c.h + 1) >> 1; // chroma rows that come out of the downsampler

    // ---- stage 1: units of 4 pixels x 2 rows -> 8 Y, 2 Cb, 2 Cr samples
    const int ux_n = nmcu * 4;
    for (int u = tid; u < ux_n * 8; u += CJ_THREADS) {
        const int uy = u / ux_n, ux = u - uy * ux_n;
        const int x = mx0 * 16 + ux * 4, cy = my * 8 + uy;
        unsigned a[4], b[4];
        load4_bgr(F + (long long)min(2 * cy, c.h - 1) * c.pitch, x, c.w, a);
        load4_bgr(F + (long long)min(2 * cy + 1, c.h - 1) * c.pitch, x, c.w, b);
        ys[2 * uy][ux] = y4(a);
        ys[2 * uy + 1][ux] = y4(b);
        if (cy >= ch) { // below the image: the last downsampled row again
            load4_bgr(F + (long long)(2 * (ch - 1)) * c.pitch, x, c.w, a);
            load4_bgr(F + (long long)min(2 * ch - 1, c.h - 1) * c.pitch, x, c.w, b);
        }
        cs[0][uy][ux] = (unsigned short)(cb2(a[0], a[1], b[0], b[1], 1) | (cb2(a[2], a[3], b[2], b[3], 2) << 8));
        cs[1][uy][ux] = (unsigned short)(cr2(a[0], a[1], b[0], b[1], 1) | (cr2(a[2], a[3], b[2], b[3], 2) << 8));
    }
    __syncthreads();

    // ---- stage 2: one thread per block
    const int mcu = tid / 6, k = tid - mcu * 6;
    const bool active = mcu < nmcu;
    const int bx = (mx0 + mcu) * 2 + (k & 1), by = my * 2 + (k >> 1); // Y blocks only
    const bool dummy = k < 4 && (bx * 8 >= c.w || by * 8 >= c.h);
    const JpegTables &T = c.tab[k >= 4 ? 1 : 0];
    int dc = 0;
    unsigned long long nz = 0; // bit j: zig-zag position j holds a non-zero coefficient
    if (active && !dummy) {
        int a[8][8];
        if (k < 4) {
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const unsigned lo = ys[(k >> 1) * 8 + y][mcu * 4 + (k & 1) * 2], hi = ys[(k >> 1) * 8 + y][mcu * 4 + (k & 1) * 2 + 1];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    a[y][x] = (int)((lo >> (8 * x)) & 255u) - 128;
                    a[y][4 + x] = (int)((hi >> (8 * x)) & 255u) - 128;
                }
            }
        } else {
#pragma unroll
            for (int y = 0; y < 8; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const unsigned v = cs[k - 4][y][mcu * 4 + x];
                    a[y][2 * x] = (int)(v & 255u) - 128;
                    a[y][2 * x + 1] = (int)(v >> 8) - 128;
                }
        }
#pragma unroll
        for (int y = 0; y < 8; ++y)
            dfx_jpeg_fdct_islow_1d<true>(a[y][0], a[y][1], a[y][2], a[y][3], a[y][4], a[y][5], a[y][6], a[y][7]);
#pragma unroll
        for (int x = 0; x < 8; ++x)
            dfx_jpeg_fdct_islow_1d<false>(a[0][x], a[1][x], a[2][x], a[3][x], a[4][x], a[5][x], a[6][x], a[7][x]);
#pragma unroll
        for (int v = 0; v < 8; ++v)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int q = dfx_jpeg_quantise(a[v][u], T.div[v * 8 + u], T.magic[v * 8 + u]);
                const int j = T.nat2zig[v * 8 + u];
                if (v == 0 && u == 0) {
                    dc = q;
                } else {
                    zz[j][tid] = (short)q;
                    nz |= (unsigned long long)(q != 0) << j;
                }
            }
    }
    dcs[tid] = (short)dc;
    __syncthreads();
    if (!active)
        return;
    if (dummy) { // the DC of the last real Y block before this one in the MCU (Y00 is always real)
        const bool right = ((mx0 + mcu) * 2 + 1) * 8 >= c.w, bottom = (my * 2 + 1) * 8 >= c.h;
        const int src = (k >> 1) && bottom ? (right ? 0 : 1) : k - 1;
        dc = dcs[mcu * 6 + src];
    }
    const int nblk = c.mcus_x * c.mcus_y * 6;
    const int b = (my * c.mcus_x + mx0 + mcu) * 6 + k; // MCU order
    const long long bi = (long long)frame * nblk + b;
    if (!EMIT) {
        unsigned bits = 0;
        int last = 0;
        while (nz) {
            const int j = __builtin_ctzll(nz);
            nz &= nz - 1;
            const int run = j - last - 1;
            last = j;
            const int vq = zz[j][tid];
            const int n = bit_length(vq < 0 ? -vq : vq);
            bits += (unsigned)(run >> 4) * T.ac_len[0xF0] + T.ac_len[((run & 15) << 4) | n] + n;
        }
        if (last != 63)
            bits += T.ac_len[0x00];
        c.dc[bi] = (short)dc;
        c.bits[bi] = bits;
        return;
    }
    Emitter E;
    E.begin(c.stream, c.plane_base[frame] * 8ull + c.bits[bi]);
    const int pb = jpeg_colour_pred_block(b);
    const int diff = dc - (pb >= 0 ? (int)c.dc[(long long)frame * nblk + pb] : 0);
    const int nb = bit_length(diff < 0 ? -diff : diff);
    E.put(T.dc_code[nb], T.dc_len[nb]);
    if (nb)
        E.put((unsigned)(diff < 0 ? diff - 1 : diff), nb);
    int last = 0;
    while (nz) {
        const int j = __builtin_ctzll(nz);
        nz &= nz - 1;
        int run = j - last - 1;
        last = j;
        while (run > 15) {
            E.put(T.ac_code[0xF0], T.ac_len[0xF0]);
            run -= 16;
        }
        const int vq = zz[j][tid];
        const int n = bit_length(vq < 0 ? -vq : vq);
        const int sym = (run << 4) | n;
        E.put(((unsigned)T.ac_code[sym] << n) | ((unsigned)(vq < 0 ? vq - 1 : vq) & ((1u << n) - 1u)), T.ac_len[sym] + n);
    }
    if (last != 63)
        E.put(T.ac_code[0x00], T.ac_len[0x00]);
    E.end();
}

} // namespace

void jpeg_colour_launch_encode(hipStream_t s, const JpegColourCtx &c) {
    const dim3 grid((c.mcus_x + CJ_MCUS - 1) / CJ_MCUS, c.mcus_y, c.n_planes);
    hipLaunchKernelGGL(k_jpeg_colour_blocks<false>, grid, dim3(CJ_THREADS), 0, s, c);
    hipLaunchKernelGGL((k_jpeg_scan<JpegColourCtx, true>), dim3(c.n_planes), dim3(1024), 0, s, c);
    hipLaunchKernelGGL(k_jpeg_layout<JpegColourCtx>, dim3(1), dim3(1), 0, s, c);
    hipLaunchKernelGGL(k_jpeg_zero<JpegColourCtx>, dim3(1024), dim3(256), 0, s, c);
    hipLaunchKernelGGL(k_jpeg_colour_blocks<true>, grid, dim3(CJ_THREADS), 0, s, c);
}
