// flow_median_kernels.hip — mask-aware median filter and occlusion fill of planar float32 flows on the device
// (dfx_flow_median_device; the arithmetic is stated in include/dfx.h, tests/flow_median_ref.py is that text in NumPy).
//
// Every sample is handled as the unsigned key of its bit pattern, key(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000): the
// order of the keys is the numeric order with -0 below +0 and the NaNs at the ends, there is no float instruction below,
// and the output is the bit pattern of one input sample (key is its own inverse up to the choice of the constant, fm_bits).
//
// Shape.  A workgroup of 256 lanes owns a tile of FM_TILE_W x FM_TILE_H = 64 x 16 pixels of one flow.  It stages the tile
// with its halo of r = ksize / 2 pixels — (16 + 2r) rows of (64 + 2r) keys per plane, the coordinates clamped to the frame,
// which is both the replicated border and the tile edge — in LDS: 16-byte loads of the 64 inner columns where base and
// strides keep the alignment, single elements otherwise, at the frame's ragged right edge and in the 2r halo columns.  The
// masked forms first stage a third plane of words, 0 for an included sample and 0xFFFFFFFF for an excluded one, and OR
// each key with its word as it is staged.  Then lane (tx, ty) computes the 4 pixels x = 4 tx .. 4 tx + 3 of row ty: it reads
// the ksize rows of 4 + 2r keys it needs as 16- and 8-byte LDS reads (a row starts at a multiple of 16 bytes: the pitch is
// 64 + 2r + 2 words for r = 1 and 64 + 2r for r = 2) and keeps them in registers for its 4 windows, so a key costs
// (16 + 2r)(64 + 2r) / 1024 = 1.2 (r = 1) / 1.33 (r = 2) global loads instead of 9 / 25.
//
// Selection.  Unmasked: the fixed-rank networks of flow_median_networks.h, 19 exchanges for 3 x 3 and 99 for 5 x 5 (the
// networks of the oracle's median9 / median25), v_min_u32 / v_max_u32 on the keys (the compiler folds pairs of them into
// v_min3 / v_max3 / v_med3_u32).  Masked: an excluded sample is 0xFFFFFFFF and sorts last (a real sample of that key is the
// same value: harmless); the network leaves the 5 / 13 smallest in order (25 / 124 exchanges: only ranks
// 0 .. (ksize² - 1) / 2 are ever asked for); m = ksize² minus the excluded count, and the sample of rank (m - 1) >> 1 is
// taken by a chain of conditional moves.
// In FILL mode a pixel whose own mask is 0 skips the network (its staged key is its value); a pixel with m == 0 is masked
// itself, so it reads its value back from global memory.  All indices are literals after unrolling: no scratch.
#include "flow_median_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"
#include "flow_median_networks.h"

namespace {

__device__ __forceinline__ unsigned fm_key(unsigned b) { return b ^ ((unsigned)((int)b >> 31) | 0x80000000u); }
__device__ __forceinline__ unsigned fm_bits(unsigned k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

#define FM_CE(a, b)                                                                                                    \
    {                                                                                                                  \
        const unsigned lo_ = min(p[a], p[b]), hi_ = max(p[a], p[b]);                                                   \
        p[a] = lo_, p[b] = hi_;                                                                                        \
    }

// the median key of the K * K keys in p (destroyed)
template <int K>
__device__ __forceinline__ unsigned fm_median(unsigned (&p)[K * K]) {
    if constexpr (K == 3) {
        FM_NET9_MEDIAN(FM_CE)
        return p[4];
    } else {
        FM_NET25_MEDIAN(FM_CE)
        return p[12];
    }
}

// the key of rank `rank` (0 .. (K * K - 1) / 2, lane-variant) of the K * K keys in p (destroyed)
template <int K>
__device__ __forceinline__ unsigned fm_select(unsigned (&p)[K * K], int rank) {
    if constexpr (K == 3) {
        FM_NET9_LOW5(FM_CE)
    } else {
        FM_NET25_LOW13(FM_CE)
    }
    unsigned res = p[0];
#pragma unroll
    for (int j = 1; j <= (K * K - 1) / 2; ++j)
        res = rank == j ? p[j] : res;
    return res;
}

template <int K>
struct FmGeom {
    static constexpr int R = K / 2;
    static constexpr int ROWS = FM_TILE_H + 2 * R;        // staged rows
    static constexpr int COLS = FM_TILE_W + 2 * R;        // staged columns: column c is pixel x0 - R + c
    static constexpr int PITCH = (COLS + 3) / 4 * 4;      // words per staged row: a row starts at a multiple of 16 bytes
    static constexpr int STRIP = 4 + 2 * R;               // keys of a row a lane's 4 windows span
    static constexpr int PLANE = ROWS * PITCH;            // words per staged plane
};

// Stages one float plane as keys.  src: the plane of this flow; (x0, y0): the tile's first pixel.  MASKED: each key is ORed
// with the exclusion word staged for its position (excl: the plane fm_stage_mask wrote, same geometry).
template <int K, bool MASKED>
__device__ __forceinline__ void fm_stage_plane(unsigned *lds, const float *src, long long pitch, int x0, int y0, int w, int h,
                                               bool wide, const unsigned *excl) {
    using G = FmGeom<K>;
    const int tid = (int)threadIdx.x;
    for (int idx = tid; idx < G::ROWS * (FM_TILE_W / 4); idx += 256) { // the 64 inner columns, 4 at a time
        const int row = idx / (FM_TILE_W / 4), q = idx % (FM_TILE_W / 4);
        const int gy = min(max(y0 - G::R + row, 0), h - 1), gx = x0 + 4 * q;
        const unsigned *s = reinterpret_cast<const unsigned *>(src) + (long long)gy * pitch;
        unsigned b[4];
        if (wide && gx + 3 < w) {
            const uint4 v = *reinterpret_cast<const uint4 *>(s + gx);
            b[0] = v.x, b[1] = v.y, b[2] = v.z, b[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                b[k] = s[min(gx + k, w - 1)];
        }
        const int at = row * G::PITCH + G::R + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            lds[at + k] = fm_key(b[k]) | (MASKED ? excl[at + k] : 0u);
    }
    for (int idx = tid; idx < G::ROWS * 2 * G::R; idx += 256) { // the halo columns
        const int row = idx / (2 * G::R), j = idx % (2 * G::R);
        const int c = j < G::R ? j : FM_TILE_W + j; // columns 0 .. R-1 and 64 + R .. 64 + 2R - 1
        const int gy = min(max(y0 - G::R + row, 0), h - 1), gx = min(max(x0 - G::R + c, 0), w - 1);
        const int at = row * G::PITCH + c;
        lds[at] = fm_key(reinterpret_cast<const unsigned *>(src)[(long long)gy * pitch + gx]) | (MASKED ? excl[at] : 0u);
    }
}

// Stages one mask plane as exclusion words: 0 = included, 0xFFFFFFFF = excluded.
template <int K>
__device__ __forceinline__ void fm_stage_mask(unsigned *lds, const unsigned char *src, long long pitch, int x0, int y0, int w,
                                              int h, bool wide) {
    using G = FmGeom<K>;
    const int tid = (int)threadIdx.x;
    for (int idx = tid; idx < G::ROWS * (FM_TILE_W / 4); idx += 256) {
        const int row = idx / (FM_TILE_W / 4), q = idx % (FM_TILE_W / 4);
        const int gy = min(max(y0 - G::R + row, 0), h - 1), gx = x0 + 4 * q;
        const unsigned char *s = src + (long long)gy * pitch;
        unsigned b[4];
        if (wide && gx + 3 < w) {
            const unsigned v = *reinterpret_cast<const unsigned *>(s + gx);
            b[0] = v & 0xFFu, b[1] = (v >> 8) & 0xFFu, b[2] = (v >> 16) & 0xFFu, b[3] = v >> 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                b[k] = s[min(gx + k, w - 1)];
        }
        unsigned *d = lds + row * G::PITCH + G::R + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            d[k] = b[k] ? 0xFFFFFFFFu : 0u;
    }
    for (int idx = tid; idx < G::ROWS * 2 * G::R; idx += 256) {
        const int row = idx / (2 * G::R), j = idx % (2 * G::R);
        const int c = j < G::R ? j : FM_TILE_W + j;
        const int gy = min(max(y0 - G::R + row, 0), h - 1), gx = min(max(x0 - G::R + c, 0), w - 1);
        lds[row * G::PITCH + c] = src[(long long)gy * pitch + gx] ? 0xFFFFFFFFu : 0u;
    }
}

// A lane's K rows of STRIP words of one staged plane, from LDS: 16-byte reads and, for K == 3, one 8-byte read per row.
template <int K>
__device__ __forceinline__ void fm_strip(const unsigned *lds, int tx, int ty, unsigned (&s)[K][FmGeom<K>::STRIP]) {
    using G = FmGeom<K>;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const unsigned *row = lds + (ty + j) * G::PITCH + 4 * tx;
        const uint4 a = *reinterpret_cast<const uint4 *>(row);
        s[j][0] = a.x, s[j][1] = a.y, s[j][2] = a.z, s[j][3] = a.w;
        if constexpr (K == 3) {
            const uint2 b = *reinterpret_cast<const uint2 *>(row + 4);
            s[j][4] = b.x, s[j][5] = b.y;
        } else {
            const uint4 b = *reinterpret_cast<const uint4 *>(row + 4);
            s[j][4] = b.x, s[j][5] = b.y, s[j][6] = b.z, s[j][7] = b.w;
        }
    }
}

struct FmWide {
    bool flow, mask, out, mask_out; // a lane's 4 pixels in one access (wave-uniform)
};

// K: ksize 3 or 5.  MASKED: a.mask is given.  MODE: FM_ALL or FM_FILL (FM_FILL only with MASKED).
template <int K, bool MASKED, int MODE>
__global__ __launch_bounds__(256, K == 3 ? 8 : (MASKED ? 5 : 6)) void k_flow_median(FmArgs a, FmWide wide) {
    using G = FmGeom<K>;
    __shared__ __attribute__((aligned(16))) unsigned lds[(MASKED ? 3 : 2) * G::PLANE];
    const int tid = (int)threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int x0 = (int)blockIdx.x * FM_TILE_W, y0 = (int)blockIdx.y * FM_TILE_H;
    const long long i = (long long)blockIdx.z;
    const float *fu = a.flow + i * a.flow_stride;
    const unsigned *excl = nullptr;
    if constexpr (MASKED) {
        fm_stage_mask<K>(lds + 2 * G::PLANE, a.mask + i * a.mask_stride, a.mask_pitch, x0, y0, a.w, a.h, wide.mask);
        excl = lds + 2 * G::PLANE;
        __syncthreads();
    }
    fm_stage_plane<K, MASKED>(lds, fu, a.row_pitch, x0, y0, a.w, a.h, wide.flow, excl);
    fm_stage_plane<K, MASKED>(lds + G::PLANE, fu + a.plane_stride, a.row_pitch, x0, y0, a.w, a.h, wide.flow, excl);
    __syncthreads();
    const int x = x0 + 4 * tx, y = y0 + ty;
    if (x >= a.w || y >= a.h)
        return;
    const int n = fq_count(a.w, x);

    // per pixel: the rank to take, whether the pixel keeps its input, and its mask_out
    int rank[4];
    bool keep[4];
    unsigned mo[4];
    if constexpr (MASKED) {
        unsigned e[K][G::STRIP];
        fm_strip<K>(lds + 2 * G::PLANE, tx, ty, e);
        int col[G::STRIP]; // minus the excluded count of each column of the strip
#pragma unroll
        for (int c = 0; c < G::STRIP; ++c) {
            col[c] = 0;
#pragma unroll
            for (int j = 0; j < K; ++j)
                col[c] += (int)e[j][c];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int m = K * K;
#pragma unroll
            for (int c = 0; c < K; ++c)
                m += col[k + c];
            const bool own = e[G::R][k + G::R] != 0u;
            rank[k] = (m - 1) >> 1;
            keep[k] = m == 0 || (MODE == FM_FILL && !own);
            mo[k] = m == 0 ? 1u : 0u;
        }
    }

    unsigned res[2][4];
#pragma unroll
    for (int plane = 0; plane < 2; ++plane) {
        unsigned s[K][G::STRIP];
        fm_strip<K>(lds + plane * G::PLANE, tx, ty, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned key = s[G::R][k + G::R];
            if constexpr (!MASKED) {
                unsigned p[K * K];
#pragma unroll
                for (int j = 0; j < K; ++j)
#pragma unroll
                    for (int c = 0; c < K; ++c)
                        p[j * K + c] = s[j][k + c];
                key = fm_median<K>(p);
            } else if (!keep[k]) {
                unsigned p[K * K];
#pragma unroll
                for (int j = 0; j < K; ++j)
#pragma unroll
                    for (int c = 0; c < K; ++c)
                        p[j * K + c] = s[j][k + c];
                key = fm_select<K>(p, rank[k]);
            }
            res[plane][k] = fm_bits(key);
            if constexpr (MASKED) { // m == 0: the centre is excluded itself, its staged key is not its value
                if (mo[k] != 0u && k < n)
                    res[plane][k] = reinterpret_cast<const unsigned *>(fu + plane * a.plane_stride)[(long long)y * a.row_pitch + x + k];
            }
        }
    }

    float ru[4], rv[4]; // the bit patterns travel as they are: no float instruction touches them
#pragma unroll
    for (int k = 0; k < 4; ++k)
        ru[k] = __uint_as_float(res[0][k]), rv[k] = __uint_as_float(res[1][k]);
    fq_store_flow(a.out + i * a.out_stride + (long long)y * a.out_pitch + x, a.out_plane, wide.out, n, ru, rv);
    if constexpr (MASKED) {
        if (a.mask_out)
            fq_store_u8(a.mask_out + i * a.mask_out_stride + (long long)y * a.mask_out_pitch + x, wide.mask_out, n, mo);
    }
}

template <int K>
void fm_launch_k(hipStream_t s, const FmArgs &a, const FmWide &wide, dim3 grid) {
    if (!a.mask)
        hipLaunchKernelGGL((k_flow_median<K, false, FM_ALL>), grid, dim3(256), 0, s, a, wide);
    else if (a.mode == FM_FILL)
        hipLaunchKernelGGL((k_flow_median<K, true, FM_FILL>), grid, dim3(256), 0, s, a, wide);
    else
        hipLaunchKernelGGL((k_flow_median<K, true, FM_ALL>), grid, dim3(256), 0, s, a, wide);
}

} // namespace

void fm_launch(hipStream_t s, const FmArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    FmWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.mask = dfx_bytes4(args.mask, args.mask_pitch, args.mask_stride);
    wide.out = dfx_planar_vec(args.out, args.out_stride, args.out_plane, args.out_pitch) == 4;
    wide.mask_out = dfx_bytes4(args.mask_out, args.mask_out_pitch, args.mask_out_stride);
    // grid.z holds at most FQ_ITEMS_MAX = 65535 flows: more than that go in several launches
    const int chunk = FQ_ITEMS_MAX;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        FmArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.flow += (long long)i0 * args.flow_stride;
        a.out += (long long)i0 * args.out_stride;
        if (a.mask)
            a.mask += (long long)i0 * args.mask_stride;
        if (a.mask_out)
            a.mask_out += (long long)i0 * args.mask_out_stride;
        const dim3 grid((unsigned)((a.w + FM_TILE_W - 1) / FM_TILE_W), (unsigned)((a.h + FM_TILE_H - 1) / FM_TILE_H),
                        (unsigned)a.n);
        if (a.ksize == 3)
            fm_launch_k<3>(s, a, wide, grid);
        else
            fm_launch_k<5>(s, a, wide, grid);
    }
}
