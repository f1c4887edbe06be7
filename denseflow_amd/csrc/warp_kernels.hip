// warp_kernels.hip — the backward warp of 8-bit images by a flow, and the photometric error of the result, on the device:
// what a consumer of flow tensors does next with a flow (an occlusion-aware loss, a frame interpolator, a flow filter), and
// mean |I0 - warp(I1, F)|, the quality figure that needs no ground truth.
//
// Image i is sampled at the positions flow i names.  Output pixel (x, y) with flow (fu, fv), all in float32, every operation
// rounded on its own (the build's -ffp-contract=off: no fused multiply-add anywhere below):
//     px = (float)x + fu;  py = (float)y + fv
//     inside = px >= 0 && py >= 0 && px <= W-1 && py <= H-1      (false for NaN and either infinity; tested before any
//                                                                 conversion to int — the test of fb_check_kernels.hip)
//     WARP_BORDER_ZERO : not inside -> every channel's sample is 0.0f
//     WARP_BORDER_CLAMP: px or py NaN -> sample 0.0f; otherwise px = min(max(px, 0), W-1), py likewise (infinities clamp)
//     x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
//     per channel, P = (float)byte: t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s = t + ay*(b - t)
// s lies in [0, 255] (the taps are representable, every rounding is monotone): no clamp on the way out.  Stored: s as
// float32, s through dfx_planar_half_bits as float16 / bfloat16, or q = (uint8)rintf(s) (ties to even).
//     valid = inside (the unclamped test in either mode) && (no occlusion mask || occ[y][x] == 0)
//     statistics of image i, over its pixels with valid == 1: count += 1, sad += sum over channels |ref - q|   (integers)
// tests/warp_ref.py is the same text in NumPy; the two agree bit for bit.
//
// The shape of k_fb_check: 4 neighbouring pixels of a row per lane, 256 threads, the taps plain byte loads (the displacement
// is unbounded: no tile to stage), no scratch, registers for eight waves per SIMD.  A lane's 4 pixels are 4 consecutive
// elements of each plane (gray, planar) or 12 consecutive elements (interleaved): C "segments" of 4 elements either way,
// each read (ref) or written (out) in one access — 4 bytes of u8, 8 of a half type, 16 of float32 — where the base and every
// stride keep that alignment (warp_launch decides once per launch), in single elements otherwise and at the ragged right
// edge.  The statistics form lets a workgroup walk WARP_STATS_ROWS rows, sums count and sad per lane in 32 bits (a workgroup's
// totals are at most 256 * 32 and 256 * 32 * 3 * 255 < 2^23), reduces them across the wave with __shfl_xor and across the four
// waves through 32 bytes of LDS, and one lane issues one 64-bit atomicAdd per word whose value it never reads: a 1080p image
// issues 2 * 8 * 34 = 544 of them.  The form without statistics has no loop, no LDS and no barrier.
// Bytes per pixel: 8 of flow, 1 .. 4 C of taps (perfectly cached .. every tap its own sector), C x elem of out, + C of ref,
// + 1 of occ, + 1 of valid where asked for.
#include "warp_kernels.h"

#include <algorithm>

#include "dfx_device.h"

namespace {

// which accesses take a lane's 4 elements at once; one value per launch, so every branch on them is wave-uniform
struct WarpWide {
    int flow, ref, out, occ, valid;
};

// m = 1..4 elements of a segment to out + at (elements of dtype): one access where wide and m == 4
__device__ __forceinline__ void warp_put4(void *out, long long at, int dtype, bool wide, int m, const float (&s)[4]) {
    if (dtype == WARP_OUT_U8) {
        unsigned char *p = static_cast<unsigned char *>(out) + at;
        unsigned q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            q[e] = (unsigned)rintf(s[e]);
        if (wide && m == 4) {
            *reinterpret_cast<unsigned *>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m)
                    p[e] = (unsigned char)q[e];
        }
    } else if (dtype == DFX_ELEM_F32) {
        float *p = static_cast<float *>(out) + at;
        if (wide && m == 4) {
            *reinterpret_cast<float4 *>(p) = make_float4(s[0], s[1], s[2], s[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m)
                    p[e] = s[e];
        }
    } else {
        unsigned short *p = static_cast<unsigned short *>(out) + at;
        unsigned q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            q[e] = dfx_planar_half_bits(s[e], dtype);
        if (wide && m == 4) {
            *reinterpret_cast<uint2 *>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m)
                    p[e] = (unsigned short)q[e];
        }
    }
}

// the 4 pixels (x .. x + 3, y) of image i; cnt / sad: the lane's statistics (STATS only)
template <int C, bool IL, bool STATS>
__device__ __forceinline__ void warp_quad(const WarpArgs &a, const WarpWide &wide, int x, int y, long long i, unsigned &cnt,
                                          unsigned &sad) {
    constexpr int XS = IL ? C : 1; // bytes (elements) between neighbouring pixels of a row
    const int n = min(4, a.w - x);
    const float *fu = a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x;
    const float *fv = fu + a.plane_stride;
    float u[4], v[4];
    if (wide.flow && n == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(fu);
        const float4 r = *reinterpret_cast<const float4 *>(fv);
        u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u[k] = k < n ? fu[k] : 0.0f;
            v[k] = k < n ? fv[k] : 0.0f;
        }
    }
    const unsigned char *src = a.src + i * a.src_image;
    const long long cs = IL ? 1 : a.src_plane; // bytes between the channels of a tap
    const float wmax = (float)(a.w - 1), hmax = (float)(a.h - 1);
    float s[4][C];
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c)
            s[k][c] = 0.0f;
        if (k < n) {
            float px = (float)(x + k) + u[k], py = (float)y + v[k];
            // the range test comes before any conversion to int: false for NaN and for either infinity
            const bool inside = px >= 0.0f && py >= 0.0f && px <= wmax && py <= hmax;
            ok[k] = inside ? 1u : 0u;
            bool take = inside;
            if (a.border == WARP_BORDER_CLAMP) {
                take = px == px && py == py;
                px = __builtin_fminf(__builtin_fmaxf(px, 0.0f), wmax);
                py = __builtin_fminf(__builtin_fmaxf(py, 0.0f), hmax);
            }
            if (take) {
                const float fx = floorf(px), fy = floorf(py);
                const int x0 = (int)fx, y0 = (int)fy;
                const float ax = px - fx, ay = py - fy;
                const int x1 = min(x0 + 1, a.w - 1), y1 = min(y0 + 1, a.h - 1);
                const unsigned char *r0 = src + (long long)y0 * a.src_pitch, *r1 = src + (long long)y1 * a.src_pitch;
                const int o0 = x0 * XS, o1 = x1 * XS;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const long long co = C == 1 ? 0 : c * cs;
                    const float p00 = (float)r0[o0 + co], p01 = (float)r0[o1 + co];
                    const float p10 = (float)r1[o0 + co], p11 = (float)r1[o1 + co];
                    const float t = p00 + ax * (p01 - p00);
                    const float b = p10 + ax * (p11 - p10);
                    s[k][c] = t + ay * (b - t);
                }
            }
        }
    }
    if (a.occ) {
        const unsigned char *o = a.occ + i * a.occ_stride + (long long)y * a.occ_pitch + x;
        if (wide.occ && n == 4) {
            const unsigned m = *reinterpret_cast<const unsigned *>(o);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((m >> (8 * k)) & 0xffu)
                    ok[k] = 0u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n && o[k] != 0)
                    ok[k] = 0u;
        }
    }
    if (a.valid) {
        unsigned char *d = a.valid + i * a.valid_stride + (long long)y * a.valid_pitch + x;
        if (wide.valid && n == 4) {
            *reinterpret_cast<unsigned *>(d) = ok[0] | (ok[1] << 8) | (ok[2] << 16) | (ok[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n)
                    d[k] = (unsigned char)ok[k];
        }
    }
    if (STATS) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            cnt += ok[k]; // 0 beyond the row's end
    }
    // segment g: the lane's 4 elements of plane g (gray, planar), or elements 4 g .. 4 g + 3 of its 12 interleaved ones
#pragma unroll
    for (int g = 0; g < C; ++g) {
        float sv[4];
        unsigned okv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = IL ? (4 * g + e) / C : e, c = IL ? (4 * g + e) % C : g;
            sv[e] = s[k][c], okv[e] = ok[k];
        }
        const int m = IL ? min(max(C * n - 4 * g, 0), 4) : n; // elements of the segment inside the row
        if (m <= 0)
            continue;
        const int xo = x * XS + (IL ? 4 * g : 0);
        if (STATS) {
            const unsigned char *r = a.ref + i * a.src_image + (IL ? 0 : g * a.src_plane) + (long long)y * a.src_pitch + xo;
            unsigned rv[4];
            if (wide.ref && m == 4) {
                const unsigned q = *reinterpret_cast<const unsigned *>(r);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    rv[e] = (q >> (8 * e)) & 0xffu;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    rv[e] = e < m ? r[e] : 0u;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m && okv[e]) {
                    const int d = (int)rv[e] - (int)(unsigned)rintf(sv[e]);
                    sad += (unsigned)(d < 0 ? -d : d);
                }
        }
        if (a.out) {
            const long long at = i * a.out_image + (IL ? 0 : g * a.out_plane) + (long long)y * a.out_pitch + xo;
            warp_put4(a.out, at, a.out_dtype, wide.out != 0, m, sv);
        }
    }
}

// C: channels; IL: interleaved (C == 3 only); STATS: with the statistics.  grid: (ceil(w / 256), ceil(h / rows), images) with
// rows = WARP_STATS_ROWS for STATS, 4 otherwise.  Eight waves per SIMD (64 registers) for every form but the planar 3-channel
// one with statistics: its three plane addresses per tap and the loop's running sums need 74 registers, so it is given 80
// (six waves per SIMD) and never spills.
template <int C, bool IL, bool STATS>
__global__ __launch_bounds__(256, (C == 3 && !IL && STATS) ? 6 : 8) void k_warp(WarpArgs a, WarpWide wide) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = ((int)blockIdx.x * 64 + lane) * 4;
    const long long i = (long long)blockIdx.z;
    unsigned cnt = 0u, sad = 0u;
    if constexpr (!STATS) {
        const int y = (int)blockIdx.y * 4 + wave;
        if (x < a.w && y < a.h)
            warp_quad<C, IL, false>(a, wide, x, y, i, cnt, sad);
    } else {
#pragma unroll 1
        for (int g = 0; g < WARP_STATS_ROWS / 4; ++g) {
            const int y = ((int)blockIdx.y * (WARP_STATS_ROWS / 4) + g) * 4 + wave;
            if (x < a.w && y < a.h)
                warp_quad<C, IL, true>(a, wide, x, y, i, cnt, sad);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            cnt += __shfl_xor(cnt, m);
            sad += __shfl_xor(sad, m);
        }
        __shared__ unsigned part[8];
        if (lane == 0)
            part[wave] = cnt, part[4 + wave] = sad;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned c4 = part[0] + part[1] + part[2] + part[3];
            const unsigned s4 = part[4] + part[5] + part[6] + part[7];
            if (c4)
                atomicAdd(a.stats + 2 * i, (unsigned long long)c4);
            if (s4)
                atomicAdd(a.stats + 2 * i + 1, (unsigned long long)s4);
        }
    }
}

template <int C, bool IL>
void warp_launch_as(hipStream_t s, const WarpArgs &a, const WarpWide &wide) {
    const unsigned gx = (unsigned)((a.w + 255) / 256);
    if (a.stats)
        hipLaunchKernelGGL((k_warp<C, IL, true>), dim3(gx, (unsigned)((a.h + WARP_STATS_ROWS - 1) / WARP_STATS_ROWS), (unsigned)a.n),
                           dim3(256), 0, s, a, wide);
    else
        hipLaunchKernelGGL((k_warp<C, IL, false>), dim3(gx, (unsigned)((a.h + 3) / 4), (unsigned)a.n), dim3(256), 0, s, a, wide);
}

} // namespace

void warp_launch(hipStream_t s, const WarpArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    const bool three = args.channels == 3, planes = three && args.planar != 0;
    const int eb = args.out_dtype == WARP_OUT_U8 ? 1 : dfx_elem_bytes(args.out_dtype);
    // a lane's 4 elements in one access: the base and every stride a multiple of that access
    WarpWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.ref = dfx_bytes4(args.ref, args.src_pitch, args.src_image, planes ? args.src_plane : 0);
    wide.out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, eb) == 4;
    wide.occ = dfx_bytes4(args.occ, args.occ_pitch, args.occ_stride, 0);
    wide.valid = dfx_bytes4(args.valid, args.valid_pitch, args.valid_stride, 0);
    if (args.stats)
        (void)hipMemsetAsync(args.stats, 0, (size_t)args.n * 2 * sizeof(unsigned long long), s);
    // grid.z holds at most 65535 images: more than that go in several launches
    const int chunk = 65535;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        WarpArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.src += (long long)i0 * args.src_image;
        a.flow += (long long)i0 * args.flow_stride;
        if (a.ref)
            a.ref += (long long)i0 * args.src_image;
        if (a.out)
            a.out = static_cast<unsigned char *>(a.out) + (long long)i0 * args.out_image * eb;
        if (a.occ)
            a.occ += (long long)i0 * args.occ_stride;
        if (a.valid)
            a.valid += (long long)i0 * args.valid_stride;
        if (a.stats)
            a.stats += 2LL * i0;
        if (!three)
            warp_launch_as<1, false>(s, a, wide);
        else if (!planes)
            warp_launch_as<3, true>(s, a, wide);
        else
            warp_launch_as<3, false>(s, a, wide);
    }
}
