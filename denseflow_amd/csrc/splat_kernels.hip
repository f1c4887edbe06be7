// splat_kernels.hip — forward warp (splat) of images and float payloads along planar flows on the device: frame 0 as seen at
// time t of F_{0->1}, and with it its labels, a depth plane or a feature map; the pixels nothing lands on are holes.  The
// scatter of flow_project_kernels.hip with a payload of C channels beside the weight instead of the flow itself.
//
// All float operations are float32, each rounded on its own (the build's -ffp-contract=off), subnormals kept.  For source
// pixel (x, y) of image i with flow (fu, fv), the skip rules, the landing test, the importance, the tap geometry and the
// weights are those of flow_project_kernels.hip word for word:
//     skip the pixel if occ != NULL and occ[y][x] != 0
//     px = (float)x + t*fu;   py = (float)y + t*fv
//     skip unless px > -1 && px < W && py > -1 && py < H     (false for NaN; tested before any conversion to int)
//     iq = 256 without importance;  imp = importance[y][x]; skip unless imp > 0;  iq = (int)rintf(fminf(imp, 256.f) * 256.f)
//     x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f);   y0, by likewise;   wt = wx * wy * iq (uint64)
//     payload, 8-bit source:   q_c = the byte
//     payload, float32 source: skip unless every channel has fabsf(v_c) <= 32768.f (false for NaN);  q_c = (int)rintf(v_c * 256.f)
//     Wsum[tap] += wt;   S_c[tap] += wt * q_c      (64-bit, two's-complement wrap)
// and per target pixel, after all sources of the image:
//     hole = Wsum < Wmin;  r_c = (double)S_c / (double)Wsum (mean) or (double)S_c / 16777216.0 (sum), times 1.0/256.0 for a
//     float32 source;  out = (float)r_c or (uint8_t)llrint(r_c);  a hole is +0 / byte 0 (zero) or not written at all (keep)
//     coverage = (float)((double)Wsum / 16777216.0)
// tests/splat_ref.py is the same text in NumPy.  The sums are integers: they do not depend on the order of the adds nor on
// how they are grouped, so both forms of the scatter give the same words and the device equals the reference bit for bit.
//
// Workspace: 1 + C 64-bit words per pixel, (Wsum, S_0 .. S_{C-1}) next to each other, pixel after pixel, image after image of
// a wave.  Passes per wave of images, all on one stream with nothing between them:
//   k_splat_zero       16-byte stores over the wave's words (a single leading / trailing word where the base is 8 mod 16);
//   k_splat_scatter    32 x 8 source pixels per workgroup of 256, one pixel per lane, grid.z the images of the wave; one
//                      instantiation per channel count and source form (8-bit planes: gray and planar 3; 8-bit interleaved
//                      3: three byte loads; float32 planes 1 .. 4); importance and occ are wave-uniform runtime branches.
//                      SPLAT_LDS_WINDOW 0: every add is a 64-bit global atomic, up to 4 (1 + C) per source pixel.
//                      SPLAT_LDS_WINDOW 1: the adds go to a 48 x 16 pixel window in LDS (768 (1 + C) words: 12 / 18 / 24 /
//                      30 KiB), placed where the tile's centre pixel lands; a tap outside the window goes to a global
//                      atomic as before; after a barrier the window's non-zero words are added to the workspace, lane after
//                      lane along the window's rows (384 (1 + C) contiguous bytes per row).
//   k_splat_normalise  the lane quad of flow_quad.h: a lane's 4 (1 + C) words as 16-byte loads where the workspace base is
//                      16-byte aligned and W (1 + C) is even (8-byte loads otherwise), the image, the hole mask and the
//                      coverage through its quad stores; with keep, a quad that holds a hole stores its other pixels singly.
// No float atomics anywhere.
#include "splat_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

#ifndef SPLAT_LDS_WINDOW
#define SPLAT_LDS_WINDOW 1 // 0: the plain global-atomic scatter (kept for profiles/splat's A/B)
#endif

namespace {

typedef unsigned long long u64;

enum : int { SP_TW = 32, SP_TH = 8, SP_THREADS = SP_TW * SP_TH }; // source tile of a workgroup, a pixel per lane
enum : int { SP_WW = SP_TW + 16, SP_WH = SP_TH + 8 };             // LDS window, pixels: 48 x 16
enum : int { SP_U8 = 0, SP_U8_IL = 1, SP_F32 = 2 };               // source forms: byte planes, interleaved bytes, float planes

struct SplatWide {
    int work, out, hole, cov;
};

__device__ __forceinline__ void sp_gadd(u64 *p, u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_splat_zero(u64 *work, long long words) {
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

// C: channels; SRC: the source form; LDSW: through the LDS window.
// grid: (ceil(w / 32), ceil(h / 8), images of the wave)
template <int C, int SRC, bool LDSW>
__global__ __launch_bounds__(SP_THREADS) void k_splat_scatter(SplatArgs a) {
    constexpr int WORDS = 1 + C, WIN = SP_WW * SP_WH * WORDS;
    __shared__ u64 win[LDSW ? WIN : 1];
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * SP_TW + tid % SP_TW, y = (int)blockIdx.y * SP_TH + tid / SP_TW;
    const long long f = (long long)blockIdx.z;
    const float *fu_p = a.flow + f * a.flow_stride;
    u64 *work = a.work + f * (long long)a.h * a.w * WORDS;
    const float wf = (float)a.w, hf = (float)a.h;
    int ox = 0, oy = 0;
    if (LDSW) {
        for (int i = tid; i < WIN; i += SP_THREADS)
            win[i] = 0ull;
        // the window sits where the tile's centre pixel lands: one broadcast load per plane, the same in every lane
        const int cx = min((int)blockIdx.x * SP_TW + SP_TW / 2, a.w - 1), cy = min((int)blockIdx.y * SP_TH + SP_TH / 2, a.h - 1);
        const float *c = fu_p + (long long)cy * a.row_pitch + cx;
        const float pcx = (float)cx + a.t * c[0], pcy = (float)cy + a.t * c[a.plane_stride];
        // NaN and the infinities end at a bound: the window is then nowhere near, and every tap goes the global way
        ox = (int)floorf(__builtin_fminf(__builtin_fmaxf(pcx, -1.0e9f), 1.0e9f)) - SP_WW / 2;
        oy = (int)floorf(__builtin_fminf(__builtin_fmaxf(pcy, -1.0e9f), 1.0e9f)) - SP_WH / 2;
        __syncthreads();
    }
    bool live = x < a.w && y < a.h;
    if (a.occ && live)
        live = a.occ[f * a.occ_stride + (long long)y * a.occ_pitch + x] == 0;
    float fu = 0.0f, fv = 0.0f;
    if (live) {
        const float *p = fu_p + (long long)y * a.row_pitch + x;
        fu = p[0], fv = p[a.plane_stride];
    }
    const float px = (float)x + a.t * fu, py = (float)y + a.t * fv;
    // the range test comes before any conversion to int: false for NaN
    live = live && px > -1.0f && px < wf && py > -1.0f && py < hf;
    int iq = 256;
    if (a.imp) {
        float imp = 0.0f;
        if (live)
            imp = a.imp[f * a.imp_stride + (long long)y * a.imp_pitch + x];
        live = live && imp > 0.0f;
        iq = live ? (int)rintf(__builtin_fminf(imp, 256.0f) * 256.0f) : 0;
        live = live && iq > 0;
    }
    int q[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
        q[c] = 0;
    if (live) {
        if (SRC == SP_F32) {
            const float *p = static_cast<const float *>(a.src) + f * a.src_image + (long long)y * a.src_pitch + x;
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c] = p[C == 1 ? 0 : c * a.src_plane];
                live = live && __builtin_fabsf(v[c]) <= 32768.0f; // false for NaN: skipped, not clamped
            }
#pragma unroll
            for (int c = 0; c < C; ++c)
                q[c] = live ? (int)rintf(v[c] * 256.0f) : 0;
        } else {
            const unsigned char *p = static_cast<const unsigned char *>(a.src) + f * a.src_image + (long long)y * a.src_pitch +
                                     (SRC == SP_U8_IL ? C * x : x);
#pragma unroll
            for (int c = 0; c < C; ++c)
                q[c] = (int)p[SRC == SP_U8_IL ? (long long)c : (C == 1 ? 0ll : c * a.src_plane)];
        }
    }
    if (live) {
        const float fx = floorf(px), fy = floorf(py);
        const int x0 = (int)fx, y0 = (int)fy;
        const int bx = (int)rintf((px - fx) * 256.0f), by = (int)rintf((py - fy) * 256.0f);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int tx = x0 + i, ty = y0 + j;
                const int wxy = (i ? bx : 256 - bx) * (j ? by : 256 - by);
                if (wxy == 0 || tx < 0 || tx >= a.w || ty < 0 || ty >= a.h)
                    continue;
                const u64 wt = (u64)(unsigned)wxy * (u64)(unsigned)iq;
                const int lx = tx - ox, ly = ty - oy;
                if (LDSW && (unsigned)lx < (unsigned)SP_WW && (unsigned)ly < (unsigned)SP_WH) {
                    u64 *w = win + (ly * SP_WW + lx) * WORDS;
                    (void)__hip_atomic_fetch_add(w, wt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (q[c] != 0) // wt * q wraps as the int64 product does
                            (void)__hip_atomic_fetch_add(w + 1 + c, wt * (u64)(long long)q[c], __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    u64 *w = work + ((long long)ty * a.w + tx) * WORDS;
                    sp_gadd(w, wt);
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (q[c] != 0)
                            sp_gadd(w + 1 + c, wt * (u64)(long long)q[c]);
                }
            }
        }
    }
    if (LDSW) {
        __syncthreads();
        // a non-zero word lies inside the frame (taps outside it were dropped); the test below only keeps that local
        for (int i = tid; i < WIN; i += SP_THREADS) {
            const u64 v = win[i];
            const int ly = i / (SP_WW * WORDS), r = i - ly * (SP_WW * WORDS);
            const int tx = ox + r / WORDS, ty = oy + ly;
            if (v != 0ull && tx >= 0 && tx < a.w && ty >= 0 && ty < a.h)
                sp_gadd(work + ((long long)ty * a.w + tx) * WORDS + (r % WORDS), v);
        }
    }
}

// C: channels; IL: the output's pixels are interleaved.  grid: fq_grid(w, h, images of the wave)
template <int C, bool IL>
__global__ __launch_bounds__(256) void k_splat_normalise(SplatArgs a, SplatWide wide) {
    constexpr int WORDS = 1 + C;
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long f = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    const u64 *p = a.work + ((f * a.h + y) * a.w + x) * WORDS;
    u64 q[4 * WORDS];
    if (wide.work && n == 4) {
#pragma unroll
        for (int k = 0; k < 2 * WORDS; ++k) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(p)[k];
            q[2 * k] = v.x, q[2 * k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * WORDS; ++k)
            q[k] = k < n * WORDS ? p[k] : 0ull;
    }
    const double post = a.src_f32 ? 0.00390625 : 1.0; // 1.0 / 256.0
    float s[4][C], oc[4];
    unsigned oh[4];
    unsigned holes = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const u64 ws = q[WORDS * e];
        const bool hole = ws < a.wmin;
        const double d = (double)ws;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double sc = (double)(long long)q[WORDS * e + 1 + c];
            double r = a.sum ? sc / 16777216.0 : sc / d;
            r = hole ? 0.0 : r * post;
            s[e][c] = a.out_u8 ? (float)(unsigned)rint(r) : (float)r; // rint on [0, 255]: llrint's value, ties to even
        }
        oh[e] = hole ? 1u : 0u;
        holes |= (e < n && hole) ? 1u : 0u;
        oc[e] = (float)(d * 5.9604644775390625e-08); // 2^-24: the same bits as the division by 16777216.0
    }
    if (a.out) {
        const int dtype = a.out_u8 ? FQ_ELEM_U8 : DFX_ELEM_F32;
        const long long row = f * a.out_image + (long long)y * a.out_pitch;
        if (a.keep && holes) {
            // the hole pixels stay as the caller left them: the others go one element at a time
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= n || oh[e])
                    continue;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const long long at = row + (IL ? (long long)((x + e) * C + c) : (C == 1 ? 0ll : c * a.out_plane) + x + e);
                    if (a.out_u8)
                        static_cast<unsigned char *>(a.out)[at] = (unsigned char)(unsigned)s[e][c];
                    else
                        static_cast<float *>(a.out)[at] = s[e][c];
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < C; ++g) { // the segments of flow_quad.h
                float sv[4];
                fq_segment<C, IL>(s, g, sv);
                const int m = fq_seg_count<C, IL>(g, n);
                if (m <= 0)
                    continue;
                fq_store_image(a.out, row + fq_seg_offset<C, IL>(x, g, C == 1 ? 0ll : a.out_plane), dtype, wide.out != 0, m, sv);
            }
        }
    }
    if (a.hole)
        fq_store_u8(a.hole + f * a.hole_stride + (long long)y * a.hole_pitch + x, wide.hole != 0, n, oh);
    if (a.cov)
        fq_store_f32(a.cov + f * a.cov_stride + (long long)y * a.cov_pitch + x, wide.cov != 0, n, oc);
}

template <int C, int SRC>
void sp_scatter_as(hipStream_t s, const SplatArgs &a) {
    hipLaunchKernelGGL((k_splat_scatter<C, SRC, SPLAT_LDS_WINDOW != 0>),
                       dim3((unsigned)((a.w + SP_TW - 1) / SP_TW), (unsigned)((a.h + SP_TH - 1) / SP_TH), (unsigned)a.n), dim3(SP_THREADS), 0,
                       s, a);
}

void sp_scatter(hipStream_t s, const SplatArgs &a) {
    if (!a.src_f32) {
        if (a.channels == 1)
            sp_scatter_as<1, SP_U8>(s, a);
        else if (a.interleaved)
            sp_scatter_as<3, SP_U8_IL>(s, a);
        else
            sp_scatter_as<3, SP_U8>(s, a);
    } else if (a.channels == 1) {
        sp_scatter_as<1, SP_F32>(s, a);
    } else if (a.channels == 2) {
        sp_scatter_as<2, SP_F32>(s, a);
    } else if (a.channels == 3) {
        sp_scatter_as<3, SP_F32>(s, a);
    } else {
        sp_scatter_as<4, SP_F32>(s, a);
    }
}

template <int C, bool IL>
void sp_normalise_as(hipStream_t s, const SplatArgs &a, const SplatWide &wide) {
    hipLaunchKernelGGL((k_splat_normalise<C, IL>), fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
}

void sp_normalise(hipStream_t s, const SplatArgs &a, const SplatWide &wide) {
    if (a.interleaved)
        sp_normalise_as<3, true>(s, a, wide);
    else if (a.channels == 1)
        sp_normalise_as<1, false>(s, a, wide);
    else if (a.channels == 2)
        sp_normalise_as<2, false>(s, a, wide);
    else if (a.channels == 3)
        sp_normalise_as<3, false>(s, a, wide);
    else
        sp_normalise_as<4, false>(s, a, wide);
}

// which accesses of the normalising pass take a lane's 4 pixels at once
SplatWide sp_wide(const SplatArgs &args) {
    const bool planes = args.channels > 1 && !args.interleaved;
    SplatWide wide;
    wide.work = ((size_t)args.work & 15) == 0 && (((long long)args.w * splat_words(args.channels)) & 1) == 0;
    wide.out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, args.out_u8 ? 1 : 4) == 4;
    wide.hole = dfx_bytes4(args.hole, args.hole_pitch, args.hole_stride, 0);
    wide.cov = args.cov && dfx_planar_vec(args.cov, args.cov_stride, 0, args.cov_pitch) == 4;
    return wide;
}

} // namespace

void splat_launch(hipStream_t s, const SplatArgs &args, long long images_per_wave) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0 || images_per_wave <= 0 || args.channels < 1 || args.channels > SPLAT_MAX_CHANNELS)
        return;
    const SplatWide wide = sp_wide(args);
    const long long per_image = (long long)args.w * args.h * splat_words(args.channels); // words
    const int chunk = (int)std::min<long long>(images_per_wave, FQ_ITEMS_MAX);                   // grid.z holds at most FQ_ITEMS_MAX = 65535 images
    const long long src_bytes = args.src_f32 ? 4 : 1, out_bytes = args.out_u8 ? 1 : 4;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        SplatArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.src = static_cast<const unsigned char *>(args.src) + (long long)i0 * args.src_image * src_bytes;
        a.flow += (long long)i0 * args.flow_stride;
        if (a.imp)
            a.imp += (long long)i0 * args.imp_stride;
        if (a.occ)
            a.occ += (long long)i0 * args.occ_stride;
        if (a.out)
            a.out = static_cast<unsigned char *>(args.out) + (long long)i0 * args.out_image * out_bytes;
        if (a.hole)
            a.hole += (long long)i0 * args.hole_stride;
        if (a.cov)
            a.cov += (long long)i0 * args.cov_stride;
        const long long words = per_image * a.n;
        const unsigned zblocks = (unsigned)std::min<long long>((words / 2 + 255) / 256 + 1, 8192);
        hipLaunchKernelGGL(k_splat_zero, dim3(zblocks), dim3(256), 0, s, a.work, words);
        sp_scatter(s, a);
        sp_normalise(s, a, wide);
    }
}
