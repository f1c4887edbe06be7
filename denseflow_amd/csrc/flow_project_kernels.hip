// flow_project_kernels.hip — forward projection (splat) of planar flows on the device: the flow as seen from the frame it
// points to (t = 1, scale = -1: the inverse flow) or from a time t in between (scale = -t / 1 - t: F_{t->0} / F_{t->1}), with
// the pixels nothing lands on marked as holes.  The one scatter of the library; every sibling call is a gather.
//
// All float operations are float32, each rounded on its own (the build's -ffp-contract=off), subnormals kept.  For source
// pixel (x, y) of a flow with value (fu, fv):
//     skip the pixel if occ != NULL and occ[y][x] != 0
//     px = (float)x + t*fu;   py = (float)y + t*fv
//     skip unless px > -1 && px < W && py > -1 && py < H     (false for NaN; tested before any conversion to int)
//     iq = 256                                                 without importance
//          imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)
//     x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)      0 .. 256;   y0, by likewise
//     qu = (int)rintf(fminf(fmaxf(fu * 256.f, -8388608.f), 8388608.f));   qv likewise
//     taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), column weights {256 - bx, bx}, row weights {256 - by, by};
//     a tap outside the frame is dropped;  wt = wx * wy * iq (uint64)
//     Wsum[tap] += wt;   Su[tap] += wt * qu;   Sv[tap] += wt * qv      (64-bit, two's-complement wrap)
// and per target pixel, after all sources of the flow:
//     hole = Wsum < Wmin;  out = hole ? +0 : (float)(((double)S / (double)Wsum) * ((double)scale / 256.0))
//     coverage = (float)((double)Wsum / 16777216.0)
// tests/flow_project_ref.py is the same text in NumPy.  The sums are integers, so they do not depend on the order in which
// the adds arrive, nor on how they are grouped: the two forms of the scatter below give the same words, and the device
// equals the reference bit for bit.  A tap of weight 0 and a payload of 0 are not added at all.
//
// Workspace: FP_WORDS (3) 64-bit words per pixel, (Wsum, Su, Sv) next to each other, pixel after pixel, flow after flow of a
// wave: the three adds of a tap fall into one or two 64-byte segments and the two taps of a row into 48 contiguous bytes.
// Passes per wave of flows, all on one stream with nothing between them:
//   k_fp_zero       16-byte stores over the wave's words (a single leading / trailing word where the base is 8 mod 16);
//   k_fp_scatter    32 x 8 source pixels per workgroup of 256, one pixel per lane, grid.z the flows of the wave.
//                   FP_LDS_WINDOW 0: every add is a 64-bit global atomic, up to 12 per source pixel.
//                   FP_LDS_WINDOW 1: the adds go to a 48 x 16 pixel window in LDS (18 KiB, ds_add_u64), placed where the
//                   tile's centre pixel lands (24 pixels to its left, 8 rows above it); a tap outside the window goes to
//                   a global atomic as before; after a barrier the window's non-zero words are added to the workspace, lane
//                   after lane along the window's rows (1152 contiguous bytes per row).
//   k_fp_normalise  the lane quad of flow_quad.h: a lane's 12 words as six 16-byte loads where the workspace base is 16-byte
//                   aligned and W is even (8-byte loads otherwise), the planes and the hole mask through its quad stores.
// No float atomics anywhere.
#include "flow_project_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

#ifndef FP_LDS_WINDOW
#define FP_LDS_WINDOW 1 // 0: the plain global-atomic scatter (kept for profiles/flow_project's A/B)
#endif

namespace {

typedef unsigned long long u64;

#ifndef FP_TILE_W
#define FP_TILE_W 32 // the source tile and the margin of the window around it can be chosen per build for an A/B
#define FP_TILE_H 8
#define FP_MARGIN_X 8
#define FP_MARGIN_Y 4
#endif
enum : int { FP_TW = FP_TILE_W, FP_TH = FP_TILE_H, FP_THREADS = FP_TW * FP_TH };  // source tile of a workgroup, a pixel per lane
enum : int { FP_WW = FP_TW + 2 * FP_MARGIN_X, FP_WH = FP_TH + 2 * FP_MARGIN_Y }; // LDS window, pixels: 48 x 16
enum : int { FP_WIN = FP_WW * FP_WH * FP_WORDS };                                  // its words: 2304, 9 per thread

struct FpWide {
    int work, out, hole, cov;
};

__device__ __forceinline__ void fp_gadd(u64 *p, u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_fp_zero(u64 *work, long long words) {
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

// IMP: with an importance plane; OCC: with an occlusion mask; LDSW: through the LDS window.
// grid: (ceil(w / 32), ceil(h / 8), flows of the wave)
template <bool IMP, bool OCC, bool LDSW>
__global__ __launch_bounds__(FP_THREADS) void k_fp_scatter(FpArgs a) {
    __shared__ u64 win[LDSW ? FP_WIN : 1];
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * FP_TW + tid % FP_TW, y = (int)blockIdx.y * FP_TH + tid / FP_TW;
    const long long f = (long long)blockIdx.z;
    const float *fu_p = a.flow + f * a.flow_stride;
    u64 *work = a.work + f * (long long)a.h * a.w * FP_WORDS;
    const float wf = (float)a.w, hf = (float)a.h;
    int ox = 0, oy = 0;
    if (LDSW) {
        for (int i = tid; i < FP_WIN; i += FP_THREADS)
            win[i] = 0ull;
        // the window sits where the tile's centre pixel lands: one broadcast load per plane, the same in every lane
        const int cx = min((int)blockIdx.x * FP_TW + FP_TW / 2, a.w - 1), cy = min((int)blockIdx.y * FP_TH + FP_TH / 2, a.h - 1);
        const float *c = fu_p + (long long)cy * a.row_pitch + cx;
        const float pcx = (float)cx + a.t * c[0], pcy = (float)cy + a.t * c[a.plane_stride];
        // NaN and the infinities end at a bound: the window is then nowhere near, and every tap goes the global way
        ox = (int)floorf(__builtin_fminf(__builtin_fmaxf(pcx, -1.0e9f), 1.0e9f)) - FP_WW / 2;
        oy = (int)floorf(__builtin_fminf(__builtin_fmaxf(pcy, -1.0e9f), 1.0e9f)) - FP_WH / 2;
        __syncthreads();
    }
    bool live = x < a.w && y < a.h;
    if (OCC && live)
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
    if (IMP) {
        float imp = 0.0f;
        if (live)
            imp = a.imp[f * a.imp_stride + (long long)y * a.imp_pitch + x];
        live = live && imp > 0.0f;
        iq = live ? (int)rintf(__builtin_fminf(imp, 256.0f) * 256.0f) : 0;
        live = live && iq > 0;
    }
    if (live) {
        const float fx = floorf(px), fy = floorf(py);
        const int x0 = (int)fx, y0 = (int)fy;
        const int bx = (int)rintf((px - fx) * 256.0f), by = (int)rintf((py - fy) * 256.0f);
        const int qu = (int)rintf(__builtin_fminf(__builtin_fmaxf(fu * 256.0f, -8388608.0f), 8388608.0f));
        const int qv = (int)rintf(__builtin_fminf(__builtin_fmaxf(fv * 256.0f, -8388608.0f), 8388608.0f));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int tx = x0 + i, ty = y0 + j;
                const int wxy = (i ? bx : 256 - bx) * (j ? by : 256 - by);
                if (wxy == 0 || tx < 0 || tx >= a.w || ty < 0 || ty >= a.h)
                    continue;
                const u64 wt = (u64)(unsigned)wxy * (u64)(unsigned)iq;
                const u64 su = wt * (u64)(long long)qu, sv = wt * (u64)(long long)qv; // wraps as the int64 product does
                const int lx = tx - ox, ly = ty - oy;
                if (LDSW && (unsigned)lx < (unsigned)FP_WW && (unsigned)ly < (unsigned)FP_WH) {
                    u64 *q = win + (ly * FP_WW + lx) * FP_WORDS;
                    (void)__hip_atomic_fetch_add(q, wt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (qu != 0)
                        (void)__hip_atomic_fetch_add(q + 1, su, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (qv != 0)
                        (void)__hip_atomic_fetch_add(q + 2, sv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    u64 *q = work + ((long long)ty * a.w + tx) * FP_WORDS;
                    fp_gadd(q, wt);
                    if (qu != 0)
                        fp_gadd(q + 1, su);
                    if (qv != 0)
                        fp_gadd(q + 2, sv);
                }
            }
        }
    }
    if (LDSW) {
        __syncthreads();
        // a non-zero word lies inside the frame (taps outside it were dropped); the test below only keeps that local
        for (int i = tid; i < FP_WIN; i += FP_THREADS) {
            const u64 v = win[i];
            const int ly = i / (FP_WW * FP_WORDS), r = i - ly * (FP_WW * FP_WORDS);
            const int tx = ox + r / FP_WORDS, ty = oy + ly;
            if (v != 0ull && tx >= 0 && tx < a.w && ty >= 0 && ty < a.h)
                fp_gadd(work + ((long long)ty * a.w + tx) * FP_WORDS + (r % FP_WORDS), v);
        }
    }
}

// grid: fq_grid(w, h, flows of the wave)
__global__ __launch_bounds__(256) void k_fp_normalise(FpArgs a, FpWide wide) {
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long f = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    const u64 *p = a.work + ((f * a.h + y) * a.w + x) * FP_WORDS;
    u64 q[4 * FP_WORDS];
    if (wide.work && n == 4) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(p)[k];
            q[2 * k] = v.x, q[2 * k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4 * FP_WORDS; ++k)
            q[k] = k < n * FP_WORDS ? p[k] : 0ull;
    }
    float ou[4], ov[4], oc[4];
    unsigned oh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const u64 ws = q[3 * e];
        const bool hole = ws < a.wmin;
        const double d = (double)ws;
        const float u = (float)(((double)(long long)q[3 * e + 1] / d) * a.sc);
        const float v = (float)(((double)(long long)q[3 * e + 2] / d) * a.sc);
        ou[e] = hole ? 0.0f : u;
        ov[e] = hole ? 0.0f : v;
        oh[e] = hole ? 1u : 0u;
        oc[e] = (float)(d * 5.9604644775390625e-08); // 2^-24: the same bits as the division by 16777216.0
    }
    if (a.out)
        fq_store_flow(a.out + f * a.out_stride + (long long)y * a.out_pitch + x, a.out_plane, wide.out != 0, n, ou, ov);
    if (a.hole)
        fq_store_u8(a.hole + f * a.hole_stride + (long long)y * a.hole_pitch + x, wide.hole != 0, n, oh);
    if (a.cov)
        fq_store_f32(a.cov + f * a.cov_stride + (long long)y * a.cov_pitch + x, wide.cov != 0, n, oc);
}

template <bool IMP, bool OCC>
void fp_scatter_as(hipStream_t s, const FpArgs &a) {
    hipLaunchKernelGGL((k_fp_scatter<IMP, OCC, FP_LDS_WINDOW != 0>),
                       dim3((unsigned)((a.w + FP_TW - 1) / FP_TW), (unsigned)((a.h + FP_TH - 1) / FP_TH), (unsigned)a.n), dim3(FP_THREADS), 0,
                       s, a);
}

// which accesses of the normalising pass take a lane's 4 pixels at once
FpWide fp_wide(const FpArgs &args) {
    FpWide wide;
    wide.work = ((size_t)args.work & 15) == 0 && (args.w & 1) == 0;
    wide.out = args.out && dfx_planar_vec(args.out, args.out_stride, args.out_plane, args.out_pitch) == 4;
    wide.hole = args.hole && (((u64)(size_t)args.hole | (u64)args.hole_pitch | (u64)args.hole_stride) & 3) == 0;
    wide.cov = args.cov && dfx_planar_vec(args.cov, args.cov_stride, 0, args.cov_pitch) == 4;
    return wide;
}

void fp_normalise(hipStream_t s, const FpArgs &a, const FpWide &wide) {
    hipLaunchKernelGGL(k_fp_normalise, fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
}

} // namespace

void fp_renormalise(hipStream_t s, const FpArgs &args) {
    if (args.n <= 0 || args.n > FQ_ITEMS_MAX || args.w <= 0 || args.h <= 0)
        return;
    fp_normalise(s, args, fp_wide(args));
}

void fp_launch(hipStream_t s, const FpArgs &args, long long flows_per_wave) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0 || flows_per_wave <= 0)
        return;
    const FpWide wide = fp_wide(args);
    const long long per_flow = (long long)args.w * args.h * FP_WORDS; // words
    const int chunk = (int)std::min<long long>(flows_per_wave, FQ_ITEMS_MAX);  // grid.z holds at most FQ_ITEMS_MAX = 65535 flows
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        FpArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.flow += (long long)i0 * args.flow_stride;
        if (a.imp)
            a.imp += (long long)i0 * args.imp_stride;
        if (a.occ)
            a.occ += (long long)i0 * args.occ_stride;
        if (a.out)
            a.out += (long long)i0 * args.out_stride;
        if (a.hole)
            a.hole += (long long)i0 * args.hole_stride;
        if (a.cov)
            a.cov += (long long)i0 * args.cov_stride;
        const long long words = per_flow * a.n;
        const unsigned zblocks = (unsigned)std::min<long long>((words / 2 + 255) / 256 + 1, 8192);
        hipLaunchKernelGGL(k_fp_zero, dim3(zblocks), dim3(256), 0, s, a.work, words);
        if (a.imp) {
            if (a.occ)
                fp_scatter_as<true, true>(s, a);
            else
                fp_scatter_as<true, false>(s, a);
        } else {
            if (a.occ)
                fp_scatter_as<false, true>(s, a);
            else
                fp_scatter_as<false, false>(s, a);
        }
        fp_normalise(s, a, wide);
    }
}
