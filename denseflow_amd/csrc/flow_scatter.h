// flow_scatter.h — the one integer scatter of the library: the forward projection of flows (flow_project_kernels.hip) and the
// forward warp of images and payloads (splat_kernels.hip) take their source fields, their landing rule, their taps, their adds,
// their LDS window, their zero pass and the shared half of their normalising pass from here.  The rules are plain C++ under
// DFX_HD, float32, every operation rounded on its own (the build's -ffp-contract=off): tests/flow_scatter_harness.cpp compiles
// this very text on the CPU and tests/test_flow_scatter_cpu.py holds its sums word for word against the NumPy references.
//
// For source pixel (x, y) of item f with flow (fu, fv):
//     skip the pixel if occ != NULL and occ[y][x] != 0
//     px = (float)x + t*fu;   py = (float)y + t*fv
//     skip unless px > -1 && px < W && py > -1 && py < H     (false for NaN; tested before any conversion to int)
//     iq = 256                                                 without importance
//          imp = importance[y][x]; skip unless imp > 0 (NaN skips);  iq = (int)rintf(fminf(imp, 256.f) * 256.f)
//     q_0 .. q_{WORDS-2}: the caller's integer payload, which may skip the pixel too
//     x0 = floorf(px); bx = (int)rintf((px - x0) * 256.f)      0 .. 256;   y0, by likewise
//     taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), column weights {256 - bx, bx}, row weights {256 - by, by};
//     a tap outside the frame is dropped;  wt = wx * wy * iq (uint64)
//     Wsum[tap] += wt;   S_c[tap] += wt * q_c      (64-bit, two's-complement wrap)
// A tap of weight 0 and a payload of 0 are not added at all.  The sums are integers, so they depend neither on the order in
// which the adds arrive nor on how they are grouped: every form of the scatter gives the same words.  No float atomics.
//
// Workspace: WORDS 64-bit words per pixel, (Wsum, S_0, ..) next to each other, pixel after pixel, item after item of a wave.
// A workgroup of 256 scatters 32 x 8 source pixels, one per lane.  Without the window every add is a 64-bit global atomic.
// With it the adds go to a 48 x 16 pixel window in LDS (ds_add_u64), placed where the tile's centre pixel lands (24 pixels to
// its left, 8 rows above it); a tap outside the window goes to a global atomic as before; after a barrier the window's non-zero
// words are added to the workspace, lane after lane along the window's rows.
#pragma once

#include <algorithm>
#include <cmath>

#include "flow_quad.h"

#if defined(__HIPCC__)
#define FS_UNROLL _Pragma("unroll")
#else
#define FS_UNROLL
#endif

typedef unsigned long long fs_u64;

enum : int { FS_TW = 32, FS_TH = 8, FS_THREADS = FS_TW * FS_TH }; // source tile of a workgroup, a pixel per lane
enum : int { FS_WW = FS_TW + 16, FS_WH = FS_TH + 8 };             // LDS window, pixels: 48 x 16
constexpr int fs_window_words(int words) { return FS_WW * FS_WH * words; }

// What both scatters read and what both normalising passes write beside their own output.  Planar float32 flows of w x h
// pixels: flow i has its u plane at flow + i * flow_stride, the v plane plane_stride behind it, rows row_pitch apart.  imp (may
// be nullptr): one float plane per item; occ (may be nullptr): one byte plane per item; hole (bytes) and cov (floats): one plane
// per item, each may be nullptr.  work: WORDS * w * h words per item of a wave; 8-byte aligned.
struct FsSource {
    const float *flow;
    const float *imp;
    const unsigned char *occ;
    unsigned char *hole;
    float *cov;
    fs_u64 *work;
    int n, w, h;
    float t;     // px = x + t * fu
    fs_u64 wmin; // hole = Wsum < wmin; >= 1 (fp_wmin)
    long long row_pitch, plane_stride, flow_stride; // floats
    long long imp_pitch, imp_stride;                // floats
    long long occ_pitch, occ_stride;                // bytes
    long long hole_pitch, hole_stride;              // bytes
    long long cov_pitch, cov_stride;                // floats
};

// FsSource::wmin of a min_weight: max(1, llrint(min_weight * 2^24)), at most 2^63 (a min_weight no sum can reach makes every
// pixel a hole).
inline fs_u64 fp_wmin(float min_weight) {
    const double m = (double)min_weight * 16777216.0;
    return m >= 9223372036854775808.0 ? (1ull << 63) : std::max<fs_u64>(1ull, (fs_u64)std::llrint(m));
}

// Where source pixel (x, y) of item f lands, in the order of the rules above.  fu, fv are 0 where the flow was not loaded.
struct FsLanding {
    bool live;
    float px, py, fu, fv;
    int iq;
};
DFX_HD FsLanding fs_landing(const FsSource &a, long long f, int x, int y, bool with_imp, bool with_occ) {
    FsLanding l;
    l.live = x < a.w && y < a.h;
    if (with_occ && l.live)
        l.live = a.occ[f * a.occ_stride + (long long)y * a.occ_pitch + x] == 0;
    l.fu = l.fv = 0.0f;
    if (l.live) {
        const float *p = a.flow + f * a.flow_stride + (long long)y * a.row_pitch + x;
        l.fu = p[0], l.fv = p[a.plane_stride];
    }
    l.px = (float)x + a.t * l.fu, l.py = (float)y + a.t * l.fv;
    // the range test comes before any conversion to int: false for NaN
    l.live = l.live && l.px > -1.0f && l.px < (float)a.w && l.py > -1.0f && l.py < (float)a.h;
    l.iq = 256;
    if (with_imp) {
        float imp = 0.0f;
        if (l.live)
            imp = a.imp[f * a.imp_stride + (long long)y * a.imp_pitch + x];
        l.live = l.live && imp > 0.0f;
        l.iq = l.live ? (int)__builtin_rintf(__builtin_fminf(imp, 256.0f) * 256.0f) : 0;
        l.live = l.live && l.iq > 0;
    }
    return l;
}

// The four taps of a live landing: add(tx, ty, wt) for every tap inside the frame whose weight is not 0.
template <typename Add>
DFX_HD void fs_taps(const FsLanding &l, int w, int h, Add add) {
    const float fx = __builtin_floorf(l.px), fy = __builtin_floorf(l.py);
    const int x0 = (int)fx, y0 = (int)fy;
    const int bx = (int)__builtin_rintf((l.px - fx) * 256.0f), by = (int)__builtin_rintf((l.py - fy) * 256.0f);
    FS_UNROLL
    for (int j = 0; j < 2; ++j) {
        FS_UNROLL
        for (int i = 0; i < 2; ++i) {
            const int tx = x0 + i, ty = y0 + j;
            const int wxy = (i ? bx : 256 - bx) * (j ? by : 256 - by);
            if (wxy == 0 || tx < 0 || tx >= w || ty < 0 || ty >= h)
                continue;
            add(tx, ty, (fs_u64)(unsigned)wxy * (fs_u64)(unsigned)l.iq);
        }
    }
}

// One 64-bit add: a relaxed atomic of workgroup scope (LDS: the window) or agent scope on the device, a plain += on the CPU.
template <bool LDS>
DFX_HD void fs_add_word(fs_u64 *p, fs_u64 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
#else
    *p += v;
#endif
}
// wt to word 0 and wt * q[c] to word 1 + c of the pixel at p; the product wraps as the int64 product does
template <int WORDS, bool LDS>
DFX_HD void fs_add_pixel(fs_u64 *p, fs_u64 wt, const int (&q)[WORDS - 1]) {
    fs_add_word<LDS>(p, wt);
    FS_UNROLL
    for (int c = 0; c < WORDS - 1; ++c)
        if (q[c] != 0)
            fs_add_word<LDS>(p + 1 + c, wt * (fs_u64)(long long)q[c]);
}

// The window of a tile: its words (fs_window_words(WORDS) of them; unused without WINDOW) and the frame pixel of its corner.
struct FsWindow {
    fs_u64 *win;
    int ox, oy;
};
// The window sits where the centre pixel of tile (tile_x, tile_y) lands.  NaN and the infinities end at a bound of +-1e9: the
// window is then nowhere near, and every tap goes the global way.
DFX_HD FsWindow fs_window(fs_u64 *win, const FsSource &a, long long f, int tile_x, int tile_y) {
    const int mx = tile_x * FS_TW + FS_TW / 2, my = tile_y * FS_TH + FS_TH / 2;
    const int cx = mx < a.w - 1 ? mx : a.w - 1, cy = my < a.h - 1 ? my : a.h - 1;
    const float *c = a.flow + f * a.flow_stride + (long long)cy * a.row_pitch + cx;
    const float pcx = (float)cx + a.t * c[0], pcy = (float)cy + a.t * c[a.plane_stride];
    FsWindow o;
    o.win = win;
    o.ox = (int)__builtin_floorf(__builtin_fminf(__builtin_fmaxf(pcx, -1.0e9f), 1.0e9f)) - FS_WW / 2;
    o.oy = (int)__builtin_floorf(__builtin_fminf(__builtin_fmaxf(pcy, -1.0e9f), 1.0e9f)) - FS_WH / 2;
    return o;
}
// lane `lane` of `lanes` clears its share of the window
template <int WORDS>
DFX_HD void fs_window_clear(fs_u64 *win, int lane, int lanes) {
    for (int i = lane; i < fs_window_words(WORDS); i += lanes)
        win[i] = 0ull;
}
// The add of one tap to item f's words `work`: to the window where the tap lies inside it, to the workspace otherwise.
template <int WORDS, bool WINDOW>
DFX_HD void fs_add(const FsWindow &o, fs_u64 *work, int w, int tx, int ty, fs_u64 wt, const int (&q)[WORDS - 1]) {
    const int lx = tx - o.ox, ly = ty - o.oy;
    if (WINDOW && (unsigned)lx < (unsigned)FS_WW && (unsigned)ly < (unsigned)FS_WH)
        fs_add_pixel<WORDS, true>(o.win + (ly * FS_WW + lx) * WORDS, wt, q);
    else
        fs_add_pixel<WORDS, false>(work + ((long long)ty * w + tx) * WORDS, wt, q);
}
// lane `lane` of `lanes` adds its share of the window's non-zero words to the workspace.  A non-zero word lies inside the frame
// (taps outside it were dropped); the test below only keeps that local.
template <int WORDS>
DFX_HD void fs_window_flush(const FsWindow &o, fs_u64 *work, int w, int h, int lane, int lanes) {
    for (int i = lane; i < fs_window_words(WORDS); i += lanes) {
        const fs_u64 v = o.win[i];
        const int ly = i / (FS_WW * WORDS), r = i - ly * (FS_WW * WORDS);
        const int tx = o.ox + r / WORDS, ty = o.oy + ly;
        if (v != 0ull && tx >= 0 && tx < w && ty >= 0 && ty < h)
            fs_add_word<false>(work + ((long long)ty * w + tx) * WORDS + (r % WORDS), v);
    }
}

// A target pixel of the normalising pass: hole = Wsum < Wmin, d = (double)Wsum, coverage = (float)(d / 16777216.0).
struct FsPixel {
    bool hole;
    double d;
    float cov;
};
DFX_HD FsPixel fs_pixel(fs_u64 ws, fs_u64 wmin) {
    FsPixel p;
    p.hole = ws < wmin;
    p.d = (double)ws;
    p.cov = (float)(p.d * 5.9604644775390625e-08); // 2^-24: the same bits as the division by 16777216.0
    return p;
}

// Which accesses of the normalising pass take a lane's 4 pixels at once (the lane quad of flow_quad.h).  `out` is the caller's.
struct FsWide {
    int work, out, hole, cov;
};
template <typename Wide>
Wide fs_wide(const FsSource &a, int words) {
    Wide wide;
    wide.work = ((size_t)a.work & 15) == 0 && (((long long)a.w * words) & 1) == 0;
    wide.out = 0;
    wide.hole = dfx_bytes4(a.hole, a.hole_pitch, a.hole_stride, 0);
    wide.cov = a.cov && dfx_planar_vec(a.cov, a.cov_stride, 0, a.cov_pitch) == 4;
    return wide;
}

// wave [i0, i0 + chunk) of the items of `args`: n and every shared per-item pointer but work, which every wave uses anew
inline void fs_step(FsSource &a, const FsSource &args, int i0, int chunk) {
    a.n = std::min(chunk, args.n - i0);
    a.flow += (long long)i0 * args.flow_stride;
    if (a.imp)
        a.imp += (long long)i0 * args.imp_stride;
    if (a.occ)
        a.occ += (long long)i0 * args.occ_stride;
    if (a.hole)
        a.hole += (long long)i0 * args.hole_stride;
    if (a.cov)
        a.cov += (long long)i0 * args.cov_stride;
}

#if defined(__HIPCC__)
// Enqueues on s the zero pass over `words` words (flow_scatter.hip): 16-byte stores, a single leading / trailing word where the
// base is 8 mod 16.
void fs_zero(hipStream_t s, fs_u64 *work, long long words);
inline dim3 fs_scatter_grid(const FsSource &a) {
    return dim3((unsigned)((a.w + FS_TW - 1) / FS_TW), (unsigned)((a.h + FS_TH - 1) / FS_TH), (unsigned)a.n);
}

// The scatter of a workgroup's tile; grid: fs_scatter_grid, FS_THREADS threads.  win: the kernel's LDS, fs_window_words(WORDS)
// words with WINDOW.  payload(landing, f, x, y, q) is called for a live landing: it fills q and says whether the pixel stays.
template <int WORDS, bool WINDOW, typename Payload>
__device__ __forceinline__ void fs_scatter_tile(fs_u64 *win, const FsSource &a, bool with_imp, bool with_occ, Payload payload) {
    const int tid = (int)threadIdx.x;
    const int x = (int)blockIdx.x * FS_TW + tid % FS_TW, y = (int)blockIdx.y * FS_TH + tid / FS_TW;
    const long long f = (long long)blockIdx.z;
    fs_u64 *work = a.work + f * (long long)a.h * a.w * WORDS;
    FsWindow o = {win, 0, 0};
    if (WINDOW) {
        fs_window_clear<WORDS>(win, tid, FS_THREADS);
        o = fs_window(win, a, f, (int)blockIdx.x, (int)blockIdx.y); // one broadcast load per plane, the same in every lane
        __syncthreads();
    }
    const FsLanding l = fs_landing(a, f, x, y, with_imp, with_occ);
    int q[WORDS - 1];
    if (l.live && payload(l, f, x, y, q))
        fs_taps(l, a.w, a.h, [&](int tx, int ty, fs_u64 wt) { fs_add<WORDS, WINDOW>(o, work, a.w, tx, ty, wt, q); });
    if (WINDOW) {
        __syncthreads();
        fs_window_flush<WORDS>(o, work, a.w, a.h, tid, FS_THREADS);
    }
}

// A lane's 4 * WORDS words of row y from pixel x on: 16-byte loads where wide and n == 4, zeros past the row's end.
template <int WORDS>
__device__ __forceinline__ void fs_load_quad(const FsSource &a, long long f, int x, int y, bool wide, int n, fs_u64 (&q)[4 * WORDS]) {
    const fs_u64 *p = a.work + ((f * a.h + y) * a.w + x) * WORDS;
    if (wide && n == 4) {
#pragma unroll
        for (int k = 0; k < 2 * WORDS; ++k) {
            const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(p)[k];
            q[2 * k] = v.x, q[2 * k + 1] = v.y;
        }
    } else {
        // an index the compiler cannot equate with the one above (as fc_row5 of the flow chain): it would otherwise hoist this
        // path's loads of the first pixel out of both paths and leave the wide one 8-byte loads in front of its 16-byte ones
        int k0 = 0;
        asm volatile("" : "+v"(k0));
#pragma unroll
        for (int k = 0; k < 4 * WORDS; ++k)
            q[k] = k < n * WORDS ? p[k0 + k] : 0ull;
    }
}
// the hole flags and the coverages of a quad to their planes
__device__ __forceinline__ void fs_store_masks(const FsSource &a, const FsWide &wide, long long f, int x, int y, int n,
                                               const unsigned (&oh)[4], const float (&oc)[4]) {
    if (a.hole)
        fq_store_u8(a.hole + f * a.hole_stride + (long long)y * a.hole_pitch + x, wide.hole != 0, n, oh);
    if (a.cov)
        fq_store_f32(a.cov + f * a.cov_stride + (long long)y * a.cov_pitch + x, wide.cov != 0, n, oc);
}
#endif
