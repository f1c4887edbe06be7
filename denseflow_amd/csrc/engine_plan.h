// engine_plan.h — the geometry every engine derives from (W, H, params): pyramid levels, frame-slot and pair-slot sizes,
// the size-dependent tables and the automatic batch.  Pure host arithmetic (no HIP): the engines' create() and set_size()
// run these, then make sure their buffers hold what the plan needs; the CPU suite compiles the header into
// tests/resize_plan_harness.cpp (tests/test_resize_plan_cpu.py).
//
// Every function fills a plan IN PLACE and must leave nothing of the plan it overwrites: a handle is re-planned for a new
// frame size inside its allocations (dfx_set_size), and a plan after another plan has to equal the plan from scratch.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/dfx.h"
#include "dfx_device.h"
#include "farneback_plan.h"

// Automatic batch (dfx_params.max_batch = 0): as many pairs as 256 Mpx of level-0 pixels hold (129 at 1080p), at most
// this many.  Small frames reach it: 2048 pairs of 224 x 224 are 103 Mpx — 0.4 of the 1080p batch — and a FlowBuffer
// only fills such a batch when it joins several clips (dfx_next_segments).
constexpr long long DFX_MAX_BATCH = 2048;

inline int dfx_plan_round(double v) { return (int)std::lrint(v); } // cvRound: round-half-even

inline int dfx_plan_batch(int W, int H, int max_batch) {
    if (max_batch > 0)
        return max_batch;
    const long long px0 = (long long)W * H;
    return (int)std::max<long long>(1, std::min<long long>(DFX_MAX_BATCH, (256LL << 20) / std::max<long long>(px0, 1)));
}
// The free-memory rule of every engine: halve the batch until B + 2 pairs take at most half of `free_bytes`.
inline int dfx_plan_fit_batch(int B, size_t per_pair, size_t free_bytes) {
    while (B > 1 && per_pair * (size_t)(B + 2) > free_bytes / 2)
        B /= 2;
    return B;
}

struct DfxPlanLevel {
    int w, h, pitch;
    long long off; // element offset inside a frame slot
};

// ---- TVL1 ---------------------------------------------------------------------------------------------------------
struct Tvl1Plan {
    int W = 0, H = 0;
    int nlevels = 0;
    DfxPlanLevel lv[DFX_LVL_MAX];
    long long frame_elems = 0;                 // floats of one pyramid of a frame slot (three of them: I, Ix, Iy)
    int n_planes = 0;                          // planes of a pair slot: PL_COUNT, PL_COUNT_GAMMA with tvl1_gamma != 0
    long long plane_stride = 0, slot_stride = 0; // floats between the planes of a pair slot / between pair slots
    int partials_stride = 0;                   // doubles per pair: >= workgroups of any step variant
    int batch = 0;                             // before the free-memory rule
    size_t per_pair = 0;                       // bytes the free-memory rule counts per pair
    bool slot_too_large = false;               // a pair slot reaches 4 GiB: 32-bit byte offsets cannot address it
};

inline void tvl1_plan(Tvl1Plan &pl, int W, int H, const dfx_params &p) {
    pl = Tvl1Plan();
    pl.W = W, pl.H = H;
    // pyramid (A.2 step 3): cvRound(size*scaleStep) per level; a level below 16 px is discarded
    long long off = 0;
    int w = W, h = H;
    for (int s = 0; s < p.tvl1_nscales && s < DFX_LVL_MAX; ++s) {
        if (s > 0) {
            w = dfx_plan_round(pl.lv[s - 1].w * p.tvl1_scale_step);
            h = dfx_plan_round(pl.lv[s - 1].h * p.tvl1_scale_step);
            if (w < 16 || h < 16)
                break;
        }
        pl.lv[s] = DfxPlanLevel{w, h, dfx_round_up(w, 64), off};
        off += (long long)pl.lv[s].pitch * h;
        pl.nlevels = s + 1;
    }
    for (int s = pl.nlevels; s < DFX_LVL_MAX; ++s)
        pl.lv[s] = DfxPlanLevel{0, 0, 0, 0};
    pl.frame_elems = off;
    pl.plane_stride = (long long)pl.lv[0].pitch * H;
    pl.n_planes = p.tvl1_gamma != 0.0 ? (int)PL_COUNT_GAMMA : (int)PL_COUNT; // u3, p31, p32 in both sets (dfx_device.h)
    pl.slot_stride = pl.plane_stride * pl.n_planes;
    // the tile kernels address a pair slot with 32-bit byte offsets behind a buffer descriptor (tvl1_device_common.h):
    // round_up(w, 64) x h x 64 B < 2^32, x 88 B with the 22 planes of a gamma handle
    pl.slot_too_large = (unsigned long long)pl.slot_stride * sizeof(float) >= (1ull << 32);
    pl.partials_stride = ((pl.lv[0].w + 63) / 64) * ((H + 3) / 4) + 64;
    pl.batch = dfx_plan_batch(W, H, p.max_batch);
    pl.per_pair = (size_t)pl.slot_stride * 4 + (size_t)W * H * 9 + (size_t)pl.frame_elems * 12;
}

// ---- Farneback ----------------------------------------------------------------------------------------------------
struct FarnPlanLevel {
    int w, h, pitch;
    long long r_off; // element offset of this level's R (5 planes) inside a frame slot
    double sigma;
    int half;    // Gaussian pre-blur half width (smoothSize / 2)
    int ker_off; // offset of this level's taps (centre first) in `taps`
    float ifx, ify;
};

struct FarnPlan {
    int W = 0, H = 0;
    int nlev = 0; // levels 0..nlev-1 (nlev = numLevelsCropped + 1)
    FarnPlanLevel lv[DFX_LVL_MAX];
    std::vector<float> taps; // the Gaussian pre-blur taps of every level, back to back
    long long frame_elems = 0;
    int pitch0 = 0;
    long long plane_stride = 0, slot_stride = 0;
    int batch = 0;
    size_t per_pair = 0;
    bool bad_kernel = false; // a level's Gaussian kernel size is not odd and positive
    // dfx_params.farn_fast_pyramids: a level below the coarsest has an odd width or height (upstream's pyrUp of the level
    // above it is then not this level's size: no result defined); fast_max_levels = the largest farn_num_levels this size
    // accepts
    bool odd_level = false;
    int fast_max_levels = 0;
};

// B.6: cv::getGaussianKernel(ksize, sigma, CV_32F); returns taps centre-first (k[0] = centre)
inline bool farn_gaussian_taps(int n, double sigma, std::vector<float> &half_out) {
    if (n < 1 || !(n & 1))
        return false;
    std::vector<double> k(n);
    bool fixed = false;
    if (sigma <= 0) {
        static const double t3[] = {0.25, 0.5, 0.25};
        static const double t5[] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
        static const double t7[] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
        const double *t = n == 3 ? t3 : n == 5 ? t5 : n == 7 ? t7 : nullptr;
        if (n == 1) {
            k[0] = 1.0;
            fixed = true;
        } else if (t) {
            std::copy(t, t + n, k.begin());
            fixed = true;
        }
    }
    if (!fixed) {
        const double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
        const double scale2x = -0.125 / (sx * sx);
        const int n2 = (n - 1) / 2;
        double sum = 0;
        for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
            k[i] = std::exp((double)(x * x) * scale2x);
            sum += k[i];
        }
        sum = sum * 2 + 1.0;
        const double mul = 1.0 / sum;
        for (int i = 0; i < n2; ++i)
            k[n - 1 - i] = k[i] = (double)(float)(k[i] * mul);
        k[n2] = (double)(float)mul;
    }
    const int half = n / 2;
    half_out.resize(half + 1);
    for (int j = 0; j <= half; ++j)
        half_out[j] = (float)k[half + j];
    return true;
}

// The taps of the Gaussian update window (upstream's updateFlow_gaussianBlur): getGaussianKernel(winSize, sigma, CV_32F)
// with sigma = (winSize / 2) * 0.3f — an integer division and a float product, widened to double — centre first.
// winSize 1 gives sigma 0 and hence the fixed table {1}.  They depend on the parameters only, not on the frame size.
inline bool farn_window_taps(int win_size, FarnWinTaps &out) {
    const double sigma = (double)((float)(win_size / 2) * 0.3f);
    std::vector<float> half;
    out = FarnWinTaps();
    if (win_size / 2 >= (int)(sizeof out.g / sizeof out.g[0]) || !farn_gaussian_taps(win_size, sigma, half))
        return false;
    std::copy(half.begin(), half.end(), out.g);
    return true;
}

// dfx_params.farn_fast_pyramids: level k is pyrDown of level k - 1, ((w + 1) / 2, (h + 1) / 2) of its size,
// and the flow climbs by pyrUp, which doubles a size: every level below the coarsest must be even both ways.  Returns the
// number of leading levels (from level 0) with even width and height — the largest level count a size accepts.
inline int farn_fast_even_levels(int W, int H) {
    int n = 0;
    for (int w = W, h = H; n < DFX_LVL_MAX && !(w & 1) && !(h & 1); w = (w + 1) / 2, h = (h + 1) / 2)
        ++n;
    return n;
}

// planes_per_slot: float planes of a pair slot (4 with M on chip, FARN_PL_COUNT otherwise: farneback_kernels.h)
inline void farn_plan(FarnPlan &pl, int W, int H, const dfx_params &p, int planes_per_slot) {
    pl = FarnPlan();
    pl.W = W, pl.H = H;
    constexpr int kMinSize = 32; // upstream MIN_SIZE
    pl.pitch0 = dfx_round_up(W, 64);
    // B.2: crop levels whose size would drop below MIN_SIZE
    double scale = 1;
    int cropped = 0;
    for (; cropped < p.farn_num_levels; cropped++) {
        scale *= p.farn_pyr_scale;
        if (W * scale < kMinSize || H * scale < kMinSize)
            break;
    }
    pl.nlev = cropped + 1;
    long long off = 0;
    for (int k = 0; k < DFX_LVL_MAX; ++k)
        pl.lv[k] = FarnPlanLevel{0, 0, 0, 0, 0.0, 0, 0, 0.f, 0.f};
    if (p.farn_fast_pyramids) {
        pl.fast_max_levels = farn_fast_even_levels(W, H);
        pl.odd_level = cropped > pl.fast_max_levels;
    }
    int fw = W, fh = H; // the (n + 1) / 2 chain of farn_fast_pyramids
    for (int k = 0; k < pl.nlev; ++k) {
        FarnPlanLevel &L = pl.lv[k];
        if (p.farn_fast_pyramids) { // level k is pyrDown of level k - 1; no Gaussian pre-blur, hence no sigma, smoothSize or taps
            L.w = fw, L.h = fh;
            fw = (fw + 1) / 2, fh = (fh + 1) / 2;
        } else {
            scale = 1;
            for (int i = 0; i < k; i++)
                scale *= p.farn_pyr_scale;
            L.sigma = (1. / scale - 1) * 0.5;
            int smooth = dfx_plan_round(L.sigma * 5) | 1;
            smooth = std::max(smooth, 3);
            L.half = smooth / 2;
            L.w = dfx_plan_round(W * scale);
            L.h = dfx_plan_round(H * scale);
            std::vector<float> taps;
            if (!farn_gaussian_taps(smooth, L.sigma, taps))
                pl.bad_kernel = true;
            L.ker_off = (int)pl.taps.size();
            pl.taps.insert(pl.taps.end(), taps.begin(), taps.end());
        }
        L.pitch = dfx_round_up(L.w, 64);
        L.r_off = off;
        off += 5LL * L.pitch * L.h;
        L.ifx = (float)(1.0 / ((double)L.w / (double)W)); // dsize given (E.1)
        L.ify = (float)(1.0 / ((double)L.h / (double)H));
    }
    pl.frame_elems = off;
    pl.plane_stride = (long long)pl.pitch0 * H;
    pl.slot_stride = pl.plane_stride * planes_per_slot;
    pl.batch = dfx_plan_batch(W, H, p.max_batch);
    pl.per_pair = (size_t)pl.slot_stride * 4 + (size_t)pl.frame_elems * 4 + (size_t)pl.plane_stride * 16 + (size_t)W * H * 9;
}

// ---- Brox ---------------------------------------------------------------------------------------------------------
struct BroxPlan {
    int W = 0, H = 0;
    std::vector<DfxPlanLevel> lv;
    long long pyr_elems = 0, frame_elems = 0; // one pyramid / the frame_planes pyramids of a frame slot
    long long plane_stride = 0, slot_stride = 0;
    int batch = 0;
    size_t per_pair = 0;
};

// frame_planes / pair_planes: BROX_FP_COUNT / BROX_PL_COUNT (brox_kernels.h)
inline void brox_plan(BroxPlan &pl, int W, int H, const dfx_params &p, int frame_planes, int pair_planes) {
    pl.lv.clear(); // the level count follows the size (24 at 3840 x 2160, 2 at 20 x 20)
    pl.W = W, pl.H = H;
    // pyramid sizes: scale accumulated in float, ceilf, until a side is <= 15 px or outer_iterations levels
    float scale = 1.0f;
    int pw = W, ph = H;
    long long off = 0;
    pl.lv.push_back(DfxPlanLevel{W, H, dfx_round_up(W, 64), 0});
    off += (long long)pl.lv[0].pitch * H;
    while (pw > 15 && ph > 15 && (int)pl.lv.size() < p.brox_outer_iterations && pl.lv.size() < 128) {
        scale *= p.brox_scale_factor;
        const int w = (int)std::ceil((float)W * scale), h = (int)std::ceil((float)H * scale);
        pl.lv.push_back(DfxPlanLevel{w, h, dfx_round_up(w, 64), off});
        off += (long long)pl.lv.back().pitch * h;
        pw = w;
        ph = h;
    }
    pl.pyr_elems = off;
    pl.frame_elems = off * frame_planes;
    pl.plane_stride = (long long)pl.lv[0].pitch * H;
    pl.slot_stride = pl.plane_stride * pair_planes;
    pl.batch = dfx_plan_batch(W, H, p.max_batch);
    pl.per_pair = (size_t)pl.slot_stride * 4 + (size_t)pl.frame_elems * 4 + (size_t)W * H * 9;
}

// ---- colour frames (DFX_ALGO_FRAMES) --------------------------------------------------------------------------------
// Frames per device batch: dfx_params.max_batch, or 32 Mpx of output frames (16 at 1080p: 100 MB of source frames per
// staging parity, enough blocks — 780 000 — to fill the device many times over).
inline int frames_plan_batch(int W, int H, int max_batch) {
    if (max_batch > 0)
        return max_batch;
    const long long px = (long long)W * H;
    return (int)std::max<long long>(1, std::min<long long>(256, (32ll << 20) / px));
}
