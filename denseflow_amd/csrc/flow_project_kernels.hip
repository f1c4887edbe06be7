// flow_project_kernels.hip — forward projection (splat) of planar flows on the device: the flow as seen from the frame it
// points to (t = 1, scale = -1: the inverse flow) or from a time t in between (scale = -t / 1 - t: F_{t->0} / F_{t->1}), with
// the pixels nothing lands on marked as holes.  The scatter is that of flow_scatter.h — its skip rules, landing test,
// importance, taps, weights and window — with the flow itself as the payload of FP_WORDS - 1 = 2 words beside the weight:
//     qu = (int)rintf(fminf(fmaxf(fu * 256.f, -8388608.f), 8388608.f));   qv likewise
//     Wsum[tap] += wt;   Su[tap] += wt * qu;   Sv[tap] += wt * qv      (64-bit, two's-complement wrap)
// and per target pixel, after all sources of the flow:
//     hole = Wsum < Wmin;  out = hole ? +0 : (float)(((double)S / (double)Wsum) * ((double)scale / 256.0))
//     coverage = (float)((double)Wsum / 16777216.0)
// All float operations are float32, each rounded on its own (the build's -ffp-contract=off), subnormals kept.
// tests/flow_project_ref.py is the same text in NumPy, and the device equals it bit for bit.
//
// Passes per wave of flows, all on one stream with nothing between them:
//   k_fs_zero       the zero pass of flow_scatter.hip over the wave's words;
//   k_fp_scatter    fs_scatter_tile, grid.z the flows of the wave.  FP_LDS_WINDOW 0: every add is a 64-bit global atomic, up
//                   to 12 per source pixel.  FP_LDS_WINDOW 1: through the 48 x 16 pixel window in LDS (18 KiB), flushed in
//                   rows of 1152 contiguous bytes.
//   k_fp_normalise  the lane quad of flow_quad.h: a lane's 12 words as six 16-byte loads where the workspace base is 16-byte
//                   aligned and W is even (8-byte loads otherwise), the planes and the hole mask through its quad stores.
#include "flow_project_kernels.h"

#ifndef FP_LDS_WINDOW
#define FP_LDS_WINDOW 1 // 0: the plain global-atomic scatter (kept for profiles/flow_project's A/B)
#endif

namespace {

typedef unsigned long long u64;

struct FpWide : FsWide {};

// IMP: with an importance plane; OCC: with an occlusion mask; LDSW: through the LDS window.  grid: fs_scatter_grid
template <bool IMP, bool OCC, bool LDSW>
__global__ __launch_bounds__(FS_THREADS) void k_fp_scatter(FpArgs a) {
    __shared__ u64 win[LDSW ? fs_window_words(FP_WORDS) : 1];
    fs_scatter_tile<FP_WORDS, LDSW>(win, a, IMP, OCC, [](const FsLanding &l, long long, int, int, int (&q)[2]) {
        q[0] = (int)rintf(__builtin_fminf(__builtin_fmaxf(l.fu * 256.0f, -8388608.0f), 8388608.0f));
        q[1] = (int)rintf(__builtin_fminf(__builtin_fmaxf(l.fv * 256.0f, -8388608.0f), 8388608.0f));
        return true;
    });
}

// grid: fq_grid(w, h, flows of the wave)
__global__ __launch_bounds__(256) void k_fp_normalise(FpArgs a, FpWide wide) {
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long f = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    u64 q[4 * FP_WORDS];
    fs_load_quad<FP_WORDS>(a, f, x, y, wide.work != 0, n, q);
    float ou[4], ov[4], oc[4];
    unsigned oh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const FsPixel p = fs_pixel(q[3 * e], a.wmin);
        const float u = (float)(((double)(long long)q[3 * e + 1] / p.d) * a.sc);
        const float v = (float)(((double)(long long)q[3 * e + 2] / p.d) * a.sc);
        ou[e] = p.hole ? 0.0f : u;
        ov[e] = p.hole ? 0.0f : v;
        oh[e] = p.hole ? 1u : 0u;
        oc[e] = p.cov;
    }
    if (a.out)
        fq_store_flow(a.out + f * a.out_stride + (long long)y * a.out_pitch + x, a.out_plane, wide.out != 0, n, ou, ov);
    fs_store_masks(a, wide, f, x, y, n, oh, oc);
}

template <bool IMP, bool OCC>
void fp_scatter_as(hipStream_t s, const FpArgs &a) {
    hipLaunchKernelGGL((k_fp_scatter<IMP, OCC, FP_LDS_WINDOW != 0>), fs_scatter_grid(a), dim3(FS_THREADS), 0, s, a);
}

FpWide fp_wide(const FpArgs &args) {
    FpWide wide = fs_wide<FpWide>(args, FP_WORDS);
    wide.out = args.out && dfx_planar_vec(args.out, args.out_stride, args.out_plane, args.out_pitch) == 4;
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
        fs_step(a, args, i0, chunk);
        if (a.out)
            a.out += (long long)i0 * args.out_stride;
        fs_zero(s, a.work, per_flow * a.n);
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
