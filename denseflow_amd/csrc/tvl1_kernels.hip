// tvl1_kernels.hip — hand-written gfx950 kernels for the -a=tvl1 hot path.
//
// Replaces the CUDA kernels that cv::cuda::OpticalFlowDual_TVL1::calc launches for the reference
// (src/denseflow_gpu.cpp:327): centeredGradientKernel, warpBackwardKernel, estimateUKernel,
// estimateDualVariablesKernel, cuda::sum, resize, convertTo, multiply, setTo, merge (SURVEY.md §2
// kernel inventory).  Wavefronts are 64 wide; tiles are 64 columns so one wave touches one
// 256-byte row segment per plane.
//
// Compiled with -ffp-contract=off (see tvl1_math.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "dfx_device.h"
#include "flow_quad.h" // dfx_planar_merge_tile
#include "tvl1_kernels.h"
#include "tvl1_math.h"
#include "tvl1_math_pk.h"
#include "tvl1_device_common.h"

// ------------------------------------------------------------------------------------------------
// frame preparation: u8 -> f32 (E.2), pyramid resize (E.1), centred gradient (A.3)

__global__ __launch_bounds__(256) void k_u8_to_f32(const unsigned char *src, long long src_frame_stride,
                                                   long long src_pitch, const int *frame_slots, float *dst,
                                                   long long dst_frame_stride, int w, int h, int pitch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h)
        return;
    const int z = blockIdx.z;
    const unsigned char *s = src + (long long)z * src_frame_stride + (long long)y * src_pitch;
    float *d = dst + (long long)frame_slots[z] * dst_frame_stride + (long long)y * pitch;
    d[x] = (float)s[x];
}

// bilinear(src, dx*ifx, dy*ify), no half-pixel centring (E.1); accumulation order as upstream.
__device__ __forceinline__ float resize_linear_px(const float *src, int sw, int sh, int spitch, int dx, int dy,
                                                  float ifx, float ify) {
    const float sx = (float)dx * ifx;
    const float sy = (float)dy * ify;
    const int x1 = (int)floorf(sx), y1 = (int)floorf(sy);
    const int x2 = x1 + 1, y2 = y1 + 1;
    const int x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
    const int x1r = min(x1, sw - 1), y1r = min(y1, sh - 1);
    float out = 0.0f;
    out = out + src[(long long)y1r * spitch + x1r] * (((float)x2 - sx) * ((float)y2 - sy));
    out = out + src[(long long)y1r * spitch + x2r] * ((sx - (float)x1) * ((float)y2 - sy));
    out = out + src[(long long)y2r * spitch + x1r] * (((float)x2 - sx) * (sy - (float)y1));
    out = out + src[(long long)y2r * spitch + x2r] * ((sx - (float)x1) * (sy - (float)y1));
    return out;
}

__global__ __launch_bounds__(256) void k_pyr_down(float *frame_I, long long frame_stride, const int *frame_slots,
                                                  long long src_off, int sw, int sh, int spitch, long long dst_off,
                                                  int dw, int dh, int dpitch, float ifx, float ify) {
    const DfxBlockXY blk = dfx_block_xy(); // XCD-aware (dfx_device.h): neighbouring rows share one L2
    const int x = blk.x * 64 + (threadIdx.x & 63);
    const int y = blk.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh)
        return;
    float *base = frame_I + (long long)frame_slots[blockIdx.z] * frame_stride;
    base[dst_off + (long long)y * dpitch + x] = resize_linear_px(base + src_off, sw, sh, spitch, x, y, ifx, ify);
}

__global__ __launch_bounds__(256) void k_centered_gradient(const float *frame_I, float *frame_Ix, float *frame_Iy,
                                                           long long frame_stride, const int *frame_slots,
                                                           long long off, int w, int h, int pitch) {
    const DfxBlockXY blk = dfx_block_xy(); // XCD-aware (dfx_device.h): neighbouring rows share one L2
    const int x = blk.x * 64 + (threadIdx.x & 63);
    const int y = blk.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h)
        return;
    const long long fb = (long long)frame_slots[blockIdx.z] * frame_stride + off;
    const float *I = frame_I + fb;
    const int xp = min(x + 1, w - 1), xm = max(x - 1, 0);
    const int yp = min(y + 1, h - 1), ym = max(y - 1, 0);
    frame_Ix[fb + (long long)y * pitch + x] = 0.5f * (I[(long long)y * pitch + xp] - I[(long long)y * pitch + xm]);
    frame_Iy[fb + (long long)y * pitch + x] = 0.5f * (I[(long long)yp * pitch + x] - I[(long long)ym * pitch + x]);
}

// ------------------------------------------------------------------------------------------------
// level control kernels

// One thread per pair: (re)arm the state machine for a level.
__global__ void k_tvl1_level_begin(Tvl1LevelCtx c, int first_level) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= c.n_pairs)
        return;
    Tvl1State *st = c.state + b;
    st->cur = first_level ? 0 : (st->cur ^ 1); // the up-sampled flow was written into the other set
    st->warp = 0;
    st->phase = (c.loop.warps > 0) ? TVL1_PH_WARP : TVL1_PH_LEVEL_DONE;
    st->seg_step0 = 0;
    st->seg_n0 = 0;
    st->next_check = TVL1_NO_CHECK;
    st->n_checks = 0;
    st->prev_error = 0.0;
    st->thr = c.thr;
    for (int i = 0; i < TVL1_MAX_WARPS; ++i)
        st->iters[i] = 0;
    st->ticket = 0u;
    st->step_work = 0;
    st->head_work = 0;
}

// p = 0 once per level (A.3; not with c.head: see dfx_device.h); u = 0 at the coarsest level (A.2 step 4). Reads state.cur.
__global__ __launch_bounds__(256) void k_tvl1_zero_planes(Tvl1LevelCtx c, int first_level) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= c.pitch || y >= c.h)
        return;
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    const long long o = (long long)y * c.pitch + x;
    if (!c.head) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            pair_plane(c, b, PL_P11_0 + 4 * cur + k)[o] = 0.0f;
    }
    if (first_level) {
        pair_plane(c, b, PL_U1_0 + 2 * cur)[o] = 0.0f;
        pair_plane(c, b, PL_U2_0 + 2 * cur)[o] = 0.0f;
    }
}

// u(level s-1) = resize(u(level s), dsize) * (1/scaleStep)  (A.2 step 5). `c` describes level s (source);
// the destination geometry is passed explicitly.  Source = set cur, destination = set cur^1.
__global__ __launch_bounds__(256) void k_tvl1_upsample_u(Tvl1LevelCtx c, int dw, int dh, int dpitch, float ifx,
                                                         float ify, float up) {
    const DfxBlockXY blk = dfx_block_xy(); // XCD-aware (dfx_device.h): neighbouring rows share one L2
    const int x = blk.x * 64 + (threadIdx.x & 63);
    const int y = blk.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh)
        return;
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    const long long o = (long long)y * dpitch + x;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float *src = pair_plane(c, b, PL_U1_0 + 2 * cur + k);
        float *dst = pair_plane(c, b, PL_U1_0 + 2 * (cur ^ 1) + k);
        const float r = resize_linear_px(src, c.w, c.h, c.pitch, x, y, ifx, ify);
        dst[o] = r * up;
    }
}

// flow = merge(u1, u2) (A.2 step 6, E.4): interleaved (u, v), dense rows of w pairs.
__global__ __launch_bounds__(256) void k_tvl1_merge(Tvl1LevelCtx c, float *out, long long out_stride) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= c.w || y >= c.h)
        return;
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    const long long o = (long long)y * c.pitch + x;
    float2 v;
    v.x = pair_plane(c, b, PL_U1_0 + 2 * cur)[o];
    v.y = pair_plane(c, b, PL_U2_0 + 2 * cur)[o];
    reinterpret_cast<float2 *>(out + (long long)b * out_stride)[(long long)y * c.w + x] = v;
}

// The same flow as two planes (DfxPlanarOut, dfx_device.h): u1 and u2 each go to the caller's plane, bounded on the way.
__global__ __launch_bounds__(256) void k_tvl1_merge_planar(Tvl1LevelCtx c, DfxPlanarOut o) {
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    dfx_planar_merge_tile(o, b, pair_plane(c, b, PL_U1_0 + 2 * cur), pair_plane(c, b, PL_U2_0 + 2 * cur), c.w, c.h, c.pitch);
}

// ------------------------------------------------------------------------------------------------
// A.6 primal update of one pixel from planes in global memory (simple variant), NC = 2 channels (u1, u2) or 3 (with the
// illumination channel u3 of dfx_params.tvl1_gamma, SURVEY.md Appendix A "with gamma"; its planes: see further down).
// With NC = 2 this is tvl1_threshold followed by v + theta * div, operation for operation: no gamma term is formed.

// channels 0 and 1 live where the two-channel kernels have always read them
static_assert(tvl1_pl_u(0, 0) == PL_U1_0 && tvl1_pl_u(1, 0) == PL_U2_0 && tvl1_pl_u(0, 1) == PL_U1_0 + 2 &&
                  tvl1_pl_u(1, 1) == PL_U2_0 + 2,
              "u1 / u2 of set S are planes PL_U1_0 + 2S, PL_U2_0 + 2S");
static_assert(tvl1_pl_p(0, 0) == PL_P11_0 && tvl1_pl_p(0, 0) + 1 == PL_P12_0 && tvl1_pl_p(1, 0) == PL_P21_0 &&
                  tvl1_pl_p(1, 0) + 1 == PL_P22_0 && tvl1_pl_p(0, 1) == PL_P11_0 + 4 && tvl1_pl_p(0, 1) + 1 == PL_P12_0 + 4 &&
                  tvl1_pl_p(1, 1) == PL_P21_0 + 4 && tvl1_pl_p(1, 1) + 1 == PL_P22_0 + 4,
              "p11, p12, p21, p22 of set S are planes PL_P11_0 + 4S ... PL_P22_0 + 4S");

template <int NC>
struct PlanesRO {
    const float *I1wx, *I1wy, *grad, *rho_c, *u[NC], *pa[NC], *pb[NC];
};

template <int NC>
__device__ __forceinline__ void estimate_u_px(const PlanesRO<NC> &P, int pitch, int x, int y, float l_t, float theta,
                                              float gamma, float (&un)[NC], float (&uo)[NC]) {
    const long long o = (long long)y * pitch + x;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
        uo[ch] = P.u[ch][o];
    const float I1wx = P.I1wx[o], I1wy = P.I1wy[o], grad = P.grad[o];
    float dot = I1wx * uo[0] + I1wy * uo[1];
    if (NC == 3)
        dot = dot + gamma * uo[NC - 1];
    const float rho = P.rho_c[o] + dot;
    const float lg = l_t * grad;
    const float fi = tvl1_div(-rho, grad);
    const bool c1 = rho < -lg, c2 = rho > lg, c3 = grad > FLT_EPSILON;
    const float w[3] = {I1wx, I1wy, gamma};
    const bool hl = x > 0, hu = y > 0;
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        const float a = l_t * w[ch], bq = fi * w[ch];
        const float d = c1 ? a : (c2 ? -a : (c3 ? bq : 0.0f));
        const float pal = hl ? P.pa[ch][o - 1] : 0.0f, pbu = hu ? P.pb[ch][o - pitch] : 0.0f;
        un[ch] = (uo[ch] + d) + theta * tvl1_divergence(P.pa[ch][o], pal, P.pb[ch][o], pbu, hl, hu);
    }
}

// A workgroup has stored its pixels of a step: where the step ends its segment, the segment tail (tvl1_device_common.h).
__device__ __forceinline__ void end_iter_tile(const Tvl1LevelCtx &c, int b, Tvl1State *st, const Tvl1StepPlan &plan,
                                              unsigned nblk, int slot, int step_id, double dsum, double *lds_red,
                                              int *lds_flag) {
    if (plan.is_last)
        end_segment_tile(c, b, st, plan.do_check != 0, nblk, slot, step_id, dsum, lds_red, lds_flag,
                         [&](Tvl1State &s, double err) { tvl1_end_segment(s, c.loop, plan, step_id, err); });
}

// A.5 for one pixel of the simple kernel's warp phase (the warp reads u1, u2 only, with or without u3)
__device__ __forceinline__ void simple_warp_px(const Tvl1LevelCtx &c, int b, int cur, int x, int y) {
    const long long o = (long long)y * c.pitch + x;
    const PairDesc pd = c.pairs[b];
    const float *I0 = c.frame_I + (long long)pd.frame_a * c.frame_stride + c.lvl_off;
    const long long fb = (long long)pd.frame_b * c.frame_stride + c.lvl_off;
    const float u1v = pair_plane(c, b, PL_U1_0 + 2 * cur)[o];
    const float u2v = pair_plane(c, b, PL_U2_0 + 2 * cur)[o];
    const WarpOut r = warp_backward_px(I0, c.frame_I + fb, c.frame_Ix + fb, c.frame_Iy + fb, c.w, c.h, c.pitch, x, y, u1v, u2v);
    pair_plane(c, b, PL_I1WX)[o] = r.I1wx;
    pair_plane(c, b, PL_I1WY)[o] = r.I1wy;
    pair_plane(c, b, PL_GRAD)[o] = r.grad;
    pair_plane(c, b, PL_RHOC)[o] = r.rho_c;
}

// ------------------------------------------------------------------------------------------------
// The step kernel, simple variant (impl 1, the cross-check form; NC = 3 with tvl1_gamma): one pixel per thread, one inner
// iteration per step.  Each thread recomputes the new u of its right and lower neighbours instead of exchanging it,
// so a step is a single launch with no intra-kernel dependency (the fused variant shares them
// through LDS).  Reads ping-pong set `src`, writes set `src ^ 1`.

template <int NC>
__global__ __launch_bounds__(256) void k_tvl1_step_simple(Tvl1LevelCtx c, int step_id) {
    __shared__ double lds_red[8];
    __shared__ int lds_flag;

    const int b = blockIdx.z;
    Tvl1State *st = c.state + b;
    const int phase = st->phase;
    if (phase == TVL1_PH_LEVEL_DONE)
        return;

    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool inside = x < c.w && y < c.h;
    const unsigned nblk = gridDim.x * gridDim.y;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const long long o = (long long)y * c.pitch + x;

    if (phase == TVL1_PH_WARP) {
        if (inside)
            simple_warp_px(c, b, st->cur, x, y);
        end_warp_tile(c, b, st, nblk, step_id, &lds_flag);
        return;
    }

    // ---- phase ITER
    const Tvl1State s0 = *st;
    const Tvl1StepPlan plan = tvl1_plan_step(s0, c.loop, step_id);
    if (plan.n_iters <= 0)
        return;
    const int S = plan.src, D = S ^ 1;
    PlanesRO<NC> P;
    P.I1wx = pair_plane(c, b, PL_I1WX);
    P.I1wy = pair_plane(c, b, PL_I1WY);
    P.grad = pair_plane(c, b, PL_GRAD);
    P.rho_c = pair_plane(c, b, PL_RHOC);
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        P.u[ch] = pair_plane(c, b, tvl1_pl_u(ch, S));
        P.pa[ch] = pair_plane(c, b, tvl1_pl_p(ch, S));
        P.pb[ch] = pair_plane(c, b, tvl1_pl_p(ch, S) + 1);
    }

    double dsum = 0.0;
    if (inside) {
        const float l_t = c.k.l_t, theta = c.k.theta, gamma = c.k.gamma;
        float un[NC], uo[NC];
        estimate_u_px(P, c.pitch, x, y, l_t, theta, gamma, un, uo);
        // forward differences of the NEW u with clamp (A.7): neighbours are recomputed here
        float ux[NC] = {}, uy[NC] = {};
        if (x + 1 < c.w) {
            float a[NC], t[NC];
            estimate_u_px(P, c.pitch, x + 1, y, l_t, theta, gamma, a, t);
#pragma unroll
            for (int ch = 0; ch < NC; ++ch)
                ux[ch] = a[ch] - un[ch];
        }
        if (y + 1 < c.h) {
            float a[NC], t[NC];
            estimate_u_px(P, c.pitch, x, y + 1, l_t, theta, gamma, a, t);
#pragma unroll
            for (int ch = 0; ch < NC; ++ch)
                uy[ch] = a[ch] - un[ch];
        }
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
            float pa = P.pa[ch][o], pb = P.pb[ch][o];
            tvl1_dual(pa, pb, ux[ch], uy[ch], c.k.taut, c.k.hyp);
            pair_plane(c, b, tvl1_pl_u(ch, D))[o] = un[ch];
            pair_plane(c, b, tvl1_pl_p(ch, D))[o] = pa;
            pair_plane(c, b, tvl1_pl_p(ch, D) + 1)[o] = pb;
        }
        if (plan.do_check) {
            const float e1 = uo[0] - un[0], e2 = uo[1] - un[1];
            dsum = (double)(e1 * e1 + e2 * e2); // diff(y,x) is stored as float upstream; u3 does not enter it
        }
    }

    end_iter_tile(c, b, st, plan, nblk, blk, step_id, dsum, lds_red, &lds_flag);
}

// ------------------------------------------------------------------------------------------------
// The step kernel, fused variant: one workgroup owns a 64 x TH tile (256 threads, TH/4 consecutive
// rows per thread) and advances it by up to K inner iterations per launch.
//
//   * the four per-warp constants (I1wx, I1wy, grad, rho_c) and the thread's own u/p values stay in
//     registers for the whole step; only neighbour values travel through LDS (6 planes x TH x 64);
//   * a K-pixel halo on every side is recomputed redundantly, so after K iterations the inner
//     (64-2K) x (TH-2K) region holds exactly the values the unfused order produces (same functions,
//     same op order, no contraction) and only that region is written back;
//   * HBM traffic per inner iteration drops from 64 B/px to 64/(K*eff) B/px and a level needs K x
//     fewer launches (the coarse levels are launch-latency bound otherwise);
//   * workgroup -> tile mapping is XCD-aware: consecutive ids go round-robin over the 8 XCDs, so each
//     XCD gets one contiguous run of tiles and halo rows are shared inside one L2.
//
// LDS layout: plane-major [6][TH][64] floats; a wave reads 64 consecutive floats of one row
// (ds_read_b32, conflict-free).

enum { L_P11 = 0, L_P12, L_P21, L_P22, L_U1, L_U2, L_PLANES };

// Load a tile, advance it n_iters inner iterations, store the owned region.  INTERIOR = the whole
// tile including its halo lies strictly inside the image (every pixel has all four neighbours), so
// no border predicate is evaluated at all; the generic instantiation handles tiles on the border.
// Returns this thread's share of sum(diff) of the last iteration when do_check.
template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ double fused_tile_iterate(const Tvl1LevelCtx &c, int b, float (*lds)[TH][64], int S,
                                                     int n_iters, bool do_check, int K, int x0, int y0) {
    constexpr int TW = 64;
    constexpr int RPT = TH / NW; // consecutive rows per thread; NW waves stack vertically
    const int D = S ^ 1;
    const int tid = threadIdx.x;
    const int lx = tid & 63, rg = tid >> 6;
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool has_left = INTERIOR || gx > 0, has_right = INTERIOR || gx + 1 < c.w;
    const int lxl = max(lx - 1, 0), lxr = min(lx + 1, TW - 1);
    const bool col_owned = lx >= K && lx < TW - K && col_in;
    const int ly0 = rg * RPT;

    float kwx[RPT], kwy[RPT], kgr[RPT], krc[RPT];
    float u1[RPT], u2[RPT], p11[RPT], p12[RPT], p21[RPT], p22[RPT];
    {
        const float *g_wx = pair_plane(c, b, PL_I1WX), *g_wy = pair_plane(c, b, PL_I1WY);
        const float *g_gr = pair_plane(c, b, PL_GRAD), *g_rc = pair_plane(c, b, PL_RHOC);
        const float *g_u1 = pair_plane(c, b, PL_U1_0 + 2 * S), *g_u2 = pair_plane(c, b, PL_U2_0 + 2 * S);
        const float *g_p11 = pair_plane(c, b, PL_P11_0 + 4 * S), *g_p12 = pair_plane(c, b, PL_P12_0 + 4 * S);
        const float *g_p21 = pair_plane(c, b, PL_P21_0 + 4 * S), *g_p22 = pair_plane(c, b, PL_P22_0 + 4 * S);
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int ly = ly0 + i;
            const int gy = y0 + ly;
            const bool in = INTERIOR || (col_in && gy >= 0 && gy < c.h);
            const long long o = in ? ((long long)gy * c.pitch + gx) : 0; // clamp: masked lanes read element 0
            const float m = in ? 1.0f : 0.0f;
            // unconditional loads (address clamped), masked by multiplication-free select below
            const float a0 = g_wx[o], a1 = g_wy[o], a2 = g_gr[o], a3 = g_rc[o];
            const float a4 = g_u1[o], a5 = g_u2[o], a6 = g_p11[o], a7 = g_p12[o], a8 = g_p21[o], a9 = g_p22[o];
            kwx[i] = in ? a0 : 0.0f;
            kwy[i] = in ? a1 : 0.0f;
            kgr[i] = in ? a2 : 0.0f;
            krc[i] = in ? a3 : 0.0f;
            u1[i] = in ? a4 : 0.0f;
            u2[i] = in ? a5 : 0.0f;
            p11[i] = in ? a6 : 0.0f;
            p12[i] = in ? a7 : 0.0f;
            p21[i] = in ? a8 : 0.0f;
            p22[i] = in ? a9 : 0.0f;
            (void)m;
            lds[L_P11][ly][lx] = p11[i];
            lds[L_P12][ly][lx] = p12[i];
            lds[L_P21][ly][lx] = p21[i];
            lds[L_P22][ly][lx] = p22[i];
        }
    }
    __syncthreads();

    double dsum = 0.0;
    for (int it = 0; it < n_iters; ++it) {
        const bool chk = do_check && (it == n_iters - 1);
        // ---- primal update (A.6): needs p at (x-1,y) and (x,y-1)
        float p12u = lds[L_P12][max(ly0 - 1, 0)][lx];
        float p22u = lds[L_P22][max(ly0 - 1, 0)][lx];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int ly = ly0 + i;
            const int gy = y0 + ly;
            float v1, v2;
            tvl1_threshold(kwx[i], kwy[i], kgr[i], krc[i], u1[i], u2[i], c.k.l_t, v1, v2);
            const float p11l = lds[L_P11][ly][lxl], p21l = lds[L_P21][ly][lxl];
            float div1, div2;
            if (INTERIOR) {
                div1 = tvl1_divergence_interior(p11[i], p11l, p12[i], p12u);
                div2 = tvl1_divergence_interior(p21[i], p21l, p22[i], p22u);
            } else {
                const bool has_up = gy > 0;
                div1 = tvl1_divergence(p11[i], p11l, p12[i], p12u, has_left, has_up);
                div2 = tvl1_divergence(p21[i], p21l, p22[i], p22u, has_left, has_up);
            }
            const float u1n = v1 + c.k.theta * div1;
            const float u2n = v2 + c.k.theta * div2;
            if (chk) {
                const bool owned = col_owned && ly >= K && ly < TH - K && (INTERIOR || (gy >= 0 && gy < c.h));
                const float e1 = u1[i] - u1n, e2 = u2[i] - u2n;
                const float dv = e1 * e1 + e2 * e2; // diff(y,x) is a float upstream
                dsum += owned ? (double)dv : 0.0;
            }
            u1[i] = u1n;
            u2[i] = u2n;
            lds[L_U1][ly][lx] = u1n;
            lds[L_U2][ly][lx] = u2n;
            p12u = p12[i]; // the row below reads this row's (still old) p12/p22 as its upper neighbour
            p22u = p22[i];
        }
        __syncthreads();
        // ---- dual update (A.7): needs the NEW u at (x+1,y) and (x,y+1), clamped at the image border
        const float u1bot = lds[L_U1][min(ly0 + RPT, TH - 1)][lx];
        const float u2bot = lds[L_U2][min(ly0 + RPT, TH - 1)][lx];
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int ly = ly0 + i;
            const int gy = y0 + ly;
            float u1r = lds[L_U1][ly][lxr], u2r = lds[L_U2][ly][lxr];
            float u1d = (i + 1 < RPT) ? u1[i + 1] : u1bot;
            float u2d = (i + 1 < RPT) ? u2[i + 1] : u2bot;
            if (!INTERIOR) {
                const bool has_down = gy + 1 < c.h;
                u1r = has_right ? u1r : u1[i];
                u2r = has_right ? u2r : u2[i];
                u1d = has_down ? u1d : u1[i];
                u2d = has_down ? u2d : u2[i];
            }
            tvl1_dual(p11[i], p12[i], u1r - u1[i], u1d - u1[i], c.k.taut, c.k.hyp);
            tvl1_dual(p21[i], p22[i], u2r - u2[i], u2d - u2[i], c.k.taut, c.k.hyp);
            lds[L_P11][ly][lx] = p11[i];
            lds[L_P12][ly][lx] = p12[i];
            lds[L_P21][ly][lx] = p21[i];
            lds[L_P22][ly][lx] = p22[i];
        }
        __syncthreads();
    }

    // ---- write back the owned region into the other ping-pong set
    {
        float *g_u1 = pair_plane(c, b, PL_U1_0 + 2 * D), *g_u2 = pair_plane(c, b, PL_U2_0 + 2 * D);
        float *g_p11 = pair_plane(c, b, PL_P11_0 + 4 * D), *g_p12 = pair_plane(c, b, PL_P12_0 + 4 * D);
        float *g_p21 = pair_plane(c, b, PL_P21_0 + 4 * D), *g_p22 = pair_plane(c, b, PL_P22_0 + 4 * D);
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int ly = ly0 + i;
            const int gy = y0 + ly;
            if (col_owned && ly >= K && ly < TH - K && (INTERIOR || (gy >= 0 && gy < c.h))) {
                int gyo = gy;
                asm volatile("" : "+v"(gyo)); // recompute the offset here: held from the loads, it costs two VGPRs of scratch
                const long long o = (long long)gyo * c.pitch + gx;
                g_u1[o] = u1[i];
                g_u2[o] = u2[i];
                g_p11[o] = p11[i];
                g_p12[o] = p12[i];
                g_p21[o] = p21[i];
                g_p22[o] = p22[i];
            }
        }
    }
    return dsum;
}

#include "tvl1_tile.h" // RowMap, TileState, tile_issue_loads / tile_consume / tile_iterate_trap / tile_store

// Backward warp (A.5) of the owned region of one tile: lane = column, the NW waves interleave over its rows
// (coalesced 256-B rows).  This phase is latency-bound (PMC: 2/3 of wave cycles waiting), so the loads are
// batched: first u1/u2/I0 of every row of the thread, then the 4x4 windows of two pixels at a time.
// WRITE_GRAD: the scalar tile function reads the grad plane; the packed one rebuilds grad from I1wx, I1wy.
template <int TH, int NW, bool WRITE_GRAD>
__device__ __forceinline__ void tile_warp(const Tvl1LevelCtx &c, int b, int cur, int K, int x0, int y0) {
    constexpr int TW = 64;
    const int SW = TW - 2 * K, SH = TH - 2 * K;
    const int tid = threadIdx.x;
    const PairDesc pd = c.pairs[b];
    const float *I0 = c.frame_I + (long long)pd.frame_a * c.frame_stride + c.lvl_off;
    const long long fb = (long long)pd.frame_b * c.frame_stride + c.lvl_off;
    const float *u1p = pair_plane(c, b, PL_U1_0 + 2 * cur);
    const float *u2p = pair_plane(c, b, PL_U2_0 + 2 * cur);
    float *o_wx = pair_plane(c, b, PL_I1WX), *o_wy = pair_plane(c, b, PL_I1WY);
    float *o_gr = pair_plane(c, b, PL_GRAD), *o_rc = pair_plane(c, b, PL_RHOC);
    constexpr int MAXRK = (TH + NW - 1) / NW; // rows per thread (K < 4 owns more rows than K >= 4)
    const int lane = tid & 63, wave = tid >> 6;
    const int x = x0 + K + lane;
    const bool col_ok = lane < SW && x < c.w;
    const float *P1 = c.frame_I + fb, *P1x = c.frame_Ix + fb, *P1y = c.frame_Iy + fb;
    float u1r[MAXRK], u2r[MAXRK], i0r[MAXRK];
    bool ok[MAXRK];
#pragma unroll
    for (int j = 0; j < MAXRK; ++j) {
        const int ly = wave + NW * j;
        const int y = y0 + K + ly;
        ok[j] = col_ok && ly < SH && y < c.h;
        const long long o = ok[j] ? ((long long)y * c.pitch + x) : 0;
        u1r[j] = u1p[o];
        u2r[j] = u2p[o];
        i0r[j] = I0[o];
    }
#pragma unroll
    for (int j0 = 0; j0 < MAXRK; j0 += 2) {
        WarpTaps Ta, Tb;
        const int ya = y0 + K + wave + NW * j0, yb = ya + NW;
        const bool oka = ok[j0], okb = (j0 + 1 < MAXRK) && ok[j0 + 1 < MAXRK ? j0 + 1 : j0];
        if (oka)
            warp_fetch(Ta, P1, P1x, P1y, c.w, c.h, c.pitch, x, ya, u1r[j0], u2r[j0]);
        if (okb)
            warp_fetch(Tb, P1, P1x, P1y, c.w, c.h, c.pitch, x, yb, u1r[j0 + 1 < MAXRK ? j0 + 1 : j0],
                       u2r[j0 + 1 < MAXRK ? j0 + 1 : j0]);
        if (oka) {
            const long long o = (long long)ya * c.pitch + x;
            const WarpOut r = warp_finish(Ta, i0r[j0], x, ya, u1r[j0], u2r[j0]);
            o_wx[o] = r.I1wx;
            o_wy[o] = r.I1wy;
            if (WRITE_GRAD)
                o_gr[o] = r.grad;
            o_rc[o] = r.rho_c;
        }
        if (okb) {
            const int j1 = j0 + 1 < MAXRK ? j0 + 1 : j0;
            const long long o = (long long)yb * c.pitch + x;
            const WarpOut r = warp_finish(Tb, i0r[j1], x, yb, u1r[j1], u2r[j1]);
            o_wx[o] = r.I1wx;
            o_wy[o] = r.I1wy;
            if (WRITE_GRAD)
                o_gr[o] = r.grad;
            o_rc[o] = r.rho_c;
        }
    }
}

template <int TH, int NW, bool INTERIOR, int MATH, bool LK>
__device__ __forceinline__ double fused_tile_iterate_trap(const Tvl1LevelCtx &c, int b, float (*lds)[TH][64],
                                                          float (*bnd)[2 * NW][64], int S, int n_iters, bool do_check,
                                                          int K, int x0, int y0, bool own_lo, bool own_hi) {
    float pf[PF_PLANES][TH / NW / 2][2];
    TileState<TH / NW / 2> T;
    const int role = RowMap<TH, NW>::who();
    tile_issue_loads<TH, NW, INTERIOR>(c, b, S, x0, y0, pf);
    tile_consume<TH, NW, INTERIOR, MATH, LK>(c, x0, y0, pf, T, lds, bnd);
    __syncthreads();
    double dsum;
    if (role * (TH / NW / 2) < K) // only roles that hold halo rows carry the per-float2 skip tests
        dsum = tile_iterate_trap<TH, NW, INTERIOR, true, MATH, LK>(c, T, lds, bnd, n_iters, do_check, K, x0, y0, role,
                                                                   own_lo, own_hi);
    else
        dsum = tile_iterate_trap<TH, NW, INTERIOR, false, MATH, LK>(c, T, lds, bnd, n_iters, do_check, K, x0, y0, role,
                                                                    own_lo, own_hi);
    tile_store<TH, NW, INTERIOR>(c, b, S ^ 1, K, x0, y0, T, own_lo, own_hi);
    return dsum;
}

// The fused step kernel: 64 x 32 tile, 4 waves, up to K inner iterations per launch.
//   PK = true : the packed-math tile function on the trapezoid row layout (the tuned default, impl 0), MATH as above;
//               LK = true: its lean form (tvl1_tile.h: DPP lane neighbours, loop constants in LDS), 128 VGPRs = 4 waves
//               per SIMD (k_tvl1_step_fused<true, MATH>, the default); LK = false: lane neighbours through LDS planes,
//               constants in registers, 168 VGPRs = 3 waves per SIMD (rounds 2-6: k_tvl1_step_fused_nbr_lds<MATH>,
//               dfx_params.variant & DFX_VAR_TVL1_STEP_NBR_LDS; the same bits);
//   PK = false: the round-1 scalar tile function, kept as a cross-check (impl 2).
#ifndef DFX_FT_TH // tile height / waves / waves per SIMD of the step kernel (A/B builds: scripts/build_variant.sh)
#define DFX_FT_TH 32
#define DFX_FT_NW 4
#define DFX_FT_WGS 3
#endif
#ifndef DFX_FT_WGS_LK // waves per SIMD of the lean form
#define DFX_FT_WGS_LK 4
#endif
constexpr int FT_TH = DFX_FT_TH, FT_NW = DFX_FT_NW;

template <bool PK, int MATH, bool LK>
__device__ __forceinline__ void step_fused(const Tvl1LevelCtx &c, int step_id, int tiles_x, int tiles_y) {
    constexpr int TW = 64, TH = FT_TH, NW = FT_NW;
    // lean: KC_PLANES float2 planes of TH/2 rows (= as many float planes of TH rows) + B_PLANES boundary planes
    constexpr int LDS_FLOATS = !PK ? L_PLANES * TH * TW : LK ? (KC_PLANES * TH + B_PLANES * 2 * NW) * TW
                                                             : (Q_PLANES * TH + 4 * NW) * TW;
    constexpr int LDS_PLANES = !PK ? 0 : LK ? KC_PLANES : Q_PLANES; // float planes of TH rows in front of bnd
    __shared__ __attribute__((aligned(16))) float lds_raw[LDS_FLOATS];
    float (*lds)[TH][TW] = reinterpret_cast<float (*)[TH][TW]>(lds_raw);
    float (*bnd2)[2 * NW][TW] = reinterpret_cast<float (*)[2 * NW][TW]>(lds_raw + LDS_PLANES * TH * TW);
    __shared__ double lds_red[8];
    __shared__ int lds_flag;

    const int b = blockIdx.z;
    Tvl1State *st = c.state + b;
    const int phase = st->phase;
    if (phase == TVL1_PH_LEVEL_DONE)
        return;

    const int K = c.loop.fuse_k;
    const unsigned nblk = gridDim.x; // = tiles of a step of this geometry (tvl1_step_grid)

    if (phase == TVL1_PH_WARP) {
        // k_tvl1_warp handles (or, with zero iterations, has just handled) this pair's warps; the lean form runs only then
        // (tvl1_launch_step), so that the in-kernel warp's registers do not count against its 128
        if (c.split_warp || LK)
            return;
        // in-kernel warp phase (scalar tile function, zero-iteration runs, the WARP_IN_STEP cross-check): classic tiling
        const int tile = dfx_xcd_tile_index((int)blockIdx.x, (int)nblk);
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const Tvl1LevelCtx &cw = dfx_kernarg_ctx(); // (a path the default configuration never takes)
        tile_warp<TH, NW, !PK>(cw, b, st->cur, K, tx * (TW - 2 * K) - K, ty * (TH - 2 * K) - K);
        end_warp_tile(cw, b, st, nblk, step_id, &lds_flag);
        return;
    }

    // ---- phase ITER
    const Tvl1StepPlan plan = tvl1_plan_step(*st, c.loop, step_id);
    if (plan.n_iters <= 0)
        return;
    // Tile of this workgroup (XCD-aware bijective remap: dispatch places workgroup id on XCD id % 8; speed only).
    // c.geom = 1: tile columns start at x = 0 (tvl1_ctrl.h) — the first tile owns its left halo columns, the last one
    // everything up to the right border; every pixel is still owned by exactly one tile and recomputed values are the
    // owner's bits, so the flows do not depend on the geometry (tests/test_tvl1_gpu.py runs both).
    const Tvl1StepGeom g = tvl1_step_geom(c.w, c.h, TW, TH, K, PK ? c.geom : 0);
    const Tvl1TilePlace tp = tvl1_tile_place(g, TW, TH, dfx_xcd_tile_index((int)blockIdx.x, (int)nblk));
    const int xs = tp.x0, ys = tp.y0;
    const bool interior = xs >= 1 && ys >= 1 && xs + TW + 1 <= c.w && ys + TH + 1 <= c.h;
    double dsum;
    if (PK) {
        if (interior)
            dsum = fused_tile_iterate_trap<TH, NW, true, MATH, LK>(c, b, lds, bnd2, plan.src, plan.n_iters,
                                                                   plan.do_check != 0, K, xs, ys, false, false);
        else
            dsum = fused_tile_iterate_trap<TH, NW, false, MATH, LK>(c, b, lds, bnd2, plan.src, plan.n_iters,
                                                                    plan.do_check != 0, K, xs, ys, tp.own_lo != 0,
                                                                    tp.own_hi != 0);
    } else {
        (void)bnd2;
        if (interior)
            dsum = fused_tile_iterate<TH, NW, true>(c, b, lds, plan.src, plan.n_iters, plan.do_check != 0, K, xs, ys);
        else
            dsum = fused_tile_iterate<TH, NW, false>(c, b, lds, plan.src, plan.n_iters, plan.do_check != 0, K, xs, ys);
    }
    end_iter_tile(c, b, st, plan, nblk, (int)blockIdx.x, step_id, dsum, lds_red, &lds_flag);
}

template <bool PK, int MATH>
__global__ __launch_bounds__(64 * FT_NW, PK ? DFX_FT_WGS_LK : DFX_FT_WGS) void k_tvl1_step_fused(Tvl1LevelCtx c, int step_id,
                                                                                          int tiles_x, int tiles_y) {
    step_fused<PK, MATH, PK>(c, step_id, tiles_x, tiles_y);
}

template <int MATH>
__global__ __launch_bounds__(64 * FT_NW, DFX_FT_WGS) void k_tvl1_step_fused_nbr_lds(Tvl1LevelCtx c, int step_id,
                                                                                   int tiles_x, int tiles_y) {
    step_fused<true, MATH, false>(c, step_id, tiles_x, tiles_y);
}

// ------------------------------------------------------------------------------------------------
// The illumination channel (dfx_params.tvl1_gamma != 0; SURVEY.md Appendix A "with gamma", rated MED): a third unknown u3
// with its dual (p31, p32) in planes PL_U3_* / PL_P31_* / PL_P32_* behind the 16 of the default slot (dfx_device.h).  The
// backward warp does not read u3 (A.5 unchanged), the convergence sum does not contain it and merge does not output it, so
// those kernels, the state machine and the ticket reduction are the default path's.  What follows is what differs:
// level begin (p31 = p32 = 0, u3 = 0 at the coarsest level), the upsample of u3 (factor 1) and the fused tile step (impl 0,
// tvl1_gamma_tile.h); the simple step (impl 1) is k_tvl1_step_simple<3> above.  Exact arithmetic with the default hypot
// reading only.

#include "tvl1_gamma_tile.h"

// p31 = p32 = 0 once per level, u3 = 0 at the coarsest level; launched behind k_tvl1_level_begin, reads state.cur.
__global__ __launch_bounds__(256) void k_tvl1_zero_planes_gamma(Tvl1LevelCtx c, int first_level) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= c.pitch || y >= c.h)
        return;
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    const long long o = (long long)y * c.pitch + x;
    pair_plane(c, b, PL_P31_0 + 2 * cur)[o] = 0.0f;
    pair_plane(c, b, PL_P32_0 + 2 * cur)[o] = 0.0f;
    if (first_level)
        pair_plane(c, b, PL_U3_0 + cur)[o] = 0.0f;
}

// u3(level s-1) = resize(u3(level s), dsize): k_tvl1_upsample_u's resize without the 1/scaleStep factor.
__global__ __launch_bounds__(256) void k_tvl1_upsample_u3(Tvl1LevelCtx c, int dw, int dh, int dpitch, float ifx, float ify) {
    const DfxBlockXY blk = dfx_block_xy();
    const int x = blk.x * 64 + (threadIdx.x & 63);
    const int y = blk.y * 4 + (threadIdx.x >> 6);
    if (x >= dw || y >= dh)
        return;
    const int b = blockIdx.z;
    const int cur = c.state[b].cur;
    pair_plane(c, b, PL_U3_0 + (cur ^ 1))[(long long)y * dpitch + x] =
        resize_linear_px(pair_plane(c, b, PL_U3_0 + cur), c.w, c.h, c.pitch, x, y, ifx, ify);
}

template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ double fused_tile_iterate_gamma(const Tvl1LevelCtx &c, int b, f2 (*kc)[TH / 2][64],
                                                           float (*bnd)[2 * NW][64], int S, int n_iters, bool do_check,
                                                           int K, int x0, int y0, bool own_lo, bool own_hi) {
    float pf[GPF_PLANES][TH / NW / 2][2];
    GammaTileState<TH / NW / 2> T;
    const int role = RowMap<TH, NW>::who();
    gamma_tile_issue_loads<TH, NW, INTERIOR>(c, b, S, x0, y0, pf);
    gamma_tile_consume<TH, NW, INTERIOR>(c, x0, y0, pf, T, kc, bnd);
    __syncthreads();
    double dsum;
    if (role * (TH / NW / 2) < K) // only roles that hold halo rows carry the per-float2 skip tests
        dsum = gamma_tile_iterate<TH, NW, INTERIOR, true>(c, T, kc, bnd, n_iters, do_check, K, x0, y0, role, own_lo, own_hi);
    else
        dsum = gamma_tile_iterate<TH, NW, INTERIOR, false>(c, T, kc, bnd, n_iters, do_check, K, x0, y0, role, own_lo, own_hi);
    gamma_tile_store<TH, NW, INTERIOR>(c, b, S ^ 1, K, x0, y0, T, own_lo, own_hi);
    return dsum;
}

// The fused step kernel with the third channel (impl 0): k_tvl1_step_fused's tiles, halo rule, geometry and ticket
// reduction (end_iter_tile), up to K inner iterations per launch, three waves per SIMD.  The dedicated warp kernel runs in
// front of every launch (the engine routes gamma handles that way), so phase WARP has nothing to do here.
__global__ __launch_bounds__(64 * FT_NW, DFX_FT_WGS) void k_tvl1_step_fused_gamma(Tvl1LevelCtx c, int step_id) {
    constexpr int TW = 64, TH = FT_TH, NW = FT_NW;
    __shared__ __attribute__((aligned(16))) f2 kc[KC_PLANES][TH / 2][TW];
    __shared__ float bnd[GB_PLANES][2 * NW][TW];
    __shared__ double lds_red[8];
    __shared__ int lds_flag;

    const int b = blockIdx.z;
    Tvl1State *st = c.state + b;
    if (st->phase != TVL1_PH_ITER)
        return;
    const int K = c.loop.fuse_k;
    const unsigned nblk = gridDim.x; // = tiles of a step of this geometry (tvl1_step_grid)
    const Tvl1StepPlan plan = tvl1_plan_step(*st, c.loop, step_id);
    if (plan.n_iters <= 0)
        return;
    const Tvl1StepGeom g = tvl1_step_geom(c.w, c.h, TW, TH, K, c.geom);
    const Tvl1TilePlace tp = tvl1_tile_place(g, TW, TH, dfx_xcd_tile_index((int)blockIdx.x, (int)nblk));
    const int xs = tp.x0, ys = tp.y0;
    const bool interior = xs >= 1 && ys >= 1 && xs + TW + 1 <= c.w && ys + TH + 1 <= c.h;
    double dsum;
    if (interior)
        dsum = fused_tile_iterate_gamma<TH, NW, true>(c, b, kc, bnd, plan.src, plan.n_iters, plan.do_check != 0, K, xs, ys,
                                                      false, false);
    else
        dsum = fused_tile_iterate_gamma<TH, NW, false>(c, b, kc, bnd, plan.src, plan.n_iters, plan.do_check != 0, K, xs, ys,
                                                       tp.own_lo != 0, tp.own_hi != 0);
    end_iter_tile(c, b, st, plan, nblk, (int)blockIdx.x, step_id, dsum, lds_red, &lds_flag);
}

// ------------------------------------------------------------------------------------------------
// host-callable launchers (the only symbols the control code uses)

static inline dim3 grid_for(int w, int h, int z) { return dim3((w + 63) / 64, (h + 3) / 4, z); }

void tvl1_launch_u8_to_f32(hipStream_t s, const unsigned char *src, long long src_frame_stride, long long src_pitch,
                           const int *frame_slots, int n_frames, float *dst, long long dst_frame_stride, int w, int h,
                           int pitch) {
    hipLaunchKernelGGL(k_u8_to_f32, grid_for(w, h, n_frames), dim3(256), 0, s, src, src_frame_stride, src_pitch,
                       frame_slots, dst, dst_frame_stride, w, h, pitch);
}

void tvl1_launch_pyr_down(hipStream_t s, float *frame_I, long long frame_stride, const int *frame_slots, int n_frames,
                          long long src_off, int sw, int sh, int spitch, long long dst_off, int dw, int dh, int dpitch,
                          float ifx, float ify) {
    hipLaunchKernelGGL(k_pyr_down, grid_for(dw, dh, n_frames), dim3(256), 0, s, frame_I, frame_stride, frame_slots,
                       src_off, sw, sh, spitch, dst_off, dw, dh, dpitch, ifx, ify);
}

void tvl1_launch_centered_gradient(hipStream_t s, const float *frame_I, float *frame_Ix, float *frame_Iy,
                                   long long frame_stride, const int *frame_slots, int n_frames, long long off, int w,
                                   int h, int pitch) {
    hipLaunchKernelGGL(k_centered_gradient, grid_for(w, h, n_frames), dim3(256), 0, s, frame_I, frame_Ix, frame_Iy,
                       frame_stride, frame_slots, off, w, h, pitch);
}

void tvl1_launch_level_begin(hipStream_t s, const Tvl1LevelCtx &c, int first_level) {
    hipLaunchKernelGGL(k_tvl1_level_begin, dim3((c.n_pairs + 63) / 64), dim3(64), 0, s, c, first_level);
    if (!c.head || first_level) // with the warp-and-head kernel only u = 0 at the coarsest level is left to do
        hipLaunchKernelGGL(k_tvl1_zero_planes, grid_for(c.pitch, c.h, c.n_pairs), dim3(256), 0, s, c, first_level);
}

// The coarsest level behind a seed chain (tvl1_seed_kernels.hip), which ends in plane set 0: cur = 0 as at any first level,
// u stays what the chain wrote, and only p is zeroed (first_level = 0 for k_tvl1_zero_planes; nothing with c.head).
// The chain writes columns x < w only: the u planes' padding columns (w <= x < pitch) hold what earlier launches left there,
// as they do at every finer level behind k_tvl1_upsample_u — unlike the unseeded first level, where k_tvl1_zero_planes
// clears them.  No kernel reads them as data; nothing may come to rely on zeroed padding at the first level.
void tvl1_launch_level_begin_seeded(hipStream_t s, const Tvl1LevelCtx &c) {
    hipLaunchKernelGGL(k_tvl1_level_begin, dim3((c.n_pairs + 63) / 64), dim3(64), 0, s, c, 1);
    if (!c.head)
        hipLaunchKernelGGL(k_tvl1_zero_planes, grid_for(c.pitch, c.h, c.n_pairs), dim3(256), 0, s, c, 0);
}

int tvl1_fused_max_k() { return FT_TH / 2 - 4; } // owned region stays >= 8 rows tall
extern "C" int dfxi_tvl1_fused_max_k() { return tvl1_fused_max_k(); } // test hook, not part of the ABI: the tests sweep up to it

// impl: 0 = packed tile function (math = dfx_params.tvl1_math; the scalar forms take the hypot reading from c.k.hyp), 1 = simple one-pixel-per-thread kernel, 2 = scalar tile
// function.  nbr_lds: impl 0 in its register form (DFX_VAR_TVL1_STEP_NBR_LDS).  The grid of the fused kernels is the step's
// tile count (tvl1_step_blocks).
void tvl1_launch_step(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int impl, int math, bool nbr_lds) {
    if (impl == 1) {
        hipLaunchKernelGGL(k_tvl1_step_simple<2>, grid_for(c.w, c.h, c.n_pairs), dim3(256), 0, s, c, step_id);
        return;
    }
    const int K = c.loop.fuse_k;
    const Tvl1StepGeom g = tvl1_step_geom(c.w, c.h, 64, FT_TH, K, 0); // classic counts: the in-kernel warp phase
    const dim3 grid(tvl1_step_blocks(c, impl), 1, c.n_pairs), block(64 * FT_NW);
    if (impl == 0 && (nbr_lds || !c.split_warp)) // the lean form has no in-kernel warp phase
        tvl1_with_math(math, [&](auto m) {
            hipLaunchKernelGGL((k_tvl1_step_fused_nbr_lds<decltype(m)::value>), grid, block, 0, s, c, step_id, g.ntx, g.nty);
        });
    else if (impl == 2)
        hipLaunchKernelGGL((k_tvl1_step_fused<false, 0>), grid, block, 0, s, c, step_id, g.ntx, g.nty);
    else
        tvl1_with_math(math, [&](auto m) {
            hipLaunchKernelGGL((k_tvl1_step_fused<true, decltype(m)::value>), grid, block, 0, s, c, step_id, g.ntx, g.nty);
        });
}

int tvl1_step_blocks(const Tvl1LevelCtx &c, int impl) {
    if (impl == 1) {
        const dim3 g = grid_for(c.w, c.h, 1);
        return (int)(g.x * g.y);
    }
    return tvl1_step_grid(c.w, c.h, 64, FT_TH, c.loop.fuse_k, impl == 0 ? c.geom : 0, c.split_warp);
}

void tvl1_launch_upsample_u(hipStream_t s, const Tvl1LevelCtx &c_src, int dw, int dh, int dpitch, float ifx, float ify,
                            float up) {
    hipLaunchKernelGGL(k_tvl1_upsample_u, grid_for(dw, dh, c_src.n_pairs), dim3(256), 0, s, c_src, dw, dh, dpitch,
                       ifx, ify, up);
}

void tvl1_launch_merge(hipStream_t s, const Tvl1LevelCtx &c0, float *out, long long out_stride) {
    hipLaunchKernelGGL(k_tvl1_merge, grid_for(c0.w, c0.h, c0.n_pairs), dim3(256), 0, s, c0, out, out_stride);
}

void tvl1_launch_merge_planar(hipStream_t s, const Tvl1LevelCtx &c0, const DfxPlanarOut &o) {
    hipLaunchKernelGGL(k_tvl1_merge_planar, dfx_planar_merge_grid(c0.w, c0.h, c0.n_pairs), dim3(256), 0, s, c0, o);
}

// ---- the illumination channel (tvl1_gamma != 0)
static inline void require_gamma_slot(const Tvl1LevelCtx &c) { // planes 16 .. 21 exist only in a 22-plane slot
    if (c.n_planes != PL_COUNT_GAMMA) {
        fprintf(stderr, "dfx: a tvl1_gamma kernel was launched on a pair slot of %d planes\n", c.n_planes);
        abort();
    }
}

void tvl1_launch_level_begin_gamma(hipStream_t s, const Tvl1LevelCtx &c, int first_level) {
    require_gamma_slot(c);
    hipLaunchKernelGGL(k_tvl1_zero_planes_gamma, grid_for(c.pitch, c.h, c.n_pairs), dim3(256), 0, s, c, first_level);
}

// impl 0: the fused tile kernel (behind tvl1_launch_warp of the same step id), 1: the simple kernel
void tvl1_launch_step_gamma(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int impl) {
    require_gamma_slot(c);
    if (impl == 1)
        hipLaunchKernelGGL(k_tvl1_step_simple<3>, grid_for(c.w, c.h, c.n_pairs), dim3(256), 0, s, c, step_id);
    else
        hipLaunchKernelGGL(k_tvl1_step_fused_gamma, dim3(tvl1_step_blocks(c, 0), 1, c.n_pairs), dim3(64 * FT_NW), 0, s, c,
                           step_id);
}

void tvl1_launch_upsample_u3(hipStream_t s, const Tvl1LevelCtx &c_src, int dw, int dh, int dpitch, float ifx, float ify) {
    require_gamma_slot(c_src);
    hipLaunchKernelGGL(k_tvl1_upsample_u3, grid_for(dw, dh, c_src.n_pairs), dim3(256), 0, s, c_src, dw, dh, dpitch, ifx, ify);
}
