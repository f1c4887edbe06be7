// tvl1_head_kernels.hip — the backward warp of the -a=tvl1 hot path fused with the head of the inner loop it starts
// (round 6; upstream: warpBackwardKernel + the first two estimateUKernel / estimateDualVariablesKernel rounds of
// cv::cuda::OpticalFlowDual_TVL1, reference call site src/denseflow_gpu.cpp:327).
//
// Why: on converging content a pair spends 25 warps per pyramid, and 20 of them (warps 1-4 of every level) consist of the
// warp and ONE two-iteration step — the first convergence check is due at iteration 1 and passes.  As two launches that
// costs, per pixel, the warp's 3 + 3 plane reads and 3 plane writes plus the step's 9 reads (x 1.5 with its 4-pixel halo)
// and 6 writes, in kernels that run at 4.4-4.9 TB/s of their own bytes.  Here one workgroup
//   1. copies the (64 + 16) x (32 + 10) neighbourhood of I1, I1x, I1y of its 64 x 32 tile into LDS (aligned 16-byte row
//      loads, clamp-to-edge applied while copying — the tile of k_tvl1_warp_lds grown to the step kernel's tile),
//   2. warps the tile's 8 rows per thread from it, two pixels at a time as packed float2 math — I1wx, I1wy, rho_c land in the registers the iterations read them from,
//      the same pixel taking the same bits whichever tile (owner or halo) computes it: warp_finish on the same taps,
//   3. re-uses the LDS for the iteration's neighbour planes and runs the head of the loop (TVL1_HEAD_ITERS = 2 iterations,
//      2-pixel halo: a tile owns 60 x 28 of its 64 x 32 pixels) with the packed tile function of the step kernel, in
//      its lean form (tvl1_tile.h) — same functions, same operation order, bit-identical,
//   4. stores u / p of the owned region into the other ping-pong set AND I1wx / I1wy / rho_c (a loop that goes on reads
//      them in the step kernel), publishes its share of the convergence sum; the last workgroup of the pair advances the
//      state machine (tvl1_ctrl.h: tvl1_plan_head / tvl1_end_head).
// Per owned pixel: 14.5 words read (7 planes x 1.22 + the image tiles' 6.0; 9.7 for a level's first warp, whose dual planes
// are zero by definition and are not read) + 9 written, against 31.3 for the two launches.  The kernel issues VALU
// instructions 2/3 to 3/4 of the time (SQ counters, profiles/round6/, profiles/head_lean/): forming I1x / I1y in LDS from a
// wider I1 tile instead of reading them (16 KB instead of 42 KB per tile) was measured SLOWER for that reason, as were
// hand-scheduled tap loads (LABNOTES.md section 11).
// Occupancy: the kernel fits 128 VGPRs and 40 KB of LDS, so four workgroups share a CU (4 waves per SIMD) and cover each
// other's load latency.  What that took: the iterations on the lean tile function, I0 loaded row by row, rows addressed
// through the scalar offset, the `far` gather as ONE copy that holds one window row, an image tile of 42 rows (vertical
// margin 3: flows in (-4, 4] are served from LDS; 15 of 10^9 pixels of the hard 1080p clip go `far`, 4 with 44 rows).
// The round-6 form (3 waves per SIMD) is kept as k_tvl1_warp_head_regs (DFX_VAR_TVL1_HEAD_NBR_LDS).
// Compiled with -ffp-contract=off (see tvl1_math.h).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dfx_device.h"
#include "tvl1_device_common.h"
#include "tvl1_kernels.h"
#include "tvl1_tile.h"

#ifndef DFX_HEAD_P_EARLY
#define DFX_HEAD_P_EARLY 0 // the dual planes' loads issued in front of the warp (A/B builds: scripts/build_variant.sh)
#endif
#ifndef DFX_HEAD_HX // the lean form's image-tile halo (A/B builds)
#define DFX_HEAD_HX 8
#define DFX_HEAD_HY 5
#endif
#ifndef DFX_HEAD_FAR_COUNT
#define DFX_HEAD_FAR_COUNT 0 // measurement builds only: count the pixels that take the `far` path (dfxi_head_far_counts)
#endif
#if DFX_HEAD_FAR_COUNT
__device__ unsigned long long dfx_head_far_px[2]; // pixels redone by the global gather, pixels warped
#endif

namespace {

constexpr int HD_TW = 64, HD_TH = 32, HD_NW = 4, HD_K = TVL1_HEAD_ITERS;
// Addressing of the kernel's own plane loads and stores: a wave's 8 rows are wave-uniform (RowMap: the role is), so a
// row's byte offset rides in the buffer instruction's scalar offset next to the plane's and ONE vector offset — the
// column's — serves all rows and planes, where 8 per-row vector offsets lived from the first load to the last store.
// Rows and columns outside the image read row 0 / column 0 (masked afterwards, as before).
__device__ __forceinline__ int head_role() { return __builtin_amdgcn_readfirstlane(RowMap<HD_TH, HD_NW>::who()); }
template <bool INTERIOR> __device__ __forceinline__ unsigned head_row_soff(const Tvl1LevelCtx &c, int y) {
    return INTERIOR || (y >= 0 && y < c.h) ? 4u * (unsigned)(y * c.pitch) : 0u;
}
template <bool INTERIOR> __device__ __forceinline__ unsigned head_col_voff(const Tvl1LevelCtx &c, int x) {
    return INTERIOR || (x >= 0 && x < c.w) ? 4u * (unsigned)x : 0u;
}

// Image tile: HX columns left and right of the 64 x 32 tile, HY rows above and below.  A pixel's 4 x 4 window starts at
// ceil(flow - 2), so a halo of H serves flows in (1 - H, H - 1]; the others take the `far` path.  HX is a multiple of 4:
// tile columns start at multiples of 60, so the 16-byte row loads stay aligned.
template <int HX_, int HY_> struct ImgTile {
    static constexpr int HX = HX_, HY = HY_, TWL = HD_TW + 2 * HX, THL = HD_TH + 2 * HY;
    static constexpr int FLOATS = 3 * THL * TWL;
    static_assert(HX % 4 == 0 && HX >= 4 && HY >= 2, "aligned row loads; the window of a zero flow must fit");
};
using ImgRegs = ImgTile<8, 6>;                     // the register form (rounds 6 on): 80 x 44, 42 240 B, 3 workgroups per CU
using ImgLean = ImgTile<DFX_HEAD_HX, DFX_HEAD_HY>; // the lean form: 80 x 42, 40 320 B (DFX_HEAD_HX 4, HY 6: 72 x 44, 38 016 B)
constexpr int HD_LDS_ITER = (Q_PLANES * HD_TH + 4 * HD_NW) * HD_TW;              // floats: 9 216 (36 864 B)
constexpr int HD_LDS_ITER_LEAN = (KC_PLANES * HD_TH + B_PLANES * 2 * HD_NW) * HD_TW; // floats: 8 192 (32 768 B)
static_assert(HD_LDS_ITER <= ImgRegs::FLOATS && HD_LDS_ITER_LEAN <= ImgLean::FLOATS,
              "the iteration planes re-use the image tile's LDS");
static_assert((HD_TW - 2 * HD_K) % 4 == 0, "tile columns must start 16-byte aligned");
// four workgroups of the lean form in a CU's 160 KB: the image tile, lds_red (8 doubles) and lds_flag
static_assert(4 * ImgLean::FLOATS + 8 * 8 + 4 <= 40 * 1024, "the lean form's LDS budget: 40 KB per workgroup");

// One pixel by the global gather (the `far` path), one window row at a time: warp_fetch's clamped addresses and
// warp_finish's sequence of rounded operations — the sums run over the window's rows, then its columns, as there — with 12
// taps in flight where warp_backward_px_v holds 48 (the scheduling barrier keeps the rows' loads apart; the rows as a
// loop that is not unrolled would leave an unused 68-byte stack slot behind in this compiler).
__device__ __forceinline__ WarpOut head_far_px(const float *I1, const float *I1x, const float *I1y, int w, int h, int pitch,
                                               int x, int y, float u1v, float u2v, float I0v) {
    const float wx = (float)x + u1v, wy = (float)y + u2v;
    const float fx0 = ceilf(wx - 2.0f), fy0 = ceilf(wy - 2.0f);
    const int xmin = (int)fminf(fmaxf(fx0, -4.0f), (float)w + 4.0f); // clamped first: NaN / Inf flows index nothing
    const int ymin = (int)fminf(fmaxf(fy0, -4.0f), (float)h + 4.0f);
    float cwx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        cwx[j] = tvl1_bicubic_coeff(wx - (fx0 + (float)j));
    float sum = 0.0f, sumx = 0.0f, sumy = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int jy = 0; jy < 4; ++jy) {
        __builtin_amdgcn_sched_barrier(0);
        const float cwy = tvl1_bicubic_coeff(wy - (fy0 + (float)jy));
        const long long ro = (long long)min(max(ymin + jy, 0), h - 1) * pitch; // clamp-to-edge point sampling
        float t1[4], tx[4], ty[4];
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const long long r = ro + min(max(xmin + jx, 0), w - 1);
            t1[jx] = I1[r];
            tx[jx] = I1x[r];
            ty[jx] = I1y[r];
        }
#pragma unroll
        for (int jx = 0; jx < 4; ++jx) {
            const float wgt = cwx[jx] * cwy;
            sum = sum + wgt * t1[jx];
            sumx = sumx + wgt * tx[jx];
            sumy = sumy + wgt * ty[jx];
            wsum = wsum + wgt;
        }
    }
    const float coeff = 1.0f / wsum;
    const float I1w = sum * coeff;
    WarpOut o;
    o.I1wx = sumx * coeff;
    o.I1wy = sumy * coeff;
    o.grad = o.I1wx * o.I1wx + o.I1wy * o.I1wy;
    o.rho_c = ((I1w - o.I1wx * u1v) - o.I1wy * u2v) - I0v;
    return o;
}

// Steps 1 + 2 for one thread: the warp of its HP float2 rows into pf[0..2] (I1wx, I1wy, rho_c), u1 / u2 into pf[3..4].
template <bool INTERIOR, class G>
__device__ __forceinline__ void head_warp(const Tvl1LevelCtx &c, int b, int cur, int x0, int y0,
                                          float *tile, float (&pf)[PF_PLANES][HD_TH / HD_NW / 2][2]) {
    constexpr int HP = HD_TH / HD_NW / 2;
    constexpr int HD_HX = G::HX, HD_HY = G::HY, HD_TWL = G::TWL, HD_THL = G::THL;
    using RM = RowMap<HD_TH, HD_NW>;
    const int lane = threadIdx.x & 63, role = head_role();
    const int x = x0 + lane;
    const bool col_in = INTERIOR || (x >= 0 && x < c.w);
    const unsigned vo = head_col_voff<INTERIOR>(c, x);
    const PairDesc pd = c.pairs[b];
    const float *I0 = c.frame_I + (long long)pd.frame_a * c.frame_stride + c.lvl_off;
    const long long fb = (long long)pd.frame_b * c.frame_stride + c.lvl_off;
    const float *P1 = c.frame_I + fb, *P1x = c.frame_Ix + fb, *P1y = c.frame_Iy + fb;
    // (buffer addressing, tvl1_device_common.h: the pair's slot, and a descriptor on this level's plane of frame a)
    const dfx_rsrc rs = pair_rsrc(c, b), r0 = dfx_make_rsrc(I0, 4u * (unsigned)(c.pitch * c.h));
    const unsigned s_u1 = plane_soff(c, PL_U1_0 + 2 * cur), s_u2 = plane_soff(c, PL_U2_0 + 2 * cur);
    // (I0 is loaded row by row below: what stays live across a row's 16 taps is that row's working set, u — the
    // iterations' u — and the finished rows' outputs)
#pragma unroll
    for (int j = 0; j < HP; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned ro = head_row_soff<INTERIOR>(c, y0 + RM::row(role, j, e));
            pf[3][j][e] = buf_ld(rs, vo, s_u1 + ro);
            pf[4][j][e] = buf_ld(rs, vo, s_u2 + ro);
        }
    const int tx0 = x0 - HD_HX, ty0 = y0 - HD_HY;
    // LDS image tile: (I1, I1x) of a pixel side by side — a tap of the bicubic sums is one ds_read_b64 for both (2 LDS cycles per
    // wave instead of 4: the warp phase keeps the LDS nearly as busy as the vector ALU) — and I1y as a plane of its own
    f2 *t1x = reinterpret_cast<f2 *>(tile);
    float *tgy = tile + 2 * HD_THL * HD_TWL;
    // image tiles: float4 q of tile row r covers image columns tx0 + 4q .. + 3 of row clamp(ty0 + r); clamp-to-edge is
    // applied here, so a tile entry IS the point-sampled texture value (k_tvl1_warp_lds has the same copy loop): a float4
    // left of the image is column 0 four times, one right of it column w - 1, one that straddles the right border is patched
    // per element (the row pitch is a multiple of 64 floats >= w, so the aligned 16-byte load never leaves the row).
    constexpr int Q = HD_TWL / 4;
    for (int i = threadIdx.x; i < HD_THL * Q; i += 64 * HD_NW) {
        const int r = i / Q, q = i - r * Q;
        const long long ro = (long long)min(max(ty0 + r, 0), c.h - 1) * c.pitch;
        const int gx = tx0 + 4 * q;
        const int lx4 = min(max(gx, 0), ((c.w - 1) >> 2) << 2); // aligned, inside the row
        // (plain pointers: this compiler's __builtin_amdgcn_raw_buffer_load_b128 emits a ONE-dword load and splats it)
        const float4 a = *reinterpret_cast<const float4 *>(P1 + ro + lx4);
        const float4 bq = *reinterpret_cast<const float4 *>(P1x + ro + lx4);
        const float4 cq = *reinterpret_cast<const float4 *>(P1y + ro + lx4);
        const int o = r * HD_TWL + 4 * q;
        if (gx >= 0 && gx + 3 <= c.w - 1) { // (the image tile is wider than the iteration tile INTERIOR speaks about)
            *reinterpret_cast<float4 *>(&t1x[o]) = make_float4(a.x, bq.x, a.y, bq.y);
            *reinterpret_cast<float4 *>(&t1x[o + 2]) = make_float4(a.z, bq.z, a.w, bq.w);
            *reinterpret_cast<float4 *>(&tgy[o]) = cq;
            continue;
        }
        const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {bq.x, bq.y, bq.z, bq.w}, cv[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = min(max(gx + e, 0), c.w - 1) - lx4; // 0..3: the element of the loaded float4 column gx + e clamps to
            t1x[o + e] = pk_set(k == 0 ? av[0] : k == 1 ? av[1] : k == 2 ? av[2] : av[3],
                                k == 0 ? bv[0] : k == 1 ? bv[1] : k == 2 ? bv[2] : bv[3]);
            tgy[o + e] = k == 0 ? cv[0] : k == 1 ? cv[1] : k == 2 ? cv[2] : cv[3];
        }
    }
    __syncthreads();
    // Two pixels at a time — the rows of float2 j — with the 16 x 3 multiply-adds of the bicubic sums as packed
    // operations: each half performs warp_finish's very sequence of rounded operations (packed f32 operations round
    // each half on its own, nothing is contracted), the final 1 / wsum and the rho_c chain run per half in scalar form.
    // A pixel whose 4 x 4 window leaves the LDS tile (|flow| beyond the margin: occlusion borders, large motion) is
    // noted in `far` and redone with the global gather afterwards (rare; kept out of this loop's register budget).
    unsigned far = 0u;
    const float xf = (float)x;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const int ya = y0 + RM::row(role, j, 0), yb = y0 + RM::row(role, j, 1);
        const bool ina = INTERIOR || (col_in && ya >= 0 && ya < c.h), inb = INTERIOR || (col_in && yb >= 0 && yb < c.h);
        const float i0a = buf_ld(r0, vo, head_row_soff<INTERIOR>(c, ya)); // in flight during the taps
        const float i0b = buf_ld(r0, vo, head_row_soff<INTERIOR>(c, yb));
        const f2 u1v = pk_set(pf[3][j][0], pf[3][j][1]), u2v = pk_set(pf[4][j][0], pf[4][j][1]);
        const f2 wx = (f2)(xf) + u1v, wy = pk_set((float)ya, (float)yb) + u2v;
        const f2 fx0 = __builtin_elementwise_ceil(wx - 2.0f), fy0 = __builtin_elementwise_ceil(wy - 2.0f);
        // the window's first tap, exactly as warp_fetch derives it (clamped before the int conversion: NaN / Inf flows)
        const int lxa = (int)fminf(fmaxf(fx0.x, -4.0f), (float)c.w + 4.0f) - tx0;
        const int lxb = (int)fminf(fmaxf(fx0.y, -4.0f), (float)c.w + 4.0f) - tx0;
        const int lya = (int)fminf(fmaxf(fy0.x, -4.0f), (float)c.h + 4.0f) - ty0;
        const int lyb = (int)fminf(fmaxf(fy0.y, -4.0f), (float)c.h + 4.0f) - ty0;
        // (0 <= l && l + 3 < N as one unsigned comparison)
        const bool oka = (unsigned)lxa < (unsigned)(HD_TWL - 3) && (unsigned)lya < (unsigned)(HD_THL - 3);
        const bool okb = (unsigned)lxb < (unsigned)(HD_TWL - 3) && (unsigned)lyb < (unsigned)(HD_THL - 3);
        far |= (ina && !oka ? 1u : 0u) << (2 * j);
        far |= (inb && !okb ? 1u : 0u) << (2 * j + 1);
        const int oa = oka ? lya * HD_TWL + lxa : 0, ob = okb ? lyb * HD_TWL + lxb : 0; // (outside the tile: redone below)
        // every weight's arm chosen by the tap's position in the window (pk_bicubic_window: half the instructions of the
        // select chain); a pixel for which that is not the chain's choice (one-ulp coincidences, NaN / infinite flows) is
        // redone below with the scalar chain, like one whose window leaves the tile
        f2 cwx[4], cwy[4];
        bool wxa, wxb, wya, wyb;
        pk_bicubic_window(wx, fx0, cwx, wxa, wxb);
        pk_bicubic_window(wy, fy0, cwy, wya, wyb);
        far |= (ina && !(wxa && wya) ? 1u : 0u) << (2 * j);
        far |= (inb && !(wxb && wyb) ? 1u : 0u) << (2 * j + 1);
        // (I1, I1x) sums per pixel (sa: pixel a, sb: pixel b; the weight enters as one half of wgt, by op_sel), I1y sums and
        // the weight sum for both pixels at once: per value the same products and additions in the same order as before
        f2 sa = (f2)(0.0f), sb = (f2)(0.0f), sumy = (f2)(0.0f), wsum = (f2)(0.0f);
#pragma unroll
        for (int jy = 0; jy < 4; ++jy) {
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const int o = jy * HD_TWL + jx;
                const f2 wgt = cwx[jx] * cwy[jy];
                sa = sa + pk_set(wgt.x, wgt.x) * t1x[oa + o];
                sb = sb + pk_set(wgt.y, wgt.y) * t1x[ob + o];
                sumy = sumy + wgt * pk_set(tgy[oa + o], tgy[ob + o]);
                wsum = wsum + wgt;
            }
        }
        const f2 sum = pk_set(sa.x, sb.x), sumx = pk_set(sa.y, sb.y);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float coeff = 1.0f / (e ? wsum.y : wsum.x);
            const float I1w = (e ? sum.y : sum.x) * coeff;
            const float I1wx = (e ? sumx.y : sumx.x) * coeff, I1wy = (e ? sumy.y : sumy.x) * coeff;
            const float rho_c = ((I1w - I1wx * pf[3][j][e]) - I1wy * pf[4][j][e]) - (e ? i0b : i0a);
            const bool in = e ? inb : ina;
            pf[0][j][e] = in ? I1wx : 0.0f;
            pf[1][j][e] = in ? I1wy : 0.0f;
            pf[2][j][e] = in ? rho_c : 0.0f;
        }
    }
#if DFX_HEAD_FAR_COUNT
    if (far)
        atomicAdd(&dfx_head_far_px[0], (unsigned long long)__builtin_popcount(far));
    if (threadIdx.x == 0)
        atomicAdd(&dfx_head_far_px[1], (unsigned long long)((min(x0 + HD_TW, c.w) - max(x0, 0)) * (min(y0 + HD_TH, c.h) - max(y0, 0))));
#endif
    // One copy of the gather for the thread's 8 pixels, as a loop that is not unrolled: the pixel's inputs and outputs are
    // picked by selects on the wave-uniform k (a register array cannot be indexed): the gather counts once against the
    // register budget, and never against the loop above.
    if (far) {
#pragma unroll 1
        for (int k = 0; k < 2 * HP; ++k) {
            if (!(far & (1u << k)))
                continue;
            float u1v = 0.0f, u2v = 0.0f;
#pragma unroll
            for (int j = 0; j < HP; ++j)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    u1v = k == 2 * j + e ? pf[3][j][e] : u1v;
                    u2v = k == 2 * j + e ? pf[4][j][e] : u2v;
                }
            const int y = y0 + RM::row(role, k >> 1, k & 1);
            const float i0v = buf_ld(r0, vo, head_row_soff<INTERIOR>(c, y));
            // (a rare path: the frame planes and the level's size from the kernel-argument segment, not from scalar
            // registers held across the rows above)
            const Tvl1LevelCtx &ck = dfx_kernarg_ctx();
            const long long fbk = (long long)pd.frame_b * ck.frame_stride + ck.lvl_off;
            const WarpOut r = head_far_px(ck.frame_I + fbk, ck.frame_Ix + fbk, ck.frame_Iy + fbk, ck.w, ck.h, ck.pitch, x, y, u1v, u2v, i0v);
#pragma unroll
            for (int j = 0; j < HP; ++j)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    pf[0][j][e] = k == 2 * j + e ? r.I1wx : pf[0][j][e];
                    pf[1][j][e] = k == 2 * j + e ? r.I1wy : pf[1][j][e];
                    pf[2][j][e] = k == 2 * j + e ? r.rho_c : pf[2][j][e];
                }
        }
    }
}

// the four dual planes of ping-pong set `cur` into pf[5..8]; p_zero (wave-uniform): the level's first warp — p = 0 (A.3),
// nobody has written those planes (k_tvl1_zero_planes leaves them alone when this kernel is in use)
template <bool INTERIOR>
__device__ __forceinline__ void head_load_p(const Tvl1LevelCtx &c, int b, int cur, int x0, int y0, bool p_zero,
                                            float (&pf)[PF_PLANES][HD_TH / HD_NW / 2][2]) {
    constexpr int HP = HD_TH / HD_NW / 2;
    if (p_zero) {
#pragma unroll
        for (int j = 0; j < HP; ++j)
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    pf[5 + q][j][e] = 0.0f;
        return;
    }
    using RM = RowMap<HD_TH, HD_NW>;
    const int lane = threadIdx.x & 63, role = head_role();
    const unsigned vo = head_col_voff<INTERIOR>(c, x0 + lane);
    const dfx_rsrc rs = pair_rsrc(c, b);
    const unsigned so[4] = {plane_soff(c, PL_P11_0 + 4 * cur), plane_soff(c, PL_P12_0 + 4 * cur),
                            plane_soff(c, PL_P21_0 + 4 * cur), plane_soff(c, PL_P22_0 + 4 * cur)};
#pragma unroll
    for (int j = 0; j < HP; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned ro = head_row_soff<INTERIOR>(c, y0 + RM::row(role, j, e));
#pragma unroll
            for (int q = 0; q < 4; ++q)
                pf[5 + q][j][e] = buf_ld(rs, vo, so[q] + ro);
        }
}

// The owned region (tile_store's ownership rule, with this kernel's addressing): u and p into ping-pong set D, and I1wx /
// I1wy / rho_c — a loop that goes on reads them in the step kernel.
// (LEAN: rho_c lies in the tile function's LDS plane kc[KC_RHOC], written by this very thread)
template <bool INTERIOR, bool LEAN>
__device__ __forceinline__ void head_store(const Tvl1LevelCtx &c, int b, int D, int x0, int y0,
                                           const TileState<HD_TH / HD_NW / 2> &T, const float *lds_raw, bool own_lo,
                                           bool own_hi) {
    constexpr int HP = HD_TH / HD_NW / 2, K = HD_K;
    const f2 (*kc)[HD_TH / 2][HD_TW] = reinterpret_cast<const f2 (*)[HD_TH / 2][HD_TW]>(lds_raw);
    using RM = RowMap<HD_TH, HD_NW>;
    const int lx = threadIdx.x & 63, role = head_role();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool col_owned = (lx >= K || own_lo) && (lx < HD_TW - K || own_hi) && col_in;
    const unsigned vo = 4u * (unsigned)gx; // (used by owned columns only)
    const dfx_rsrc rs = pair_rsrc(c, b);
    const unsigned s_wx = plane_soff(c, PL_I1WX), s_wy = plane_soff(c, PL_I1WY), s_rc = plane_soff(c, PL_RHOC);
    const unsigned s_u1 = plane_soff(c, PL_U1_0 + 2 * D), s_u2 = plane_soff(c, PL_U2_0 + 2 * D);
    const unsigned s_p11 = plane_soff(c, PL_P11_0 + 4 * D), s_p12 = plane_soff(c, PL_P12_0 + 4 * D);
    const unsigned s_p21 = plane_soff(c, PL_P21_0 + 4 * D), s_p22 = plane_soff(c, PL_P22_0 + 4 * D);
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        const f2 krc = LEAN ? kc[KC_RHOC][role * HP + j][lx] : T.krc[j];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int ly = RM::row(role, j, e), gy = y0 + ly;
            if (col_owned && ly >= K && ly < HD_TH - K && (INTERIOR || (gy >= 0 && gy < c.h))) {
                const unsigned ro = 4u * (unsigned)(gy * c.pitch);
                buf_st(rs, vo, s_u1 + ro, e ? T.u1[j].y : T.u1[j].x);
                buf_st(rs, vo, s_u2 + ro, e ? T.u2[j].y : T.u2[j].x);
                buf_st(rs, vo, s_p11 + ro, e ? T.p11[j].y : T.p11[j].x);
                buf_st(rs, vo, s_p12 + ro, e ? T.p12[j].y : T.p12[j].x);
                buf_st(rs, vo, s_p21 + ro, e ? T.p21[j].y : T.p21[j].x);
                buf_st(rs, vo, s_p22 + ro, e ? T.p22[j].y : T.p22[j].x);
                buf_st(rs, vo, s_wx + ro, e ? T.kwx[j].y : T.kwx[j].x);
                buf_st(rs, vo, s_wy + ro, e ? T.kwy[j].y : T.kwy[j].x);
                buf_st(rs, vo, s_rc + ro, e ? krc.y : krc.x);
            }
        }
    }
}

// LEAN: the iterations on the lean form of the tile function (tvl1_tile.h: DPP lane neighbours, rho_c / grad / 1/grad in
// LDS).  Its interior form hands lane 0 and lane 63 the value 0 for the neighbour outside the tile; with HD_K = 2
// iterations at most and a 2-pixel halo those lanes lie outside every owned pixel's dependency cone, as in the step
// kernel at K = 4: after n iterations a value is exact up to n columns from the tile's edge, and the owned columns
// start HD_K >= n columns in.
template <bool INTERIOR, int MATH, bool LEAN>
__device__ __forceinline__ double head_tile(const Tvl1LevelCtx &c, int b, float *lds_raw, const Tvl1StepPlan &plan, int x0,
                                            int y0, bool own_lo, bool own_hi, bool p_zero) {
    constexpr int TH = HD_TH, NW = HD_NW, HP = TH / NW / 2;
    float (*lds)[TH][HD_TW] = reinterpret_cast<float (*)[TH][HD_TW]>(lds_raw);
    float (*bnd)[2 * NW][HD_TW] =
        reinterpret_cast<float (*)[2 * NW][HD_TW]>(lds_raw + (LEAN ? (int)KC_PLANES : (int)Q_PLANES) * TH * HD_TW);
    using G = typename std::conditional<LEAN, ImgLean, ImgRegs>::type;
    float pf[PF_PLANES][HP][2];
    TileState<HP> T;
    const int role = RowMap<TH, NW>::who();
#if DFX_HEAD_P_EARLY
    head_load_p<INTERIOR>(c, b, plan.src, x0, y0, p_zero, pf); // in flight while the warp runs
#endif
    head_warp<INTERIOR, G>(c, b, plan.src, x0, y0, lds_raw, pf);
#if !DFX_HEAD_P_EARLY
    head_load_p<INTERIOR>(c, b, plan.src, x0, y0, p_zero, pf);
#endif
    __syncthreads(); // every thread is done with the image tile: its LDS becomes the iteration's neighbour planes
    tile_consume<TH, NW, INTERIOR, MATH, LEAN>(c, x0, y0, pf, T, lds, bnd);
    __syncthreads();
    double dsum;
    if (role * HP < HD_K) // only roles that hold halo rows carry the per-float2 skip tests
        dsum = tile_iterate_trap<TH, NW, INTERIOR, true, MATH, LEAN>(c, T, lds, bnd, plan.n_iters, plan.do_check != 0, HD_K, x0, y0,
                                                               role, own_lo, own_hi);
    else
        dsum = tile_iterate_trap<TH, NW, INTERIOR, false, MATH, LEAN>(c, T, lds, bnd, plan.n_iters, plan.do_check != 0, HD_K, x0,
                                                                y0, role, own_lo, own_hi);
    head_store<INTERIOR, LEAN>(c, b, plan.src ^ 1, x0, y0, T, lds_raw, own_lo, own_hi);
    return dsum;
}

// One workgroup = one 64 x 32 tile of one pair; grid.x = tiles of the head's geometry (tvl1_head_blocks), grid.z = pair.
template <int MATH, bool LEAN>
__device__ __forceinline__ void warp_head(const Tvl1LevelCtx &c, int step_id) {
    __shared__ __attribute__((aligned(16))) float lds_raw[LEAN ? ImgLean::FLOATS : ImgRegs::FLOATS];
    __shared__ double lds_red[8];
    __shared__ int lds_flag;
    const int b = blockIdx.z;
    Tvl1State *st = c.state + b;
    if (st->phase != TVL1_PH_WARP)
        return;
    // every workgroup derives the head's plan from the state as it stands (it changes only once every workgroup of the
    // pair has arrived, below)
    const Tvl1StepPlan plan = tvl1_plan_head(*st, c.loop);
    const bool p_zero = st->warp == 0; // the level's first warp: p = 0 by definition, not by reading zeros
    const unsigned nblk = gridDim.x;
    const Tvl1StepGeom g = tvl1_step_geom(c.w, c.h, HD_TW, HD_TH, HD_K, 1);
    const Tvl1TilePlace tp = tvl1_tile_place(g, HD_TW, HD_TH, dfx_xcd_tile_index((int)blockIdx.x, (int)nblk));
    const int xs = tp.x0, ys = tp.y0;
    const bool interior = xs >= 1 && ys >= 1 && xs + HD_TW + 1 <= c.w && ys + HD_TH + 1 <= c.h;
    double dsum;
    if (interior)
        dsum = head_tile<true, MATH, LEAN>(c, b, lds_raw, plan, xs, ys, false, false, p_zero);
    else
        dsum = head_tile<false, MATH, LEAN>(c, b, lds_raw, plan, xs, ys, tp.own_lo != 0, tp.own_hi != 0, p_zero);

    // the tile's share of sum(diff), the arrival ticket, and — in the pair's last workgroup — the state transition
    end_segment_tile(c, b, st, plan.do_check != 0, nblk, (int)blockIdx.x, step_id, dsum, lds_red, &lds_flag,
                     [&](Tvl1State &s, double err) { tvl1_end_head(s, c.loop, plan, step_id, err); });
}

} // namespace

// The default: the lean form, 128 VGPRs and 40 KB of LDS = 4 workgroups per CU (4 waves per SIMD).
template <int MATH>
__global__ __launch_bounds__(64 * HD_NW, 4) void k_tvl1_warp_head(Tvl1LevelCtx c, int step_id) {
    warp_head<MATH, true>(c, step_id);
}

// The register form of round 6 (dfx_params.variant & DFX_VAR_TVL1_HEAD_NBR_LDS): the iterations' lane neighbours through LDS
// planes, their constants in registers, the 80 x 44 image tile; 3 waves per SIMD.  The same bits.
template <int MATH>
__global__ __launch_bounds__(64 * HD_NW, 3) void k_tvl1_warp_head_regs(Tvl1LevelCtx c, int step_id) {
    warp_head<MATH, false>(c, step_id);
}

#if DFX_HEAD_FAR_COUNT
extern "C" int dfxi_head_far_counts(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(dfx_head_far_px), sizeof(dfx_head_far_px)) != hipSuccess)
        return -1;
    const unsigned long long zero[2] = {0, 0};
    return reset && hipMemcpyToSymbol(HIP_SYMBOL(dfx_head_far_px), zero, sizeof(zero)) != hipSuccess ? -1 : 0;
}
#endif

int tvl1_head_blocks(const Tvl1LevelCtx &c) { return tvl1_step_grid(c.w, c.h, HD_TW, HD_TH, HD_K, 1, 1); }

void tvl1_launch_warp_head(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int math, bool regs) {
    const dim3 grid(tvl1_head_blocks(c), 1, c.n_pairs), block(64 * HD_NW);
    tvl1_with_math(math, [&](auto m) {
        if (regs)
            hipLaunchKernelGGL((k_tvl1_warp_head_regs<decltype(m)::value>), grid, block, 0, s, c, step_id);
        else
            hipLaunchKernelGGL((k_tvl1_warp_head<decltype(m)::value>), grid, block, 0, s, c, step_id);
    });
}
