// tvl1_tile.h — the packed-math tile function of the -a=tvl1 inner loop (device code), shared by the step kernel
// (tvl1_kernels.hip: k_tvl1_step_fused) and the warp-and-head kernel (tvl1_head_kernels.hip: k_tvl1_warp_head).
// Semantics: cv::cuda tvl1flow.cu's estimateUKernel / estimateDualVariablesKernel as restated in SURVEY.md A.6-A.7
// (reference call site src/denseflow_gpu.cpp:327).  Compiled with -ffp-contract=off (see tvl1_math.h).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "dfx_device.h"
#include "tvl1_device_common.h"
#include "tvl1_math.h"
#include "tvl1_math_pk.h"

// ------------------------------------------------------------------------------------------------
// The fused step, packed-math variant (the tuned default).  Same tile, same halo scheme, same bits as
// fused_tile_iterate above, but:
//   * a thread's 8 rows are held as HP = 4 float2 values {row, mirror row}: every float operation of the
//     iteration runs as one v_pk_* instruction for two rows (tvl1_math_pk.h) — the loop is bound by VALU
//     issue, and packed float math doubles the issue rate of 60 % of its instructions;
//   * p12 / p22 are only ever read across a role boundary, so instead of two full LDS planes there are two
//     2*NW-row boundary planes: LDS 48 KB -> 36 KB;
//   * 1/grad (refined, tvl1_refined_rcp) is constant over a warp's iterations and kept in registers.
// LDS planes: p11, p21 (left neighbour), u1, u2 (right neighbour), [TH][64] each; boundary rows of p12 / p22
// and nothing else: [2 * NW][64].
// MATH = dfx_params.tvl1_math.  0: the oracle's arithmetic, bit for bit (the default; hypot as CUDA's libdevice
// evaluates it, tvl1_math.h).  2 / 3: the same exact arithmetic with the other two hypot readings (sqrtf(x*x + y*y) /
// the host libm's correctly rounded hypotf), bit-identical to the oracle under the matching ORC_VAR_TVL1_*_HYPOT.
// 1: the opt-in fast arithmetic (tvl1_math_pk.h "fast"): FMA contraction, v_sqrt_f32 for the hypot, v_rcp_f32 for the
// divisions — a tolerance mode (max-abs <= 1e-3 of the exact flow on the BASELINE clips).

enum { Q_P11 = 0, Q_P21, Q_U1, Q_U2, Q_PLANES };

// The lean form of the tile function (LK = true: the step kernel's default, 128 VGPRs = 4 waves per SIMD).  Same tile,
// same rows per thread, same arithmetic and error-sum order, but the tile's data lives elsewhere:
//   * the lane +-1 neighbours (p11 / p21 from the left, u1 / u2 from the right) come from the neighbouring lane's register
//     by DPP (wave_shr:1 / wave_shl:1; a tile row is exactly one wave) instead of through the four [TH][64] LDS planes.  gfx9
//     has no DPP on VOP3P: the primal's p - p_left is formed per half (v_subrev_f32 with a DPP source), the dual's
//     u_right - u from v_mov_b32_dpp values; either way every half is the same IEEE subtraction as before.  Lane 0 (left) and lane 63 (right) receive 0 instead of their own value: in an interior
//     tile they are halo lanes outside every owned pixel's dependency cone over n_iters <= K iterations, and at the image
//     border the has_left / has_right selects replace them as before;
//   * rho_c, grad and 1/grad, constant over the iterations, move into the LDS that frees: float2-interleaved planes
//     kc[KC_*][role * HP + j][lane], one ds_read_b64 per float2 (wave-private: no barrier); l_t * grad is recomputed in the
//     loop (the same product, the same bits);
//   * the vertical neighbours across roles travel through boundary rows for u as they already did for p12 / p22:
//     bnd[B_*][2 * NW][64].
// LDS: 3 x [TH/2][64] float2 + 4 x [2 * NW][64] float = 32 KB at TH = 32 (the register form: 36 KB).
enum { KC_RHOC = 0, KC_GRAD, KC_RGRAD, KC_PLANES };
enum { B_P12 = 0, B_P22, B_U1, B_U2, B_PLANES };

// the value of lane - 1 (lane 0: 0) / lane + 1 (lane 63: 0) of a wave (the border tiles, where a select follows)
__device__ __forceinline__ float lane_from_left(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); // wave_shr:1
}
__device__ __forceinline__ float lane_from_right(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true)); // wave_shl:1
}

// The interior tiles' primal differences: a - (a of lane - 1) and b - (b of lane - 1) for both halves, one v_subrev_f32 with
// a DPP source each (lane 0: a - 0).  Inline assembly because the compiler packs the scalar subtractions back into
// v_pk_add_f32 (SLP), which takes no DPP operand, and then keeps a v_mov_b32_dpp per half.
// s_nop 1: a DPP instruction reading a VGPR that a VALU instruction wrote needs two wait states in between.
__device__ __forceinline__ void sub_from_left(f2 a, f2 b, f2 &da, f2 &db) {
    float r0, r1, r2, r3;
    asm("s_nop 1\n\t"
        "v_subrev_f32_dpp %0, %4, %4 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_subrev_f32_dpp %1, %5, %5 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_subrev_f32_dpp %2, %6, %6 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_subrev_f32_dpp %3, %7, %7 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y));
    da = pk_set(r0, r1);
    db = pk_set(r2, r3);
}

// The interior tiles' dual differences: (a of lane + 1) - a and (b of lane + 1) - b for both halves, one v_sub_f32 with a DPP
// source each (lane 63: 0 - a) instead of a v_mov_b32_dpp per half and a packed subtraction.  The same IEEE subtraction per
// half.  Its results feed the max / min of the CUDA hypot reading, and in front of its own v_max_f32 / v_min_f32 the compiler
// puts a canonicalising v_max_f32 per half after inline assembly (it cannot know that a difference is never a signalling
// NaN): pk_dual<HYP, true> therefore forms max / min in assembly as well (pk_abs_max_min).
//
// What the loop cost after these (profiles/tvl1_loop_diet/, static, interior tile, a role without skips, per iteration = 4
// float2s of two rows each; since then the convergence check left the iterations that have none: TVL1_CHECK_PEEL below, 482):
// 550 vector instructions in k_tvl1_step_fused<true, 0> (581 before), 539 in k_tvl1_warp_head<0> (570), of
// them 332 packed and 32 with a DPP source; 17 / 16 ds_*; 108 / 121 s_nop (87 / 103).  Three reductions made the difference,
// each bit-identical and measured alone against the parent on one MI355X (bench.py --steps 20 --warmup 5, three alternations,
// parent 540.6 - 541.2 pairs/s): the square root inside pk_dual_denominator without its NaN guard 543.5 - 545.5 (+0.7 %), that
// and its half reciprocal root unrefined 547.6 - 549.3 (+1.4 %), this subtraction 541.9 - 543.9 (+0.4 %); all three on another
// box 544.9 - 545.7 against 533.7 - 534.9 (+2.1 %).  Rejected: pk_threshold's two compares and two selects per half as one compare
// of |rho| against l_t * grad, one v_bfi_b32 (l_t with the sign of the quotient) and one select — 8 vector instructions fewer
// per iteration, bit-identical on 2^22 operands and at every boundary, but 540.4 - 542.1 alone (+0.07 %: inside the parent's
// spread) and nothing on top of the others; it is valid for lambda >= 0 only, which the engine does not require, so it
// needed a second path for such handles.  Not kept.
#ifndef TVL1_DPP_USUB
#define TVL1_DPP_USUB 1 // 0: v_mov_b32_dpp + compiler-generated subtractions (A/B switch for measurements)
#endif
__device__ __forceinline__ void sub_right_minus_self(f2 a, f2 b, f2 &da, f2 &db) {
    float r0, r1, r2, r3;
    asm("s_nop 1\n\t"
        "v_sub_f32_dpp %0, %4, %4 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_sub_f32_dpp %1, %5, %5 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_sub_f32_dpp %2, %6, %6 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_sub_f32_dpp %3, %7, %7 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3)
        : "v"(a.x), "v"(a.y), "v"(b.x), "v"(b.y));
    da = pk_set(r0, r1);
    db = pk_set(r2, r3);
}

// The convergence check out of the iterations that have none (profiles/tvl1_check_peel/).  Only the last iteration of a step
// that ends a segment evaluates the error, a few of the ~120 coarsest-level steps of a headline batch; written as
// `if (chk) { e = u - u_new; e1s = e1 * e1 + e2 * e2; }` the compiler if-converts the block and every iteration pays for it:
// the differences, squares and sum (20 packed operations), a select per half on the wave-uniform `chk` to keep the old e1s,
// and the float -> double conversions, additions and ownership selects of the sum itself.  With this switch the lean form's
// loop takes one wave-uniform branch per iteration into one of two copies of the primal half: without the check (nothing of
// the above, u updated in place) or with it; the dual half is common.  Interior loop of k_tvl1_step_fused<true, 0>, a role
// without skips, static: 550 -> 482 vector instructions in an iteration without a check (534 with one), of them 332 -> 312
// packed, 32 with a DPP source as before; s_nop 108 -> 127.  Against the parent on one MI355X (bench.py --steps 20 --warmup 5,
// three alternations): 557.0 - 558.9 vs 546.6 - 549.2 pairs/s (+1.9 %), the step kernel 926 -> 904 us per launch, the same bits.
// The register forms (LK = false) keep the one body: they have no register to spare.  Peeling whole iterations off the loop
// (a second copy of both halves behind it) gave the step kernel 8 - 36 bytes of scratch and 55 KB of code; this form stays at
// 128 VGPRs without scratch and at 45 KB.  0: one body, the check decided in every iteration (A/B switch for measurements).
// Rejected with it: the four vertical-neighbour differences of a float2 as one v_sub_f32 per half in assembly instead of the
// compiler's two v_mov_b32 + v_pk_add_f32 (16 vector instructions fewer per iteration) — alone 551.9 - 553.7, whose lowest run
// is not above the parent's highest by the parent's spread (by 0.01 pairs/s), and alone it left the warp-and-head kernel with 68
// bytes of nominal scratch; on top of the peel it gave 560.9 - 561.2 (+0.5 %).  Not kept.
#ifndef TVL1_CHECK_PEEL
#define TVL1_CHECK_PEEL 1
#endif

// The packed tile function in four phases: issue the HBM loads of a tile (raw, into registers) / turn them into the
// tile state (mask, pack, 1/grad, LDS neighbour planes) / iterate / store the owned region.

constexpr int PF_PLANES = 9; // I1wx, I1wy, rho_c, u1, u2, p11, p12, p21, p22 of ping-pong set S

// Which tile rows a thread holds (trapezoid layout): half e of float2 j is
//   e = 0: row role*HP + j,  e = 1: row TH-1 - role*HP - j
// Every row is paired with its mirror image, so both halves of a float2 are equally far from the tile's top / bottom
// edge: the halo rows of the temporal blocking, whose values stop mattering as the fused iterations proceed, sit
// together in the float2s of role 0 and can be SKIPPED as whole packed operations (tile_iterate_trap).
// role = (wave + workgroup) % NW, so the light role visits every SIMD equally often.
template <int TH, int NW> struct RowMap {
    static constexpr int RPT = TH / NW, HP = RPT / 2;
    static __device__ __forceinline__ int who() { // role of this wave
        const int wave = threadIdx.x >> 6;
        return (int)((wave + blockIdx.x) % NW);
    }
    static __device__ __forceinline__ int row(int who, int j, int e) { return e ? TH - 1 - who * HP - j : who * HP + j; }
};

template <int HP> struct TileState {
    f2 kwx[HP], kwy[HP], kgr[HP], krg[HP], klg[HP], krc[HP];
    f2 u1[HP], u2[HP], p11[HP], p12[HP], p21[HP], p22[HP];
};

// pf[plane][j][e] = half e of float2 j (RowMap).
template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ void tile_issue_loads(const Tvl1LevelCtx &c, int b, int S, int x0, int y0,
                                                 float (&pf)[PF_PLANES][TH / NW / 2][2]) {
    constexpr int RPT = TH / NW, HP = RPT / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, who = RM::who();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const dfx_rsrc rs = pair_rsrc(c, b); // (buffer addressing: tvl1_device_common.h)
    const unsigned so[PF_PLANES] = {plane_soff(c, PL_I1WX),         plane_soff(c, PL_I1WY),
                                    plane_soff(c, PL_RHOC),         plane_soff(c, PL_U1_0 + 2 * S),
                                    plane_soff(c, PL_U2_0 + 2 * S),  plane_soff(c, PL_P11_0 + 4 * S),
                                    plane_soff(c, PL_P12_0 + 4 * S), plane_soff(c, PL_P21_0 + 4 * S),
                                    plane_soff(c, PL_P22_0 + 4 * S)};
#pragma unroll
    for (int j = 0; j < HP; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gy = y0 + RM::row(who, j, e);
            const bool in = INTERIOR || (col_in && gy >= 0 && gy < c.h);
#if DFX_TVL1_DEBUG == 2 // measurement build only: the arithmetic without the HBM traffic (WRONG flows)
            const unsigned o = 4u * (unsigned)(lx + (in ? 0 : 64));
#else
            const unsigned o = in ? 4u * (unsigned)(gy * c.pitch + gx) : 0u; // masked lanes read element 0
#endif
#pragma unroll
            for (int q = 0; q < PF_PLANES; ++q)
                pf[q][j][e] = buf_ld(rs, o, so[q]);
        }
}

// LK: lds = the KC_PLANES constant planes (as f2 [TH/2][64] each), bnd = B_PLANES boundary planes; kgr / krg / klg / krc
// of T are left unset (they live in LDS).  !LK: lds = the Q_PLANES neighbour planes, bnd = the p12 / p22 boundary planes.
template <int TH, int NW, bool INTERIOR, int MATH, bool LK = false>
__device__ __forceinline__ void tile_consume(const Tvl1LevelCtx &c, int x0, int y0,
                                             const float (&pf)[PF_PLANES][TH / NW / 2][2], TileState<TH / NW / 2> &T,
                                             float (*lds)[TH][64], float (*bnd)[2 * NW][64]) {
    constexpr int RPT = TH / NW, HP = RPT / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, rg = RM::who();
    f2 (*kc)[TH / 2][64] = reinterpret_cast<f2 (*)[TH / 2][64]>(lds);
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        float t[PF_PLANES][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gy = y0 + RM::row(rg, j, e);
            const bool in = INTERIOR || (col_in && gy >= 0 && gy < c.h);
#pragma unroll
            for (int q = 0; q < PF_PLANES; ++q)
                t[q][e] = in ? pf[q][j][e] : 0.0f;
        }
        T.kwx[j] = pk_set(t[0][0], t[0][1]);
        T.kwy[j] = pk_set(t[1][0], t[1][1]);
        // grad = I1wx^2 + I1wy^2 exactly as the warp computes it (A.5): one plane less to read per step
        T.kgr[j] = T.kwx[j] * T.kwx[j] + T.kwy[j] * T.kwy[j];
        T.krc[j] = pk_set(t[2][0], t[2][1]);
        T.u1[j] = pk_set(t[3][0], t[3][1]);
        T.u2[j] = pk_set(t[4][0], t[4][1]);
        T.p11[j] = pk_set(t[5][0], t[5][1]);
        T.p12[j] = pk_set(t[6][0], t[6][1]);
        T.p21[j] = pk_set(t[7][0], t[7][1]);
        T.p22[j] = pk_set(t[8][0], t[8][1]);
        if (MATH != 1) { // 1 / grad where the chain's third arm can apply, 0 where grad <= FLT_EPSILON (pk_threshold)
            const f2 r = pk_refined_rcp(T.kgr[j]);
            T.krg[j] = pk_set(T.kgr[j].x > FLT_EPSILON ? r.x : 0.0f, T.kgr[j].y > FLT_EPSILON ? r.y : 0.0f);
            T.klg[j] = c.k.l_t * T.kgr[j];
        } else { // fast: the iteration only needs l_t * grad and -1 / grad (0 where grad <= FLT_EPSILON: no update)
            const f2 r = pk_refined_rcp(T.kgr[j]);
            T.krg[j] = pk_set(T.kgr[j].x > FLT_EPSILON ? -r.x : 0.0f, T.kgr[j].y > FLT_EPSILON ? -r.y : 0.0f);
            T.kgr[j] = c.k.l_t * T.kgr[j];
        }
        if (LK) {
            kc[KC_RHOC][rg * HP + j][lx] = T.krc[j];
            kc[KC_GRAD][rg * HP + j][lx] = T.kgr[j];
            kc[KC_RGRAD][rg * HP + j][lx] = T.krg[j];
        } else {
            lds[Q_P11][RM::row(rg, j, 0)][lx] = T.p11[j].x;
            lds[Q_P11][RM::row(rg, j, 1)][lx] = T.p11[j].y;
            lds[Q_P21][RM::row(rg, j, 0)][lx] = T.p21[j].x;
            lds[Q_P21][RM::row(rg, j, 1)][lx] = T.p21[j].y;
        }
    }
    // rows read as upper neighbours by other roles: the last upper-half row, the highest lower-half row
    bnd[0][rg][lx] = T.p12[HP - 1].x;
    bnd[1][rg][lx] = T.p22[HP - 1].x;
    bnd[0][NW + rg][lx] = T.p12[0].y;
    bnd[1][NW + rg][lx] = T.p22[0].y;
}

// n_iters inner iterations on the tile state; ends with a barrier.  Returns this thread's share of sum(diff) of the
// last iteration when do_check.
//   * vertical neighbours: the upper half of float2 j looks up to float2 j-1 and down to j+1, the mirrored lower
//     half the other way round, so the subtrahend of (p12 - p12_up) and the minuend of (u_down - u) take their halves
//     from two different float2s.  The source writes them per half; the compiler packs each back into one v_pk_add_f32
//     with negated operands behind two v_mov_b32 that assemble the register pair (32 of the loop's 33 v_mov_b32: three
//     instructions per difference where two v_sub_f32 would do — tried and not kept, see TVL1_CHECK_PEEL above);
//   * the convergence check belongs to the last iteration alone: the lean form branches, once per iteration and
//     wave-uniformly, between a primal half without it and one with it (TVL1_CHECK_PEEL);
//   * iteration m of n only has to produce rows that the owned region [K, TH-K) can still depend on: with
//     d = n - m iterations to go, u is needed on [K-d, TH-K+d] and p on [K-d, TH-K+d).  For the float2 whose rows are
//     a from the edges that means: primal update iff a >= K-d-1, dual update iff a >= K-d.  Role 0 (a = 0 .. HP-1)
//     skips 6 of its 16 primal and 10 of its 16 dual float2-updates at K = 4: 14 % of the arithmetic of a full step.
//     Skipped rows keep stale values nobody reads (the store and the error sum only touch rows >= K).
// LK: the lean form (DPP lane neighbours, constants from LDS; see the top of this file), lds / bnd as in tile_consume.
template <int TH, int NW, bool INTERIOR, bool SKIPS, int MATH, bool LK = false>
__device__ __forceinline__ double tile_iterate_trap(const Tvl1LevelCtx &c, TileState<TH / NW / 2> &T,
                                                    float (*lds)[TH][64], float (*bnd)[2 * NW][64], int n_iters,
                                                    bool do_check, int K, int x0, int y0, int role, bool own_lo,
                                                    bool own_hi) {
    const f2 (*kc)[TH / 2][64] = reinterpret_cast<const f2 (*)[TH / 2][64]>(lds);
    constexpr int TW = 64;
    constexpr int RPT = TH / NW, HP = RPT / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63;
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool has_left = INTERIOR || gx > 0, has_right = INTERIOR || gx + 1 < c.w;
    const int lxl = max(lx - 1, 0), lxr = min(lx + 1, TW - 1);
    const bool col_owned = (lx >= K || own_lo) && (lx < TW - K || own_hi) && col_in;
    const float l_t = c.k.l_t, theta = c.k.theta, taut = c.k.taut;
    const float taut_s = taut * TVL1_SQRT_DOWN; // exact: see pk_dual
    const int a0 = role * HP;                  // distance of float2 0 from the tile's top / bottom edge
    const int xu = max(role - 1, 0);           // bnd slot of the row above this role's upper half (role 0: halo)
    const bool innermost = role == NW - 1;     // its two halves touch: rows TH/2-1 and TH/2
    const int yu = NW + min(role + 1, NW - 1); // bnd slot of the row above this role's lower half
    const int row_xd = a0 + HP;                // row below the upper half
    const int row_yd = min(TH - a0, TH - 1);   // row below the lower half (role 0: clamped, halo)
    double dsum = 0.0;
    constexpr bool PEEL = LK && TVL1_CHECK_PEEL;
#if DFX_TVL1_DEBUG == 1
    n_iters = 0;
#endif
    // The primal half of iteration `it`.  CM says what it knows about the convergence check: 0 = this iteration has none (no
    // difference, no square, no select; u is updated in place), 1 = it has one, 2 = decided at run time (do_check and the
    // last iteration; the compiler if-converts that into selects on a wave-uniform condition in every iteration).
    f2 e1s[HP]; // (declared out here, not inside the lambda: there it costs k_tvl1_step_fused_nbr_lds<1> two registers)
    auto primal = [&](const int it, auto cm) __attribute__((always_inline)) {
        constexpr int CM = decltype(cm)::value;
        const bool chk = CM == 2 ? do_check && (it == n_iters - 1) : CM == 1;
        const int need = K - (n_iters - 1 - it); // rows closer than this to the edge need no dual update any more
        // ---- primal update (A.6)
        const float p12ux = bnd[0][xu][lx], p22ux = bnd[1][xu][lx];
        const float p12uy = innermost ? T.p12[HP - 1].x : bnd[0][yu][lx];
        const float p22uy = innermost ? T.p22[HP - 1].x : bnd[1][yu][lx];
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            if (SKIPS && a0 + j < need - 1) {
                e1s[j] = (f2)(0.0f);
                continue;
            }
            const int lya = RM::row(role, j, 0), lyb = RM::row(role, j, 1);
            const f2 krc = LK ? kc[KC_RHOC][role * HP + j][lx] : T.krc[j];
            const f2 kgr = LK ? kc[KC_GRAD][role * HP + j][lx] : T.kgr[j];
            const f2 krg = LK ? kc[KC_RGRAD][role * HP + j][lx] : T.krg[j];
            f2 v1, v2;
            if (MATH != 1)
                pk_threshold(T.kwx[j], T.kwy[j], kgr, krg, LK ? l_t * kgr : T.klg[j], krc, T.u1[j], T.u2[j], l_t, v1, v2);
            else
                pk_threshold_fast(T.kwx[j], T.kwy[j], kgr, krg, krc, T.u1[j], T.u2[j], l_t, v1, v2);
            f2 p11l, p21l; // (the interior lean form needs only the differences)
            if (!LK) {
                p11l = pk_set(lds[Q_P11][lya][lxl], lds[Q_P11][lyb][lxl]);
                p21l = pk_set(lds[Q_P21][lya][lxl], lds[Q_P21][lyb][lxl]);
            } else if (!INTERIOR) {
                p11l = pk_set(lane_from_left(T.p11[j].x), lane_from_left(T.p11[j].y));
                p21l = pk_set(lane_from_left(T.p21[j].x), lane_from_left(T.p21[j].y));
            }
            // upper neighbours: upper half <- float2 j-1, lower half <- float2 j+1
            const f2 p12u = pk_set(j > 0 ? T.p12[j > 0 ? j - 1 : 0].x : p12ux,
                                   j + 1 < HP ? T.p12[j + 1 < HP ? j + 1 : 0].y : p12uy);
            const f2 p22u = pk_set(j > 0 ? T.p22[j > 0 ? j - 1 : 0].x : p22ux,
                                   j + 1 < HP ? T.p22[j + 1 < HP ? j + 1 : 0].y : p22uy);
            f2 div1, div2;
            if (INTERIOR && LK) { // p11 - p11l per half: the DPP operand cannot feed a packed instruction
                f2 d1, d2;
                sub_from_left(T.p11[j], T.p21[j], d1, d2);
                div1 = d1 + (T.p12[j] - p12u);
                div2 = d2 + (T.p22[j] - p22u);
            } else if (INTERIOR) {
                div1 = (T.p11[j] - p11l) + (T.p12[j] - p12u);
                div2 = (T.p21[j] - p21l) + (T.p22[j] - p22u);
            } else {
                const bool up_a = y0 + lya > 0, up_b = y0 + lyb > 0;
                div1 = pk_divergence(T.p11[j], p11l, T.p12[j], p12u, has_left, up_a, up_b);
                div2 = pk_divergence(T.p21[j], p21l, T.p22[j], p22u, has_left, up_a, up_b);
            }
            const f2 u1n = MATH != 1 ? v1 + theta * div1 : pk_fma((f2)(theta), div1, v1);
            const f2 u2n = MATH != 1 ? v2 + theta * div2 : pk_fma((f2)(theta), div2, v2);
            if (chk) {
                const f2 e1 = T.u1[j] - u1n, e2 = T.u2[j] - u2n;
                e1s[j] = MATH != 1 ? e1 * e1 + e2 * e2 : pk_fma(e1, e1, e2 * e2);
            }
            T.u1[j] = u1n;
            T.u2[j] = u2n;
            if (!LK) {
                lds[Q_U1][lya][lx] = u1n.x;
                lds[Q_U1][lyb][lx] = u1n.y;
                lds[Q_U2][lya][lx] = u2n.x;
                lds[Q_U2][lyb][lx] = u2n.y;
            }
        }
        if (LK) { // rows read as lower neighbours by other roles: the first upper-half row, the highest lower-half row
            bnd[B_U1][role][lx] = T.u1[0].x;
            bnd[B_U2][role][lx] = T.u2[0].x;
            bnd[B_U1][NW + role][lx] = T.u1[HP - 1].y;
            bnd[B_U2][NW + role][lx] = T.u2[HP - 1].y;
        }
        if (chk) { // rows in ascending order within each half
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int jj = 0; jj < HP; ++jj) {
                    const int j = e ? HP - 1 - jj : jj;
                    const int ly = RM::row(role, j, e), gy = y0 + ly;
                    const bool owned = col_owned && ly >= K && ly < TH - K && (INTERIOR || (gy >= 0 && gy < c.h));
                    const float dv = e ? e1s[j].y : e1s[j].x;
                    dsum += owned ? (double)dv : 0.0;
                }
        }
        __syncthreads();
    };
    auto dual = [&](const int it) __attribute__((always_inline)) {
        const int need = K - (n_iters - 1 - it);
        // ---- dual update (A.7)
        float u1dx, u2dx, u1dy, u2dy;
        if (LK) { // row a0 + HP: role + 1's first upper-half row (innermost: its own lower half); row TH - a0: role - 1's
                  // highest lower-half row (role 0: clamped to its own row TH - 1, halo)
            u1dx = innermost ? T.u1[HP - 1].y : bnd[B_U1][min(role + 1, NW - 1)][lx];
            u2dx = innermost ? T.u2[HP - 1].y : bnd[B_U2][min(role + 1, NW - 1)][lx];
            u1dy = role == 0 ? T.u1[0].y : bnd[B_U1][NW + max(role - 1, 0)][lx];
            u2dy = role == 0 ? T.u2[0].y : bnd[B_U2][NW + max(role - 1, 0)][lx];
        } else {
            u1dx = lds[Q_U1][row_xd][lx];
            u2dx = lds[Q_U2][row_xd][lx];
            u1dy = lds[Q_U1][row_yd][lx];
            u2dy = lds[Q_U2][row_yd][lx];
        }
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            if (SKIPS && a0 + j < need)
                continue;
            const int lya = RM::row(role, j, 0), lyb = RM::row(role, j, 1);
            f2 u1r, u2r; // (the interior lean form needs only the differences)
            if (!LK) {
                u1r = pk_set(lds[Q_U1][lya][lxr], lds[Q_U1][lyb][lxr]);
                u2r = pk_set(lds[Q_U2][lya][lxr], lds[Q_U2][lyb][lxr]);
            } else if (!INTERIOR) {
                u1r = pk_set(lane_from_right(T.u1[j].x), lane_from_right(T.u1[j].y));
                u2r = pk_set(lane_from_right(T.u2[j].x), lane_from_right(T.u2[j].y));
            }
            // lower neighbours: upper half <- float2 j+1, lower half <- float2 j-1
            f2 u1d = pk_set(j + 1 < HP ? T.u1[j + 1 < HP ? j + 1 : 0].x : u1dx, j > 0 ? T.u1[j > 0 ? j - 1 : 0].y : u1dy);
            f2 u2d = pk_set(j + 1 < HP ? T.u2[j + 1 < HP ? j + 1 : 0].x : u2dx, j > 0 ? T.u2[j > 0 ? j - 1 : 0].y : u2dy);
            if (!INTERIOR) {
                const bool dn_a = y0 + lya + 1 < c.h, dn_b = y0 + lyb + 1 < c.h;
                u1r.x = has_right ? u1r.x : T.u1[j].x;
                u1r.y = has_right ? u1r.y : T.u1[j].y;
                u2r.x = has_right ? u2r.x : T.u2[j].x;
                u2r.y = has_right ? u2r.y : T.u2[j].y;
                u1d.x = dn_a ? u1d.x : T.u1[j].x;
                u1d.y = dn_b ? u1d.y : T.u1[j].y;
                u2d.x = dn_a ? u2d.x : T.u2[j].x;
                u2d.y = dn_b ? u2d.y : T.u2[j].y;
            }
            // u_right - u: per half with the DPP source in the interior lean form, packed otherwise — the same bits
            f2 u1x, u2x;
            constexpr bool USUB = LK && INTERIOR && TVL1_DPP_USUB && MATH != 1 && MATH != TVL1_HYP_LIBM;
            if (USUB) {
                sub_right_minus_self(T.u1[j], T.u2[j], u1x, u2x);
            } else if (LK && INTERIOR) {
                u1x = pk_set(lane_from_right(T.u1[j].x) - T.u1[j].x, lane_from_right(T.u1[j].y) - T.u1[j].y);
                u2x = pk_set(lane_from_right(T.u2[j].x) - T.u2[j].x, lane_from_right(T.u2[j].y) - T.u2[j].y);
            } else {
                u1x = u1r - T.u1[j];
                u2x = u2r - T.u2[j];
            }
            if (MATH != 1) {
                pk_dual<MATH, USUB, LK>(T.p11[j], T.p12[j], u1x, u1d - T.u1[j], taut, taut_s);
                pk_dual<MATH, USUB, LK>(T.p21[j], T.p22[j], u2x, u2d - T.u2[j], taut, taut_s);
            } else {
                pk_dual_fast(T.p11[j], T.p12[j], u1x, u1d - T.u1[j], taut);
                pk_dual_fast(T.p21[j], T.p22[j], u2x, u2d - T.u2[j], taut);
            }
            if (!LK) {
                lds[Q_P11][lya][lx] = T.p11[j].x;
                lds[Q_P11][lyb][lx] = T.p11[j].y;
                lds[Q_P21][lya][lx] = T.p21[j].x;
                lds[Q_P21][lyb][lx] = T.p21[j].y;
            }
        }
        bnd[0][role][lx] = T.p12[HP - 1].x;
        bnd[1][role][lx] = T.p22[HP - 1].x;
        bnd[0][NW + role][lx] = T.p12[0].y;
        bnd[1][NW + role][lx] = T.p22[0].y;
        __syncthreads();
    };
    for (int it = 0; it < n_iters; ++it) {
        if (!PEEL)
            primal(it, std::integral_constant<int, 2>());
        else if (do_check && it == n_iters - 1) // one wave-uniform branch per iteration; the dual half is common
            primal(it, std::integral_constant<int, 1>());
        else
            primal(it, std::integral_constant<int, 0>());
        dual(it);
    }
    return dsum;
}

// write back the owned region into ping-pong set D
template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ void tile_store(const Tvl1LevelCtx &c, int b, int D, int K, int x0, int y0,
                                           const TileState<TH / NW / 2> &T, bool own_lo, bool own_hi) {
    constexpr int TW = 64;
    constexpr int RPT = TH / NW, HP = RPT / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, rg = RM::who();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool col_owned = (lx >= K || own_lo) && (lx < TW - K || own_hi) && col_in;
    const dfx_rsrc rs = pair_rsrc(c, b);
    const unsigned s_u1 = plane_soff(c, PL_U1_0 + 2 * D), s_u2 = plane_soff(c, PL_U2_0 + 2 * D);
    const unsigned s_p11 = plane_soff(c, PL_P11_0 + 4 * D), s_p12 = plane_soff(c, PL_P12_0 + 4 * D);
    const unsigned s_p21 = plane_soff(c, PL_P21_0 + 4 * D), s_p22 = plane_soff(c, PL_P22_0 + 4 * D);
#pragma unroll
    for (int j = 0; j < HP; ++j) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int ly = RM::row(rg, j, e);
            const int gy = y0 + ly;
            if (col_owned && ly >= K && ly < TH - K && (INTERIOR || (gy >= 0 && gy < c.h)) && DFX_TVL1_DEBUG != 2) {
                const unsigned o = 4u * (unsigned)(gy * c.pitch + gx);
                buf_st(rs, o, s_u1, e ? T.u1[j].y : T.u1[j].x);
                buf_st(rs, o, s_u2, e ? T.u2[j].y : T.u2[j].x);
                buf_st(rs, o, s_p11, e ? T.p11[j].y : T.p11[j].x);
                buf_st(rs, o, s_p12, e ? T.p12[j].y : T.p12[j].x);
                buf_st(rs, o, s_p21, e ? T.p21[j].y : T.p21[j].x);
                buf_st(rs, o, s_p22, e ? T.p22[j].y : T.p22[j].x);
            }
        }
    }
}

