// tvl1_gamma_tile.h — the tile function of the -a=tvl1 inner loop WITH the illumination channel (dfx_params.tvl1_gamma != 0;
// device code), used by k_tvl1_step_fused_gamma (tvl1_kernels.hip).  A tile function of its own beside tvl1_tile.h's, so
// that the default kernels' code does not move.
// Semantics: cv::cuda tvl1flow.cu's estimateUKernel / estimateDualVariablesKernel with gamma, as restated in SURVEY.md
// A.6-A.7 "with gamma" (rated MED, parity unpinned).  Compiled with -ffp-contract=off (see tvl1_math.h).
//
// Same tile (64 x TH, K-pixel halo), same trapezoid row layout and skips, same error-sum order as tile_iterate_trap; the
// third channel's dependency cone is the first two's (u3 reads p31 / p32 of the left and upper neighbour, the dual reads u3
// of the right and lower one), so the geometry and the work accounting of tvl1_ctrl.h carry over.  The form is the lean one
// (tvl1_tile.h, LK): lane neighbours by DPP, rho_c / grad / 1/grad as float2 planes in LDS, vertical neighbours across
// roles through boundary rows — with three channels: 6 boundary planes instead of 4 (36 KB of LDS), and 11 state arrays
// per thread instead of 8, which is why the kernel is built for three waves per SIMD (162 VGPRs) and not four.
// Arithmetic: the exact mode with the default hypot reading only (tvl1_math 0).
#pragma once

#include "tvl1_tile.h"

enum { GB_PB = 0, GB_U = 3, GB_PLANES = 6 }; // boundary rows: p12, p22, p32 / u1, u2, u3

// I1wx, I1wy, rho_c, then per channel ch = 0, 1, 2: u, pa (p11 / p21 / p31), pb (p12 / p22 / p32) of ping-pong set S
constexpr int GPF_PLANES = 12;

template <int HP> struct GammaTileState {
    f2 kwx[HP], kwy[HP];
    f2 u[3][HP], pa[3][HP], pb[3][HP];
};

// A.6 with gamma: rho = rho_c + ((I1wx*u1 + I1wy*u2) + gamma*u3); the chain's factor (l_t, -l_t, fi, 0) multiplies I1wx,
// I1wy and gamma (pk_threshold: selecting the factor first gives the bits of selecting among the products).
__device__ __forceinline__ void pk_threshold_gamma(f2 I1wx, f2 I1wy, f2 grad, f2 rgrad, f2 lg, f2 rho_c, f2 u1, f2 u2, f2 u3,
                                                   float l_t, float gamma, f2 (&v)[3]) {
    const f2 rho = rho_c + ((I1wx * u1 + I1wy * u2) + gamma * u3);
    f2 f = pk_div_with_rcp(-rho, grad, rgrad);
    f.x = rho.x > lg.x ? -l_t : f.x;
    f.y = rho.y > lg.y ? -l_t : f.y;
    f.x = rho.x < -lg.x ? l_t : f.x;
    f.y = rho.y < -lg.y ? l_t : f.y;
    v[0] = u1 + f * I1wx;
    v[1] = u2 + f * I1wy;
    v[2] = u3 + f * gamma;
}

// a - (a of lane - 1) for both halves (lane 0: a - 0): sub_from_left of tvl1_tile.h for one float2
__device__ __forceinline__ f2 sub_from_left1(f2 a) {
    float r0, r1;
    asm("s_nop 1\n\t"
        "v_subrev_f32_dpp %0, %2, %2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "v_subrev_f32_dpp %1, %3, %3 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(r0), "=&v"(r1)
        : "v"(a.x), "v"(a.y));
    return pk_set(r0, r1);
}

template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ void gamma_tile_issue_loads(const Tvl1LevelCtx &c, int b, int S, int x0, int y0,
                                                       float (&pf)[GPF_PLANES][TH / NW / 2][2]) {
    constexpr int HP = TH / NW / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, who = RM::who();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const dfx_rsrc rs = pair_rsrc(c, b); // the slot's size follows c.slot_stride: all 22 planes are in range
    unsigned so[GPF_PLANES] = {plane_soff(c, PL_I1WX), plane_soff(c, PL_I1WY), plane_soff(c, PL_RHOC)};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        so[3 + 3 * ch] = plane_soff(c, tvl1_pl_u(ch, S));
        so[4 + 3 * ch] = plane_soff(c, tvl1_pl_p(ch, S));
        so[5 + 3 * ch] = plane_soff(c, tvl1_pl_p(ch, S) + 1);
    }
#pragma unroll
    for (int j = 0; j < HP; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gy = y0 + RM::row(who, j, e);
            const bool in = INTERIOR || (col_in && gy >= 0 && gy < c.h);
            const unsigned o = in ? 4u * (unsigned)(gy * c.pitch + gx) : 0u; // masked lanes read element 0
#pragma unroll
            for (int q = 0; q < GPF_PLANES; ++q)
                pf[q][j][e] = buf_ld(rs, o, so[q]);
        }
}

// kc: the KC_PLANES constant planes, bnd: the GB_PLANES boundary planes
template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ void gamma_tile_consume(const Tvl1LevelCtx &c, int x0, int y0,
                                                   const float (&pf)[GPF_PLANES][TH / NW / 2][2],
                                                   GammaTileState<TH / NW / 2> &T, f2 (*kc)[TH / 2][64],
                                                   float (*bnd)[2 * NW][64]) {
    constexpr int HP = TH / NW / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, rg = RM::who();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
#pragma unroll
    for (int j = 0; j < HP; ++j) {
        float t[GPF_PLANES][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int gy = y0 + RM::row(rg, j, e);
            const bool in = INTERIOR || (col_in && gy >= 0 && gy < c.h);
#pragma unroll
            for (int q = 0; q < GPF_PLANES; ++q)
                t[q][e] = in ? pf[q][j][e] : 0.0f;
        }
        T.kwx[j] = pk_set(t[0][0], t[0][1]);
        T.kwy[j] = pk_set(t[1][0], t[1][1]);
        // grad = I1wx^2 + I1wy^2 as the warp computes it (A.5; no gamma^2 term)
        const f2 kgr = T.kwx[j] * T.kwx[j] + T.kwy[j] * T.kwy[j];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            T.u[ch][j] = pk_set(t[3 + 3 * ch][0], t[3 + 3 * ch][1]);
            T.pa[ch][j] = pk_set(t[4 + 3 * ch][0], t[4 + 3 * ch][1]);
            T.pb[ch][j] = pk_set(t[5 + 3 * ch][0], t[5 + 3 * ch][1]);
        }
        const f2 r = pk_refined_rcp(kgr); // 1 / grad where the chain's third arm can apply, 0 elsewhere (pk_threshold)
        kc[KC_RHOC][rg * HP + j][lx] = pk_set(t[2][0], t[2][1]);
        kc[KC_GRAD][rg * HP + j][lx] = kgr;
        kc[KC_RGRAD][rg * HP + j][lx] = pk_set(kgr.x > FLT_EPSILON ? r.x : 0.0f, kgr.y > FLT_EPSILON ? r.y : 0.0f);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { // rows read as upper neighbours by other roles
        bnd[GB_PB + ch][rg][lx] = T.pb[ch][HP - 1].x;
        bnd[GB_PB + ch][NW + rg][lx] = T.pb[ch][0].y;
    }
}

// n_iters inner iterations on the tile state; ends with a barrier.  Returns this thread's share of sum(diff) of the last
// iteration when do_check (diff = (u1 - u1new)^2 + (u2 - u2new)^2: u3 does not enter it).  Row bookkeeping and skips:
// tile_iterate_trap.
template <int TH, int NW, bool INTERIOR, bool SKIPS>
__device__ __forceinline__ double gamma_tile_iterate(const Tvl1LevelCtx &c, GammaTileState<TH / NW / 2> &T,
                                                     const f2 (*kc)[TH / 2][64], float (*bnd)[2 * NW][64], int n_iters,
                                                     bool do_check, int K, int x0, int y0, int role, bool own_lo,
                                                     bool own_hi) {
    constexpr int TW = 64;
    constexpr int HP = TH / NW / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63;
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool has_left = INTERIOR || gx > 0, has_right = INTERIOR || gx + 1 < c.w;
    const bool col_owned = (lx >= K || own_lo) && (lx < TW - K || own_hi) && col_in;
    const float l_t = c.k.l_t, theta = c.k.theta, taut = c.k.taut, gamma = c.k.gamma;
    const float taut_s = taut * TVL1_SQRT_DOWN; // exact: see pk_dual
    const int a0 = role * HP;                  // distance of float2 0 from the tile's top / bottom edge
    const int xu = max(role - 1, 0);           // bnd slot of the row above this role's upper half (role 0: halo)
    const bool innermost = role == NW - 1;     // its two halves touch: rows TH/2-1 and TH/2
    const int yu = NW + min(role + 1, NW - 1); // bnd slot of the row above this role's lower half
    double dsum = 0.0;
    for (int it = 0; it < n_iters; ++it) {
        const bool chk = do_check && (it == n_iters - 1);
        const int need = K - (n_iters - 1 - it); // rows closer than this to the edge need no dual update any more
        // ---- primal update (A.6)
        float pbux[3], pbuy[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            pbux[ch] = bnd[GB_PB + ch][xu][lx];
            pbuy[ch] = innermost ? T.pb[ch][HP - 1].x : bnd[GB_PB + ch][yu][lx];
        }
        f2 e1s[HP];
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            if (SKIPS && a0 + j < need - 1) {
                e1s[j] = (f2)(0.0f);
                continue;
            }
            const int lya = RM::row(role, j, 0), lyb = RM::row(role, j, 1);
            const f2 krc = kc[KC_RHOC][role * HP + j][lx];
            const f2 kgr = kc[KC_GRAD][role * HP + j][lx];
            const f2 krg = kc[KC_RGRAD][role * HP + j][lx];
            f2 v[3], un[3];
            pk_threshold_gamma(T.kwx[j], T.kwy[j], kgr, krg, l_t * kgr, krc, T.u[0][j], T.u[1][j], T.u[2][j], l_t, gamma, v);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                // upper neighbours: upper half <- float2 j-1, lower half <- float2 j+1
                const f2 pbu = pk_set(j > 0 ? T.pb[ch][j > 0 ? j - 1 : 0].x : pbux[ch],
                                      j + 1 < HP ? T.pb[ch][j + 1 < HP ? j + 1 : 0].y : pbuy[ch]);
                f2 div;
                if (INTERIOR) {
                    div = sub_from_left1(T.pa[ch][j]) + (T.pb[ch][j] - pbu);
                } else {
                    const f2 pal = pk_set(lane_from_left(T.pa[ch][j].x), lane_from_left(T.pa[ch][j].y));
                    div = pk_divergence(T.pa[ch][j], pal, T.pb[ch][j], pbu, has_left, y0 + lya > 0, y0 + lyb > 0);
                }
                un[ch] = v[ch] + theta * div;
            }
            if (chk) {
                const f2 e1 = T.u[0][j] - un[0], e2 = T.u[1][j] - un[1];
                e1s[j] = e1 * e1 + e2 * e2;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                T.u[ch][j] = un[ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { // rows read as lower neighbours by other roles
            bnd[GB_U + ch][role][lx] = T.u[ch][0].x;
            bnd[GB_U + ch][NW + role][lx] = T.u[ch][HP - 1].y;
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
        // ---- dual update (A.7): row a0 + HP is role + 1's first upper-half row (innermost: its own lower half), row TH - a0
        // role - 1's highest lower-half row (role 0: clamped to its own row TH - 1, halo)
        float udx[3], udy[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            udx[ch] = innermost ? T.u[ch][HP - 1].y : bnd[GB_U + ch][min(role + 1, NW - 1)][lx];
            udy[ch] = role == 0 ? T.u[ch][0].y : bnd[GB_U + ch][NW + max(role - 1, 0)][lx];
        }
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            if (SKIPS && a0 + j < need)
                continue;
            const int lya = RM::row(role, j, 0), lyb = RM::row(role, j, 1);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const f2 u = T.u[ch][j];
                // lower neighbours: upper half <- float2 j+1, lower half <- float2 j-1
                f2 ud = pk_set(j + 1 < HP ? T.u[ch][j + 1 < HP ? j + 1 : 0].x : udx[ch],
                               j > 0 ? T.u[ch][j > 0 ? j - 1 : 0].y : udy[ch]);
                f2 ux;
                if (INTERIOR) {
                    ux = pk_set(lane_from_right(u.x) - u.x, lane_from_right(u.y) - u.y);
                } else {
                    const bool dn_a = y0 + lya + 1 < c.h, dn_b = y0 + lyb + 1 < c.h;
                    f2 ur = pk_set(lane_from_right(u.x), lane_from_right(u.y));
                    ur.x = has_right ? ur.x : u.x;
                    ur.y = has_right ? ur.y : u.y;
                    ud.x = dn_a ? ud.x : u.x;
                    ud.y = dn_b ? ud.y : u.y;
                    ux = ur - u;
                }
                pk_dual<TVL1_HYP_CUDA>(T.pa[ch][j], T.pb[ch][j], ux, ud - u, taut, taut_s);
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            bnd[GB_PB + ch][role][lx] = T.pb[ch][HP - 1].x;
            bnd[GB_PB + ch][NW + role][lx] = T.pb[ch][0].y;
        }
        __syncthreads();
    }
    return dsum;
}

// write back the owned region into ping-pong set D
template <int TH, int NW, bool INTERIOR>
__device__ __forceinline__ void gamma_tile_store(const Tvl1LevelCtx &c, int b, int D, int K, int x0, int y0,
                                                 const GammaTileState<TH / NW / 2> &T, bool own_lo, bool own_hi) {
    constexpr int TW = 64;
    constexpr int HP = TH / NW / 2;
    using RM = RowMap<TH, NW>;
    const int lx = threadIdx.x & 63, rg = RM::who();
    const int gx = x0 + lx;
    const bool col_in = INTERIOR || (gx >= 0 && gx < c.w);
    const bool col_owned = (lx >= K || own_lo) && (lx < TW - K || own_hi) && col_in;
    const dfx_rsrc rs = pair_rsrc(c, b);
    unsigned s_u[3], s_pa[3], s_pb[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        s_u[ch] = plane_soff(c, tvl1_pl_u(ch, D));
        s_pa[ch] = plane_soff(c, tvl1_pl_p(ch, D));
        s_pb[ch] = plane_soff(c, tvl1_pl_p(ch, D) + 1);
    }
#pragma unroll
    for (int j = 0; j < HP; ++j) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int ly = RM::row(rg, j, e);
            const int gy = y0 + ly;
            if (col_owned && ly >= K && ly < TH - K && (INTERIOR || (gy >= 0 && gy < c.h))) {
                const unsigned o = 4u * (unsigned)(gy * c.pitch + gx);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    buf_st(rs, o, s_u[ch], e ? T.u[ch][j].y : T.u[ch][j].x);
                    buf_st(rs, o, s_pa[ch], e ? T.pa[ch][j].y : T.pa[ch][j].x);
                    buf_st(rs, o, s_pb[ch], e ? T.pb[ch][j].y : T.pb[ch][j].x);
                }
            }
        }
    }
}
