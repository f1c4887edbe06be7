// dfx_device.h — data layout in HBM shared by the host control code and the HIP kernels.
//
// Layout (all planes are float32, row pitch padded to 64 floats = 256 B so every row starts on a
// cache-line boundary and 16-B vector accesses stay aligned):
//
//   frame slot f  : three pyramids  I, Ix, Iy     (Ix/Iy = centred gradient)
//                   level s lives at element offset lvl_off[s] of the slot, pitch lvl_pitch[s]
//   pair slot b   : n_planes work planes (16; 22 with tvl1_gamma) sized for level 0, reused by every level with the
//                   level's own pitch:  u[2 sets][2], p[2 sets][4], I1wx, I1wy, grad, rho_c
//                   (ping-pong sets: a fused U+dual step reads one set and writes the other)
//
// A frame's pyramid is built once and serves as I1 of pair i and as I0 of pair i+step.
#pragma once

#include "tvl1_ctrl.h"

#define DFX_LVL_MAX 16

// The most workgroups a launch takes along grid.y or grid.z.  A launcher that puts a caller's count of items (flows, frames,
// planes) there walks the batch in launches of at most this many and offsets every per-item pointer by the launch's first item.
constexpr int DFX_GRID_YZ_MAX = 65535;

enum : int {
    PL_U1_0 = 0, PL_U2_0, PL_U1_1, PL_U2_1,                // u sets 0/1
    PL_P11_0, PL_P12_0, PL_P21_0, PL_P22_0,                // p set 0
    PL_P11_1, PL_P12_1, PL_P21_1, PL_P22_1,                // p set 1
    PL_I1WX, PL_I1WY, PL_GRAD, PL_RHOC,
    PL_COUNT,
    // dfx_params.tvl1_gamma != 0: the illumination channel u3 and its dual (p31, p32) BEHIND the 16 planes above, whose
    // indices stay what they are; a pair slot then has PL_COUNT_GAMMA planes (Tvl1LevelCtx::n_planes)
    PL_U3_0 = PL_COUNT, PL_U3_1,                           // u3 sets 0/1
    PL_P31_0, PL_P32_0, PL_P31_1, PL_P32_1,                // (p31, p32) sets 0/1
    PL_COUNT_GAMMA
};
// plane of channel ch = 0, 1, 2 (u1, u2, u3) in ping-pong set S: u, and the first of its two dual planes (the second follows it)
DFX_HD constexpr int tvl1_pl_u(int ch, int S) { return ch < 2 ? PL_U1_0 + 2 * S + ch : PL_U3_0 + S; }
DFX_HD constexpr int tvl1_pl_p(int ch, int S) { return ch < 2 ? PL_P11_0 + 4 * S + 2 * ch : PL_P31_0 + 2 * S; }

struct PairDesc {
    int frame_a; // frame slot of I0
    int frame_b; // frame slot of I1
};

struct Tvl1Consts {
    float l_t;   // (float)(lambda*theta)
    float taut;  // (float)(tau/theta)
    float theta; // (float)theta
    int hyp;     // hypot reading of the exact arithmetic (tvl1_math.h: TVL1_HYP_*) for the scalar kernel forms
    float gamma; // (float)tvl1_gamma: weight of the illumination channel u3 (0: no such channel; only the gamma kernels read it)
};

// Everything a TVL1 kernel needs for one level; passed by value as the kernel argument.
struct Tvl1LevelCtx {
    // geometry of this level
    int w, h, pitch;
    // frame pyramids
    const float *frame_I;   // base of frame slot 0, pyramid I
    const float *frame_Ix;
    const float *frame_Iy;
    long long frame_stride; // elements between frame slots
    long long lvl_off;      // element offset of this level inside a frame slot
    // pair work planes
    float *planes;          // base of pair slot 0
    long long plane_stride; // elements between planes of one slot
    long long slot_stride;  // elements between pair slots
    // control
    Tvl1State *state;       // [n_pairs]
    const PairDesc *pairs;  // [n_pairs]
    double *partials;       // [n_pairs][partials_stride]
    int partials_stride;
    int n_pairs;
    Tvl1LoopCfg loop;
    Tvl1Consts k;
    double thr;             // scaledEpsilon of this level = eps^2 * (w*h)   (A.3)
    int level;              // level index (0 = full resolution)
    int *iters_out;         // [n_pairs][DFX_LVL_MAX][TVL1_MAX_WARPS] executed inner iterations
    int *checks_out;        // [n_pairs][DFX_LVL_MAX][2] convergence sums evaluated, steps that did work
    long long *work_out;    // [n_pairs][DFX_LVL_MAX][2] half-row updates per tile column: step kernel, warp-and-head kernel
    // completion signalling
    unsigned int *level_done_count; // device counter of pairs that finished the level
    volatile int *host_done_flag;   // pinned host word: set to done_token when every pair finished
    int done_token;
    int split_warp; // the backward warp runs as its own kernel in front of every step: the step kernel skips phase WARP
    int warp_lds;   // that kernel gathers through an LDS tile (the default; 0 with DFX_VAR_TVL1_WARP_GATHER)
    int head;       // the warp kernel also runs the head of the loop it starts (k_tvl1_warp_head).  The dual planes of a level's
                    // first warp are zero by definition (A.3): that kernel does not read them and k_tvl1_zero_planes does
                    // not write them
    int geom;       // tile geometry of the default step kernel: bit 0 = tile columns start at x = 0, bit 1 = halo as wide
                    // as the step is long (k_tvl1_step_fused; 0 = classic)
    int n_planes;   // planes of a pair slot: PL_COUNT, or PL_COUNT_GAMMA with the illumination channel (slot_stride = n_planes x
                    // plane_stride).  No kernel reads it (they address through slot_stride): the launchers of the gamma kernels
                    // check it, so that none of them is ever started on a 16-plane slot
};

static inline int dfx_round_up(int v, int m) { return (v + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------------
// Planar output (dfx_calc_batch_planar*): flow i of a launch is a u plane at base + i * flow_stride and a v plane
// plane_stride elements behind it, rows row_pitch elements apart — the [M, 2, H, W] layout of a tensor consumer.  Every
// engine's last writer stores both planes itself (dfx_planar_store*), the bound applied in the same store.  The elements
// are float32, or (dfx_calc_batch_planar_as*) float16 / bfloat16: the float32 value converted once in that store.
enum : int { DFX_ELEM_F32 = 0, DFX_ELEM_F16 = 1, DFX_ELEM_BF16 = 2 }; // = DFX_PLANAR_F32 / _F16 / _BF16 of include/dfx.h
DFX_HD int dfx_elem_bytes(int elem) { return elem == DFX_ELEM_F32 ? 4 : 2; }
struct DfxPlanarOut {
    void *base;                                     // u plane of the launch's first flow
    long long flow_stride, plane_stride, row_pitch; // in elements
    float bound;                                    // 0: raw values; b > 0: clamp(x, -b, b) / b
    int vec;                                        // elements per store that base and all three strides keep aligned: 4, 2 or 1
    int elem;                                       // DFX_ELEM_*: one value per launch, so every branch on it is wave-uniform
};
// 4 elements in one store (16 bytes of float32, 8 bytes of a half type), 2 (8 / 4 bytes), or single elements
static inline int dfx_planar_vec(const void *base, long long flow_stride, long long plane_stride, long long row_pitch,
                                 int elem_bytes = 4) {
    const unsigned long long e = (unsigned long long)elem_bytes;
    const unsigned long long bits = (unsigned long long)(size_t)base | ((unsigned long long)flow_stride * e) |
                                    ((unsigned long long)plane_stride * e) | ((unsigned long long)row_pitch * e);
    return (bits & (4 * e - 1)) == 0 ? 4 : (bits & (2 * e - 1)) == 0 ? 2 : 1;
}
// byte planes (masks, 8-bit images): whether a lane's 4 bytes go in one access — the plane is there, and its base and every
// stride (in bytes; a stride the layout does not have is 0) are multiples of 4
static inline bool dfx_bytes4(const void *base, long long s0, long long s1 = 0, long long s2 = 0) {
    return base && (((unsigned long long)(size_t)base | (unsigned long long)s0 | (unsigned long long)s1 | (unsigned long long)s2) & 3) == 0;
}

// ------------------------------------------------------------------------------------------------
// Caller-supplied initial flows (dfx_calc_batch_init*): one W x H field per pair of a launch, raw pixels, in the caller's
// own layout — interleaved (u, v) rows (step 2, v = u + 1) or two planes (step 1).  Pixel (x, y) of pair i of the launch is
// u[i * pair_stride + y * row_pitch + x * step] and the same element of v.  The engines only ever read it.
struct DfxSeedIn {
    const float *u, *v;               // pixel (0, 0) of the launch's first pair
    int step;                         // floats between neighbouring pixels of a row: 2 or 1
    long long row_pitch, pair_stride; // in floats
};

// ------------------------------------------------------------------------------------------------
// XCD-aware workgroup -> tile mapping (device code only).  MI355X has 8 XCDs with a private 4 MiB L2 each and the
// dispatcher is observed to place workgroup b of a launch on XCD b % 8 (MI355X_MICROARCH.md, "Workgroup dispatch"):
// with the plain blockIdx -> tile mapping the neighbours of a tile — whose halo, box-filter or gather footprint
// overlaps its own — run on seven OTHER XCDs and every L2 fetches the shared rows for itself.  dfx_block_xy() hands
// each XCD one contiguous run of the (x, y) tiles of a grid instead (row-major, bijective for any tile count; grid.z
// = pair / frame is left alone).  A speed choice only: nothing depends on where a workgroup runs.
// Tile index of the workgroup with dispatch index `lin` among `nt`: workgroups lin = k, k + 8, k + 16 ... (XCD k) get the
// contiguous tiles [k*q + min(k, r), ...) with q = nt / 8, r = nt % 8 — a bijection of [0, nt) for every nt (checked on
// the CPU: tests/test_ctrl_logic.py).  Plain C++ so that the test compiles the very function the kernels use.
DFX_HD int dfx_xcd_tile_index(int lin, int nt) {
    const int q = nt >> 3, rem = nt & 7, k = lin & 7;
    return k * q + (k < rem ? k : rem) + (lin >> 3);
}
#if defined(__HIPCC__)
#include <hip/hip_bf16.h>
// Bilinear sample of a strided source at destination pixel (dx, dy): the pyramid resize of both engines (SURVEY.md E.1 —
// no half-pixel centring, upstream's accumulation order; resize_linear_px / resize_linear_px_f with neighbouring pixels
// `step` floats apart and rows `spitch` floats).  The one place the seed kernels of both engines take it from: the order of
// the four rounded multiply-adds is what their bit-exactness rests on.
__device__ __forceinline__ float dfx_seed_resize_px(const float *src, int sw, int sh, long long spitch, int step, int dx, int dy,
                                                    float ifx, float ify) {
    const float sx = (float)dx * ifx;
    const float sy = (float)dy * ify;
    const int x1 = (int)floorf(sx), y1 = (int)floorf(sy);
    const int x2 = x1 + 1, y2 = y1 + 1;
    const int x2r = min(x2, sw - 1), y2r = min(y2, sh - 1);
    const int x1r = min(x1, sw - 1), y1r = min(y1, sh - 1);
    float out = 0.0f;
    out = out + src[(long long)y1r * spitch + (long long)x1r * step] * (((float)x2 - sx) * ((float)y2 - sy));
    out = out + src[(long long)y1r * spitch + (long long)x2r * step] * ((sx - (float)x1) * ((float)y2 - sy));
    out = out + src[(long long)y2r * spitch + (long long)x1r * step] * (((float)x2 - sx) * (sy - (float)y1));
    out = out + src[(long long)y2r * spitch + (long long)x2r * step] * ((sx - (float)x1) * (sy - (float)y1));
    return out;
}
// One value on its way to a plane of DfxPlanarOut.  b == 0: the value itself, the bits the interleaved output holds.
// b > 0: the clamped value through ONE IEEE division (no reciprocal), NaN -> 0: float32 np.clip(x, -b, b) / b.
__device__ __forceinline__ float dfx_planar_value(float x, float b) {
    if (b > 0.0f)
        x = x != x ? 0.0f : __builtin_fminf(__builtin_fmaxf(x, -b), b) / b;
    return x;
}
// The 16 bits a half plane holds for the float32 value y: ONE conversion, round to nearest even — float16 with
// subnormals, +-inf from 65520 on and signed zeros; bfloat16 the rounded upper half of y, a carry may reach inf.  Plain
// casts: the compiler selects the conversion instructions.
__device__ __forceinline__ unsigned short dfx_planar_half_bits(float y, int elem) {
    if (elem == DFX_ELEM_F16) {
        const _Float16 hv = (_Float16)y;
        return __builtin_bit_cast(unsigned short, hv);
    }
    const __hip_bfloat16 bv = __float2bfloat16(y);
    return __builtin_bit_cast(unsigned short, bv);
}
// n = 1..4 values that are already dfx_planar_value()s to elements p .. p + n - 1 of a half plane (p at a multiple of 4
// elements of its row): one 8-byte store, 4-byte stores for aligned pairs, single elements otherwise.
__device__ __forceinline__ void dfx_planar_put_half(unsigned short *p, int vec, int n, const float (&a)[4], int elem) {
    unsigned short q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        q[k] = dfx_planar_half_bits(a[k], elem);
    if (vec == 4 && n == 4) {
        *reinterpret_cast<uint2 *>(p) = make_uint2((unsigned)q[0] | ((unsigned)q[1] << 16), (unsigned)q[2] | ((unsigned)q[3] << 16));
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        if (vec >= 2 && k + 1 < n) {
            *reinterpret_cast<unsigned *>(p + k) = (unsigned)q[k] | ((unsigned)q[k + 1] << 16);
        } else {
            if (k < n)
                p[k] = q[k];
            if (k + 1 < n)
                p[k + 1] = q[k + 1];
        }
    }
}
// Pixels x .. x + n - 1 (x a multiple of 4, n = 1..4) of row y of flow i, u and v each to its plane: one 16-byte store per
// plane where o.vec and n allow, 8-byte stores for aligned pairs, single floats otherwise (odd widths, unaligned pitches);
// the half types the same at half the bytes.
__device__ __forceinline__ void dfx_planar_store4(const DfxPlanarOut &o, int i, int x, int y, int n, const float (&u)[4],
                                                  const float (&v)[4]) {
    const long long at = (long long)i * o.flow_stride + (long long)y * o.row_pitch + x;
    float a[4], c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        a[k] = dfx_planar_value(u[k], o.bound), c[k] = dfx_planar_value(v[k], o.bound);
    if (o.elem != DFX_ELEM_F32) {
        unsigned short *hu = static_cast<unsigned short *>(o.base) + at;
        dfx_planar_put_half(hu, o.vec, n, a, o.elem);
        dfx_planar_put_half(hu + o.plane_stride, o.vec, n, c, o.elem);
        return;
    }
    float *du = static_cast<float *>(o.base) + at;
    float *dv = du + o.plane_stride;
    if (o.vec == 4 && n == 4) {
        *reinterpret_cast<float4 *>(du) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4 *>(dv) = make_float4(c[0], c[1], c[2], c[3]);
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        if (o.vec >= 2 && k + 1 < n) {
            *reinterpret_cast<float2 *>(du + k) = make_float2(a[k], a[k + 1]);
            *reinterpret_cast<float2 *>(dv + k) = make_float2(c[k], c[k + 1]);
        } else {
            if (k < n)
                du[k] = a[k], dv[k] = c[k];
            if (k + 1 < n)
                du[k + 1] = a[k + 1], dv[k + 1] = c[k + 1];
        }
    }
}
// The same for a lane that holds two pixels (x even, n = 1 or 2).
__device__ __forceinline__ void dfx_planar_store2(const DfxPlanarOut &o, int i, int x, int y, int n, float u0, float u1,
                                                  float v0, float v1) {
    const long long at = (long long)i * o.flow_stride + (long long)y * o.row_pitch + x;
    const float a0 = dfx_planar_value(u0, o.bound), a1 = dfx_planar_value(u1, o.bound);
    const float c0 = dfx_planar_value(v0, o.bound), c1 = dfx_planar_value(v1, o.bound);
    if (o.elem != DFX_ELEM_F32) {
        unsigned short *hu = static_cast<unsigned short *>(o.base) + at;
        unsigned short *hv = hu + o.plane_stride;
        const unsigned short p0 = dfx_planar_half_bits(a0, o.elem), p1 = dfx_planar_half_bits(a1, o.elem);
        const unsigned short q0 = dfx_planar_half_bits(c0, o.elem), q1 = dfx_planar_half_bits(c1, o.elem);
        if (o.vec >= 2 && n == 2) {
            *reinterpret_cast<unsigned *>(hu) = (unsigned)p0 | ((unsigned)p1 << 16);
            *reinterpret_cast<unsigned *>(hv) = (unsigned)q0 | ((unsigned)q1 << 16);
            return;
        }
        hu[0] = p0, hv[0] = q0;
        if (n == 2)
            hu[1] = p1, hv[1] = q1;
        return;
    }
    float *du = static_cast<float *>(o.base) + at;
    float *dv = du + o.plane_stride;
    if (o.vec >= 2 && n == 2) {
        *reinterpret_cast<float2 *>(du) = make_float2(a0, a1);
        *reinterpret_cast<float2 *>(dv) = make_float2(c0, c1);
        return;
    }
    du[0] = a0, dv[0] = c0;
    if (n == 2)
        du[1] = a1, dv[1] = c1;
}
// (the merge kernels' planar form, dfx_planar_merge_tile / dfx_planar_merge_grid, is in flow_quad.h with the lane quad it uses)
#ifndef DFX_XCD_REMAP
#define DFX_XCD_REMAP 1 // 0: plain blockIdx (A/B builds, scripts/build_variant.sh)
#endif
struct DfxBlockXY {
    int x, y;
};
__device__ __forceinline__ DfxBlockXY dfx_block_xy() {
    DfxBlockXY r;
    r.x = (int)blockIdx.x;
    r.y = (int)blockIdx.y;
#if DFX_XCD_REMAP
    const int gx = (int)gridDim.x;
    const int t = dfx_xcd_tile_index(r.y * gx + r.x, gx * (int)gridDim.y);
    r.y = t / gx;
    r.x = t - r.y * gx;
#endif
    return r;
}
// the same for a grid whose x dimension already is a linear tile index
__device__ __forceinline__ int dfx_block_linear() {
#if DFX_XCD_REMAP
    return dfx_xcd_tile_index((int)blockIdx.x, (int)gridDim.x);
#else
    return (int)blockIdx.x;
#endif
}
#endif

