// plane_warp_kernels.hip — the backward warp of float32 / float16 / bfloat16 planes, and of opaque 1-, 2- or 4-byte elements
// (label maps), by a flow: what a holder of a flow does with the labels, a depth plane, a soft mask or a feature map of frame 1
// to see them at the pixels of frame 0.  The sibling of warp_kernels.hip, for any channel count and both layouts.
//
// Image i is sampled at the positions flow i names.  Output pixel (x, y) with flow (fu, fv), all in float32, every operation
// rounded on its own (the build's -ffp-contract=off):
//     px = (float)x + fu;  py = (float)y + fv
//     inside, take, the clamp and x0 x1 y0 y1 ax ay: fq_tap of flow_quad.h (dfx_warp_device's position)
//     valid = inside && (no occlusion mask || occ[y][x] == 0)
//     bilinear: every tap converted exactly to float32, per channel s = fq_lerp(p00, p01, p10, p11, ax, ay), stored as float32
//               or through dfx_planar_half_bits
//     nearest : xn = (int)rintf(px), yn = (int)rintf(py) after the same test and clamp (fq_nearest); the element is copied as
//               a bit pattern
//     INVALID_ZERO: every pixel is written, one without take as all-zero bits;  INVALID_KEEP: only pixels with valid are
// tests/plane_warp_ref.py is the same text in NumPy; the two agree bit for bit (a bilinear NaN: in NaN-ness).
//
// Two kernels, because the two layouts want opposite lane mappings.
// k_pw_planar: the lane quad of flow_quad.h.  Flow, mask and tap are worked out once per pixel; a lane keeps two weights and
// four byte offsets inside a plane per pixel (one offset for nearest) across the channel loop, which advances one
// wave-uniform plane base per channel: a tap's address is that scalar base plus a 32-bit lane offset.  BIG: a plane that
// spans 4 GiB or more keeps 64-bit offsets instead.  Each iteration gathers 4 taps x 4 pixels and stores one quad.
// k_pw_interleaved: lanes run over (pixel, group of E = 16 / element bytes channels); the lanes of a pixel read neighbouring
// 16 bytes of the same tap and write neighbouring bytes of out, and all read that pixel's flow (one address, one fetch).
// Where the channel count is no multiple of E or a base or stride breaks the 16-byte alignment, the same lanes move their
// E channels one element at a time: the same bits.
// Bytes per pixel: 8 of flow, C x elem x (1 .. 4) of taps (perfectly cached .. every tap its own sector), C x elem of out,
// + 1 of occ, + 1 of valid where asked for.  No LDS, no scratch.
#include "plane_warp_kernels.h"

#include <algorithm>
#include <type_traits>

#include "dfx_device.h"
#include "flow_quad.h"

static_assert(PW_ELEM_U8 == FQ_ELEM_U8 && PW_BORDER_ZERO == FQ_BORDER_ZERO && PW_BORDER_CLAMP == FQ_BORDER_CLAMP, "flow_quad.h");

namespace {

// what is one value per launch, so that every branch on it is wave-uniform
struct PwWide {
    int flow, occ, valid, out; // planar: which accesses take a lane's 4 elements at once
    int il;                    // interleaved: 16-byte taps and whole-group stores
    int epl, groups, g0;       // interleaved: channels per lane, groups per pixel in this launch, first group of the launch
};

// SRC of a form: bilinear, the DFX_ELEM_* code of the source; nearest, the bytes of an element
template <int SAMPLE, int SRC>
constexpr int pw_src_bytes() { return SAMPLE == PW_SAMPLE_NEAREST ? SRC : (SRC == DFX_ELEM_F32 ? 4 : 2); }

template <int B>
__device__ __forceinline__ unsigned pw_load_bits(const char *p) {
    if constexpr (B == 4)
        return *reinterpret_cast<const unsigned *>(p);
    else if constexpr (B == 2)
        return *reinterpret_cast<const unsigned short *>(p);
    else
        return *reinterpret_cast<const unsigned char *>(p);
}
template <int B>
__device__ __forceinline__ void pw_store_bits(char *p, unsigned q) {
    if constexpr (B == 4)
        *reinterpret_cast<unsigned *>(p) = q;
    else if constexpr (B == 2)
        *reinterpret_cast<unsigned short *>(p) = (unsigned short)q;
    else
        *reinterpret_cast<unsigned char *>(p) = (unsigned char)q;
}
// the stored bits of a float32 sample: itself, or the typed planes' one conversion
__device__ __forceinline__ unsigned pw_out_bits(float s, int out_dtype) {
    return out_dtype == DFX_ELEM_F32 ? __builtin_bit_cast(unsigned, s) : (unsigned)dfx_planar_half_bits(s, out_dtype);
}

// A wave-uniform pointer as the scalar registers hold it.  Opaque to the loop optimiser: without it the channel loop's tap
// addresses become sixteen 64-bit vector induction variables and the kernel spills; with it a tap is one load at
// (scalar base) + (32-bit lane offset).
template <class T>
__device__ __forceinline__ T *pw_uniform(T *p) {
    unsigned long long v = (unsigned long long)p;
    asm volatile("" : "+s"(v)); // no instruction: the value passes through a scalar register pair
    // said to be global memory, which an integer does not say by itself: global, not flat, loads and stores
    return (T *)(__attribute__((address_space(1))) T *)v;
}

// A 32-bit lane offset on its way into an address inside the channel loop.  Opaque as well: otherwise the offsets are widened
// to 64 bits once in front of the loop and held as register pairs (32 registers for the sixteen taps).
template <class Off>
__device__ __forceinline__ Off pw_lane(Off o) {
    if constexpr (sizeof(Off) == 4)
        asm volatile("" : "+v"(o));
    return o;
}

// A quad of B-byte elements to p .. p + 4 B - 1.  KEEP: only the elements whose bit of okm is set; a quad that holds one that is
// not stores the others singly.
template <int B, bool KEEP>
__device__ __forceinline__ void pw_store_quad(char *p, bool wide, int n, const unsigned (&q)[4], unsigned okm) {
    bool all = n == 4;
    if (KEEP)
        all = all && okm == 15u;
    if (wide && all) {
        if constexpr (B == 4)
            *reinterpret_cast<uint4 *>(p) = make_uint4(q[0], q[1], q[2], q[3]);
        else if constexpr (B == 2)
            *reinterpret_cast<uint2 *>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
        else
            *reinterpret_cast<unsigned *>(p) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    } else {
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (k < n && (!KEEP || (okm >> k & 1u)))
                pw_store_bits<B>(p + k * B, q[k]);
    }
}

// ------------------------------------------------------------------------------------------------
// Planar.  What a lane keeps of its 4 pixels (x .. x + 3, y) across the channel loop: per pixel the byte offsets of its taps
// inside a plane (one for nearest), the two weights and take; the byte offset of its quad inside a plane of out.
template <int SAMPLE, bool BIG>
struct PwQuad {
    using Off = std::conditional_t<BIG, long long, unsigned>;
    static constexpr int TAPS = SAMPLE == PW_SAMPLE_NEAREST ? 1 : 4;
    Off o[4][TAPS], oo;
    float ax[4], ay[4];
    bool tk[4];
};
// sb, ob: bytes of an element of the source and of out
template <int SAMPLE, bool BIG>
__device__ __forceinline__ void pw_quad_taps(const PwArgs &a, int x, int y, const float (&u)[4], const float (&v)[4], int sb, int ob,
                                             PwQuad<SAMPLE, BIG> &qd) {
    using Off = typename PwQuad<SAMPLE, BIG>::Off;
    const Off pitchb = (Off)(a.src_pitch * sb);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // a pixel past the row's end has flow 0: in range under either border, loaded and never stored
        const float px = (float)(x + k) + u[k], py = (float)y + v[k];
        if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
            const FqNear t = fq_nearest(px, py, a.w, a.h, a.border);
            qd.tk[k] = t.take;
            qd.o[k][0] = (Off)t.yn * pitchb + (Off)(t.xn * sb);
            qd.ax[k] = qd.ay[k] = 0.0f;
        } else {
            const FqTap t = fq_tap(px, py, a.w, a.h, a.border);
            qd.tk[k] = t.take;
            const Off r0 = (Off)t.y0 * pitchb, r1 = (Off)t.y1 * pitchb;
            const Off c0 = (Off)(t.x0 * sb), c1 = (Off)(t.x1 * sb);
            qd.o[k][0] = r0 + c0, qd.o[k][1] = r0 + c1, qd.o[k][2] = r1 + c0, qd.o[k][3] = r1 + c1;
            qd.ax[k] = t.ax, qd.ay[k] = t.ay;
        }
    }
    qd.oo = (Off)(((long long)y * a.out_pitch + x) * ob);
}

// The channel loop of the lane's quad in image i.
template <int SAMPLE, bool KEEP, bool BIG, int SRC>
__device__ __forceinline__ void pw_planar_channels(const PwArgs &a, const PwWide &wide, long long i, int n,
                                                   const PwQuad<SAMPLE, BIG> &qd, unsigned okm) {
    constexpr int SB = pw_src_bytes<SAMPLE, SRC>();
    const auto &o = qd.o;
    const auto &ax = qd.ax, &ay = qd.ay;
    const auto &tk = qd.tk;
    const auto oo = qd.oo;
    const int od = a.out_dtype;
    const int ob = SAMPLE == PW_SAMPLE_NEAREST ? SB : dfx_elem_bytes(od);
    // one wave-uniform base per channel for the source and for out: the loop's only address arithmetic is two scalar adds
    const char *sp = static_cast<const char *>(a.src) + i * a.src_image * SB;
    char *op = static_cast<char *>(a.out) + i * a.out_image * ob;
    const long long sstep = a.src_plane * SB, ostep = a.out_plane * ob;
    const bool wout = wide.out != 0;
#pragma unroll 1
    for (int c = 0; c < a.channels; ++c) {
        const char *const spc = pw_uniform(sp);
        char *const opc = pw_uniform(op);
        unsigned q[4];
        if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned e = pw_load_bits<SB>(spc + pw_lane(o[k][0]));
                q[k] = (KEEP || tk[k]) ? e : 0u; // KEEP stores valid pixels only, and those are taken
            }
            pw_store_quad<SB, KEEP>(opc + pw_lane(oo), wout, n, q, okm);
        } else {
            float s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                s[k] = fq_lerp(fq_load_elem<SRC>(spc + pw_lane(o[k][0]), 0), fq_load_elem<SRC>(spc + pw_lane(o[k][1]), 0),
                               fq_load_elem<SRC>(spc + pw_lane(o[k][2]), 0), fq_load_elem<SRC>(spc + pw_lane(o[k][3]), 0), ax[k], ay[k]);
            if (od == DFX_ELEM_F32) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[k] = (KEEP || tk[k]) ? __builtin_bit_cast(unsigned, s[k]) : 0u;
                pw_store_quad<4, KEEP>(opc + pw_lane(oo), wout, n, q, okm);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    q[k] = (KEEP || tk[k]) ? (unsigned)dfx_planar_half_bits(s[k], od) : 0u;
                pw_store_quad<2, KEEP>(opc + pw_lane(oo), wout, n, q, okm);
            }
        }
        sp += sstep, op += ostep;
    }
}

// SAMPLE: PW_SAMPLE_*; KEEP: PW_INVALID_KEEP; BIG: a plane of the source or of out spans 4 GiB or more, 64-bit lane offsets.
// grid: fq_grid(w, h, images).  Eight waves per SIMD (64 registers) for the 32-bit forms: the taps bind, as in k_warp.  The
// BIG forms hold twice the offset registers (up to 32 for the four pixels' taps) and are given four waves per SIMD (128).
template <int SAMPLE, bool KEEP, bool BIG>
__global__ __launch_bounds__(256, BIG ? 4 : 8) void k_pw_planar(PwArgs a, PwWide wide) {
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long i = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    float u[4], v[4];
    fq_load_flow(a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x, a.plane_stride, wide.flow != 0, n, u, v);
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const FqTap t = fq_tap((float)(x + k) + u[k], (float)y + v[k], a.w, a.h, a.border);
        ok[k] = (k < n && t.inside) ? 1u : 0u;
    }
    if (a.occ)
        fq_mask_clear(a.occ + i * a.occ_stride + (long long)y * a.occ_pitch + x, wide.occ != 0, n, ok);
    if (a.valid)
        fq_store_u8(a.valid + i * a.valid_stride + (long long)y * a.valid_pitch + x, wide.valid != 0, n, ok);
    if (!a.out)
        return;
    const unsigned okm = ok[0] | (ok[1] << 1) | (ok[2] << 2) | (ok[3] << 3);
    if (KEEP && !okm)
        return;
    const int sd = a.src_dtype;
    const int sb = sd == PW_ELEM_U8 ? 1 : dfx_elem_bytes(sd);
    PwQuad<SAMPLE, BIG> qd;
    pw_quad_taps<SAMPLE, BIG>(a, x, y, u, v, sb, SAMPLE == PW_SAMPLE_NEAREST ? sb : dfx_elem_bytes(a.out_dtype), qd);
    if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
        if (sd == DFX_ELEM_F32)
            pw_planar_channels<SAMPLE, KEEP, BIG, 4>(a, wide, i, n, qd, okm);
        else if (sd == PW_ELEM_U8)
            pw_planar_channels<SAMPLE, KEEP, BIG, 1>(a, wide, i, n, qd, okm);
        else
            pw_planar_channels<SAMPLE, KEEP, BIG, 2>(a, wide, i, n, qd, okm);
    } else {
        if (sd == DFX_ELEM_F32)
            pw_planar_channels<SAMPLE, KEEP, BIG, DFX_ELEM_F32>(a, wide, i, n, qd, okm);
        else if (sd == DFX_ELEM_F16)
            pw_planar_channels<SAMPLE, KEEP, BIG, DFX_ELEM_F16>(a, wide, i, n, qd, okm);
        else
            pw_planar_channels<SAMPLE, KEEP, BIG, DFX_ELEM_BF16>(a, wide, i, n, qd, okm);
    }
}

// ------------------------------------------------------------------------------------------------
// Interleaved.  The E = 16 / SB channels g * E .. of pixel (x, y): src at the image's first element, out at the pixel's.
template <int SAMPLE, int SRC>
__device__ __forceinline__ void pw_il_group(const PwArgs &a, bool wide, const char *src, char *out, int g, bool take, const FqTap &t,
                                            const FqNear &tn) {
    constexpr int SB = pw_src_bytes<SAMPLE, SRC>();
    constexpr int E = 16 / SB;
    const long long rowb = a.src_pitch * SB, pixb = (long long)a.channels * SB, cb = (long long)g * 16;
    const int od = a.out_dtype;
    if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
        const char *p = src + tn.yn * rowb + tn.xn * pixb + cb;
        if (wide) {
            uint4 e = make_uint4(0u, 0u, 0u, 0u);
            if (take)
                e = *reinterpret_cast<const uint4 *>(p);
            *reinterpret_cast<uint4 *>(out) = e;
        } else {
            const int m = min(E, a.channels - g * E);
            for (int k = 0; k < m; ++k)
                pw_store_bits<SB>(out + k * SB, take ? pw_load_bits<SB>(p + k * SB) : 0u);
        }
    } else {
        const int ob = dfx_elem_bytes(od);
        const char *r0 = src + t.y0 * rowb + cb, *r1 = src + t.y1 * rowb + cb;
        const char *p00 = r0 + t.x0 * pixb, *p01 = r0 + t.x1 * pixb, *p10 = r1 + t.x0 * pixb, *p11 = r1 + t.x1 * pixb;
        if (wide) {
            unsigned q[E];
#pragma unroll
            for (int k = 0; k < E; ++k)
                q[k] = 0u;
            if (take) {
                // four 16-byte taps, E exact conversions each
                const uint4 e00 = *reinterpret_cast<const uint4 *>(p00), e01 = *reinterpret_cast<const uint4 *>(p01);
                const uint4 e10 = *reinterpret_cast<const uint4 *>(p10), e11 = *reinterpret_cast<const uint4 *>(p11);
                const unsigned w00[4] = {e00.x, e00.y, e00.z, e00.w}, w01[4] = {e01.x, e01.y, e01.z, e01.w};
                const unsigned w10[4] = {e10.x, e10.y, e10.z, e10.w}, w11[4] = {e11.x, e11.y, e11.z, e11.w};
#pragma unroll
                for (int k = 0; k < E; ++k) {
                    float f00, f01, f10, f11;
                    if constexpr (SRC == DFX_ELEM_F32) {
                        f00 = __builtin_bit_cast(float, w00[k]), f01 = __builtin_bit_cast(float, w01[k]);
                        f10 = __builtin_bit_cast(float, w10[k]), f11 = __builtin_bit_cast(float, w11[k]);
                    } else {
                        const int sh = 16 * (k & 1);
                        const unsigned short h00 = (unsigned short)(w00[k >> 1] >> sh), h01 = (unsigned short)(w01[k >> 1] >> sh);
                        const unsigned short h10 = (unsigned short)(w10[k >> 1] >> sh), h11 = (unsigned short)(w11[k >> 1] >> sh);
                        if constexpr (SRC == DFX_ELEM_F16) {
                            f00 = fq_f16_to_f32(h00), f01 = fq_f16_to_f32(h01), f10 = fq_f16_to_f32(h10), f11 = fq_f16_to_f32(h11);
                        } else {
                            f00 = fq_bf16_to_f32(h00), f01 = fq_bf16_to_f32(h01), f10 = fq_bf16_to_f32(h10), f11 = fq_bf16_to_f32(h11);
                        }
                    }
                    q[k] = pw_out_bits(fq_lerp(f00, f01, f10, f11, t.ax, t.ay), od);
                }
            }
            if (ob == 4) {
#pragma unroll
                for (int k = 0; k < E; k += 4)
                    *reinterpret_cast<uint4 *>(out + 4 * k) = make_uint4(q[k], q[k + 1], q[k + 2], q[k + 3]);
            } else if constexpr (E == 8) {
                *reinterpret_cast<uint4 *>(out) = make_uint4(q[0] | (q[1] << 16), q[2] | (q[3] << 16), q[4] | (q[5] << 16), q[6] | (q[7] << 16));
            } else {
                *reinterpret_cast<uint2 *>(out) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
            }
        } else {
            const int m = min(E, a.channels - g * E);
            for (int k = 0; k < m; ++k) {
                unsigned q = 0u;
                if (take)
                    q = pw_out_bits(fq_lerp(fq_load_elem<SRC>(p00, k), fq_load_elem<SRC>(p01, k), fq_load_elem<SRC>(p10, k),
                                            fq_load_elem<SRC>(p11, k), t.ax, t.ay), od);
                if (ob == 4)
                    pw_store_bits<4>(out + 4 * k, q);
                else
                    pw_store_bits<2>(out + 2 * k, q);
            }
        }
    }
}

// grid: (ceil(w * groups / 256), min(h, DFX_GRID_YZ_MAX), images): a lane is (pixel x, group g0 + g) of the rows blockIdx.y,
// blockIdx.y + gridDim.y, ..  w * groups < 2^31 (the launcher splits the groups of wider pixels over launches).
template <int SAMPLE, bool KEEP>
__global__ __launch_bounds__(256, 8) void k_pw_interleaved(PwArgs a, PwWide wide) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= (unsigned)a.w * (unsigned)wide.groups)
        return;
    const int x = (int)(t / (unsigned)wide.groups), g = wide.g0 + (int)(t - (unsigned)x * (unsigned)wide.groups);
    const long long i = (long long)blockIdx.z;
    const int sd = a.src_dtype, E = wide.epl;
    const int ob = SAMPLE == PW_SAMPLE_NEAREST ? 16 / E : dfx_elem_bytes(a.out_dtype);
    for (int y = (int)blockIdx.y; y < a.h; y += (int)gridDim.y) {
        const float *fu = a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x;
        const float px = (float)x + fu[0], py = (float)y + fu[a.plane_stride];
        FqTap tb{};
        FqNear tn{};
        bool inside, take;
        if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
            tn = fq_nearest(px, py, a.w, a.h, a.border);
            inside = tn.inside, take = tn.take;
        } else {
            tb = fq_tap(px, py, a.w, a.h, a.border);
            inside = tb.inside, take = tb.take;
        }
        bool ok = inside;
        if (a.occ)
            ok = ok && a.occ[i * a.occ_stride + (long long)y * a.occ_pitch + x] == 0;
        if (a.valid && g == 0)
            a.valid[i * a.valid_stride + (long long)y * a.valid_pitch + x] = ok ? 1 : 0;
        if (!a.out || (KEEP && !ok))
            continue;
        const char *src = static_cast<const char *>(a.src) + i * a.src_image * (16 / E);
        char *out = static_cast<char *>(a.out) + (i * a.out_image + (long long)y * a.out_pitch + (long long)x * a.channels + (long long)g * E) * ob;
        const bool w16 = wide.il != 0;
        if constexpr (SAMPLE == PW_SAMPLE_NEAREST) {
            if (sd == DFX_ELEM_F32)
                pw_il_group<SAMPLE, 4>(a, w16, src, out, g, take, tb, tn);
            else if (sd == PW_ELEM_U8)
                pw_il_group<SAMPLE, 1>(a, w16, src, out, g, take, tb, tn);
            else
                pw_il_group<SAMPLE, 2>(a, w16, src, out, g, take, tb, tn);
        } else {
            if (sd == DFX_ELEM_F32)
                pw_il_group<SAMPLE, DFX_ELEM_F32>(a, w16, src, out, g, take, tb, tn);
            else if (sd == DFX_ELEM_F16)
                pw_il_group<SAMPLE, DFX_ELEM_F16>(a, w16, src, out, g, take, tb, tn);
            else
                pw_il_group<SAMPLE, DFX_ELEM_BF16>(a, w16, src, out, g, take, tb, tn);
        }
    }
}

template <int SAMPLE, bool KEEP>
void pw_launch_as(hipStream_t s, const PwArgs &a, const PwWide &wide, bool big) {
    if (!a.planar) {
        const dim3 grid((unsigned)(((long long)a.w * wide.groups + 255) / 256), (unsigned)std::min(a.h, DFX_GRID_YZ_MAX), (unsigned)a.n);
        hipLaunchKernelGGL((k_pw_interleaved<SAMPLE, KEEP>), grid, dim3(256), 0, s, a, wide);
    } else if (big) {
        hipLaunchKernelGGL((k_pw_planar<SAMPLE, KEEP, true>), fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
    } else {
        hipLaunchKernelGGL((k_pw_planar<SAMPLE, KEEP, false>), fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
    }
}

inline int pw_bytes(int dtype) { return dtype == PW_ELEM_U8 ? 1 : dfx_elem_bytes(dtype); }
// whether base and every stride (in elements of eb bytes) are multiples of `align` bytes
inline bool pw_aligned(const void *base, int eb, long long align, long long s0, long long s1, long long s2 = 0) {
    const unsigned long long e = (unsigned long long)eb;
    const unsigned long long bits = (unsigned long long)(size_t)base | ((unsigned long long)s0 * e) | ((unsigned long long)s1 * e) |
                                    ((unsigned long long)s2 * e);
    return (bits & (unsigned long long)(align - 1)) == 0;
}

} // namespace

void pw_launch(hipStream_t s, const PwArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0 || args.channels <= 0)
        return;
    const int sb = pw_bytes(args.src_dtype), ob = args.sample == PW_SAMPLE_NEAREST ? sb : pw_bytes(args.out_dtype);
    const bool planes = args.planar != 0 && args.channels > 1;
    PwWide wide{};
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.occ = dfx_bytes4(args.occ, args.occ_pitch, args.occ_stride, 0);
    wide.valid = dfx_bytes4(args.valid, args.valid_pitch, args.valid_stride, 0);
    wide.out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, ob) == 4;
    // interleaved: E channels per lane; 16-byte taps and whole-group stores where the channels are whole groups and both
    // buffers keep the accesses' alignment (out's access is min(16, E * ob) bytes)
    const int E = 16 / sb;
    const long long groups = ((long long)args.channels + E - 1) / E;
    wide.epl = E;
    wide.il = args.channels % E == 0 && pw_aligned(args.src, sb, 16, args.src_pitch, args.src_image, args.channels) &&
              (!args.out || pw_aligned(args.out, ob, std::min(16, E * ob), args.out_pitch, args.out_image, args.channels));
    // planar: 32-bit lane offsets while a plane of the source and of out spans less than 4 GiB
    const unsigned long long span_s = ((unsigned long long)(args.h - 1) * (unsigned long long)args.src_pitch + (unsigned long long)args.w) * sb;
    const unsigned long long span_o = args.out ? ((unsigned long long)(args.h - 1) * (unsigned long long)args.out_pitch + (unsigned long long)args.w) * ob : 0;
    const bool big = span_s >= (1ull << 32) || span_o >= (1ull << 32);
    // grid.z holds at most FQ_ITEMS_MAX = 65535 images: more than that go in several launches; an interleaved launch holds
    // at most 2^31 - 1 lanes per row: wider pixels go group range by group range
    const long long gmax = args.planar ? groups : std::max(1LL, 0x7fffffffLL / args.w);
    const int chunk = FQ_ITEMS_MAX;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        PwArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.src = static_cast<const char *>(args.src) + (long long)i0 * args.src_image * sb;
        a.flow += (long long)i0 * args.flow_stride;
        if (a.out)
            a.out = static_cast<char *>(args.out) + (long long)i0 * args.out_image * ob;
        if (a.occ)
            a.occ += (long long)i0 * args.occ_stride;
        if (a.valid)
            a.valid += (long long)i0 * args.valid_stride;
        for (long long g0 = 0; g0 < groups; g0 += gmax) {
            wide.g0 = (int)g0, wide.groups = (int)std::min(gmax, groups - g0);
            if (args.sample == PW_SAMPLE_NEAREST)
                args.keep ? pw_launch_as<PW_SAMPLE_NEAREST, true>(s, a, wide, big) : pw_launch_as<PW_SAMPLE_NEAREST, false>(s, a, wide, big);
            else
                args.keep ? pw_launch_as<PW_SAMPLE_BILINEAR, true>(s, a, wide, big) : pw_launch_as<PW_SAMPLE_BILINEAR, false>(s, a, wide, big);
        }
    }
}
