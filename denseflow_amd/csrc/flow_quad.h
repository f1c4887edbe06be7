// flow_quad.h — the one idiom of the flow post-processing kernels (fb_check, warp, flow_chain, global_motion, flow_project,
// flow_median, interpolate, flow_colour) and of the engines' planar merge kernels.
//
// The lane quad.  A lane owns 4 neighbouring pixels x .. x + 3 of one row (x a multiple of 4), a wave 1 KB of that row per
// float plane, a workgroup of 256 threads 256 pixels of `rows` rows, wave w the rows w, w + 4, ..; grid.z is the image.  The
// last lane of a row holds n = min(4, W - x) pixels.  Every access of a quad takes (pointer to its first element, wide, n):
// one 4- / 8- / 16-byte access where `wide` — one value per launch and buffer, decided on the host by dfx_planar_vec /
// dfx_bytes4 from the base and every stride, so a branch on it is wave-uniform — and n == 4 allow it, single elements
// otherwise.  A load gives 0 for the elements past the row's end; a store leaves them alone.
//
// The bilinear tap.  fq_tap is the one statement of "where does a position sample an image": the range test on the floats
// before any conversion to int (false for NaN and either infinity), the two border modes, floor, x1 / y1 clamped to the last
// column / row (x0 / y0 never need it).  fq_lerp is the one three-step interpolation.  Both are plain C++, float32, every
// operation rounded on its own (the build's -ffp-contract=off): tests/flow_quad_harness.cpp compiles this very text on the CPU
// and tests/test_flow_quad_cpu.py holds it bit for bit against the NumPy references the kernels are tested with.
#pragma once

#include "dfx_device.h"

enum : int { FQ_BORDER_ZERO = 0, FQ_BORDER_CLAMP = 1 }; // = DFX_WARP_BORDER_* of include/dfx.h
enum : int { FQ_ELEM_U8 = 3 };                          // = DFX_WARP_U8; 0 .. 2 are DFX_ELEM_F32 / _F16 / _BF16

// ------------------------------------------------------------------------------------------------
// The bilinear tap of position (px, py) in a W x H image.
//     inside = px >= 0 && py >= 0 && px <= W-1 && py <= H-1
//     FQ_BORDER_ZERO : take = inside
//     FQ_BORDER_CLAMP: take = px, py both not NaN;  px = min(max(px, 0), W-1), py likewise (infinities clamp)
//     take: x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
// Without take the position itself never reaches floor or a cast: the fields are those of position (0, 0), in range, and the
// caller does not sample.
struct FqTap {
    bool inside, take;
    int x0, x1, y0, y1;
    float ax, ay;
};
DFX_HD FqTap fq_tap(float px, float py, int w, int h, int border) {
    const float wmax = (float)(w - 1), hmax = (float)(h - 1);
    FqTap t;
    // the range test comes before any conversion to int: false for NaN and for either infinity
    t.inside = px >= 0.0f && py >= 0.0f && px <= wmax && py <= hmax;
    t.take = t.inside;
    if (border == FQ_BORDER_CLAMP) {
        t.take = px == px && py == py;
        px = __builtin_fminf(__builtin_fmaxf(px, 0.0f), wmax);
        py = __builtin_fminf(__builtin_fmaxf(py, 0.0f), hmax);
    }
    // a position that is not sampled is (0, 0) before floor and the cast see it (as in the NumPy references): no branch here,
    // and the fields are in range either way
    px = t.take ? px : 0.0f;
    py = t.take ? py : 0.0f;
    const float fx = __builtin_floorf(px), fy = __builtin_floorf(py);
    t.x0 = (int)fx, t.y0 = (int)fy;
    t.ax = px - fx, t.ay = py - fy;
    t.x1 = t.x0 + 1 < w - 1 ? t.x0 + 1 : w - 1;
    t.y1 = t.y0 + 1 < h - 1 ? t.y0 + 1 : h - 1;
    return t;
}

// the bilinear value of four taps: p00 p01 on row y0, p10 p11 on row y1.  Nothing is shortcut: 0 * (inf - x) is NaN.
DFX_HD float fq_lerp(float p00, float p01, float p10, float p11, float ax, float ay) {
    const float t = p00 + ax * (p01 - p00);
    const float b = p10 + ax * (p11 - p10);
    return t + ay * (b - t);
}

// the sample of a float plane at a taken tap (pitch: elements between rows)
DFX_HD float fq_sample_f32(const float *p, long long pitch, const FqTap &t) {
    const float *r0 = p + (long long)t.y0 * pitch, *r1 = p + (long long)t.y1 * pitch;
    return fq_lerp(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.ax, t.ay);
}

// the samples of the C channels of an 8-bit image at a taken tap, P = (float)byte.  IL: the channels of a pixel lie next to
// each other (C bytes per pixel); otherwise in planes `plane` bytes apart.  pitch: bytes between rows.
template <int C, bool IL>
DFX_HD void fq_sample_u8(const unsigned char *img, long long pitch, long long plane, const FqTap &t, float (&s)[C]) {
    constexpr int XS = IL ? C : 1;
    const long long cs = IL ? 1 : plane; // bytes between the channels of a tap
    const unsigned char *r0 = img + (long long)t.y0 * pitch, *r1 = img + (long long)t.y1 * pitch;
    const int o0 = t.x0 * XS, o1 = t.x1 * XS;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < C; ++c) {
        const long long co = C == 1 ? 0 : c * cs;
        s[c] = fq_lerp((float)r0[o0 + co], (float)r0[o1 + co], (float)r1[o0 + co], (float)r1[o1 + co], t.ax, t.ay);
    }
}

// ------------------------------------------------------------------------------------------------
// Segments.  A lane's 4 pixels of C channels are C "segments" of 4 consecutive elements in memory: plane g (gray, planar), or
// elements 4 g .. 4 g + 3 of its 4 C interleaved ones.  Element e of segment g is channel fq_seg_channel of pixel fq_seg_pixel.
template <int C, bool IL>
DFX_HD constexpr int fq_seg_pixel(int g, int e) { return IL ? (4 * g + e) / C : e; }
template <int C, bool IL>
DFX_HD constexpr int fq_seg_channel(int g, int e) { return IL ? (4 * g + e) % C : g; }
// elements of segment g inside the row, of a lane with n pixels: 0 .. 4
template <int C, bool IL>
DFX_HD int fq_seg_count(int g, int n) {
    const int m = C * n - 4 * g;
    return IL ? (m < 0 ? 0 : (m > 4 ? 4 : m)) : n;
}
// element offset of segment g of the lane at x from the row's start in plane 0 (plane: elements between planes)
template <int C, bool IL>
DFX_HD long long fq_seg_offset(int x, int g, long long plane) { return IL ? (long long)(x * C + 4 * g) : g * plane + x; }
// segment g of per-pixel, per-channel values
template <int C, bool IL, typename T>
DFX_HD void fq_segment(const T (&s)[4][C], int g, T (&seg)[4]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e < 4; ++e)
        seg[e] = s[fq_seg_pixel<C, IL>(g, e)][fq_seg_channel<C, IL>(g, e)];
}

// ------------------------------------------------------------------------------------------------
// Typed planes (plane_warp_kernels.hip): the nearest position, the exact half -> float conversions, a typed tap load.
// The nearest pixel of position (px, py): the range test, take and the clamp of fq_tap, word for word, then rintf (ties to
// even) of each coordinate.  A taken position lies in [0, W-1] x [0, H-1] before it is rounded, so xn, yn are in range; one
// that is not taken is (0, 0), as in fq_tap.
struct FqNear {
    bool inside, take;
    int xn, yn;
};
DFX_HD FqNear fq_nearest(float px, float py, int w, int h, int border) {
    const float wmax = (float)(w - 1), hmax = (float)(h - 1);
    FqNear t;
    t.inside = px >= 0.0f && py >= 0.0f && px <= wmax && py <= hmax;
    t.take = t.inside;
    if (border == FQ_BORDER_CLAMP) {
        t.take = px == px && py == py;
        px = __builtin_fminf(__builtin_fmaxf(px, 0.0f), wmax);
        py = __builtin_fminf(__builtin_fmaxf(py, 0.0f), hmax);
    }
    px = t.take ? px : 0.0f;
    py = t.take ? py : 0.0f;
    t.xn = (int)__builtin_rintf(px), t.yn = (int)__builtin_rintf(py);
    return t;
}

// float16 bits as float32, exactly: subnormals are kept (value = mantissa * 2^-24), infinities and NaNs keep their sign and
// the payload in the upper mantissa bits.  On the device it is the compiler's conversion; the integer form is what a host
// compiler without a 16-bit float type builds, and the two agree on all 65536 patterns.
DFX_HD float fq_f16_to_f32(unsigned short b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, b);
#else
    const unsigned sign = ((unsigned)b & 0x8000u) << 16, e = ((unsigned)b >> 10) & 0x1fu, m = (unsigned)b & 0x3ffu;
    unsigned bits;
    if (e == 0x1fu)
        bits = sign | 0x7f800000u | (m << 13);
    else if (e != 0u)
        bits = sign | ((e + 112u) << 23) | (m << 13);
    else { // zero or a subnormal: m * 2^-24 is exact in float32
        const float v = (float)m * 5.9604644775390625e-08f;
        return sign ? -v : v;
    }
    return __builtin_bit_cast(float, bits);
#endif
}
// bfloat16 bits as float32: the upper half
DFX_HD float fq_bf16_to_f32(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }

// element `at` of a plane of dtype DFX_ELEM_F32 / _F16 / _BF16 as float32, exactly
template <int ELEM>
DFX_HD float fq_load_elem(const void *p, long long at) {
    if constexpr (ELEM == DFX_ELEM_F32)
        return static_cast<const float *>(p)[at];
    else if constexpr (ELEM == DFX_ELEM_F16)
        return fq_f16_to_f32(static_cast<const unsigned short *>(p)[at]);
    else
        return fq_bf16_to_f32(static_cast<const unsigned short *>(p)[at]);
}
// the bilinear sample of a typed plane at a taken tap (pitch: elements between rows)
template <int ELEM>
DFX_HD float fq_sample_elem(const void *p, long long pitch, const FqTap &t) {
    const long long r0 = (long long)t.y0 * pitch, r1 = (long long)t.y1 * pitch;
    return fq_lerp(fq_load_elem<ELEM>(p, r0 + t.x0), fq_load_elem<ELEM>(p, r0 + t.x1), fq_load_elem<ELEM>(p, r1 + t.x0),
                   fq_load_elem<ELEM>(p, r1 + t.x1), t.ax, t.ay);
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// Geometry: 256 threads, grid fq_grid(w, h, images, rows).  A kernel whose workgroup walks more than 4 rows calls fq_y once
// per group g = 0 .. rows / 4 - 1 of 4 rows.
__device__ __forceinline__ int fq_x() { return ((int)blockIdx.x * 64 + ((int)threadIdx.x & 63)) * 4; }
__device__ __forceinline__ int fq_y(int rows = 4, int g = 0) { return (int)blockIdx.y * rows + 4 * g + ((int)threadIdx.x >> 6); }
__device__ __forceinline__ int fq_count(int w, int x) { return min(4, w - x); }
// grid.z holds the items of one launch, at most FQ_ITEMS_MAX (dfx_device.h's DFX_GRID_YZ_MAX): a launcher walks a larger
// batch in several launches.
constexpr int FQ_ITEMS_MAX = DFX_GRID_YZ_MAX;
static inline dim3 fq_grid(int w, int h, int n, int rows = 4) {
    return dim3((unsigned)((w + 255) / 256), (unsigned)((h + rows - 1) / rows), (unsigned)n);
}

// ------------------------------------------------------------------------------------------------
// Quad loads.
// the u plane at pu and the v plane `plane` elements behind it
__device__ __forceinline__ void fq_load_flow(const float *pu, long long plane, bool wide, int n, float (&u)[4], float (&v)[4]) {
    const float *pv = pu + plane;
    if (wide && n == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(pu);
        const float4 r = *reinterpret_cast<const float4 *>(pv);
        u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // loads under a branch, not selects: as selects the compiler issues pu[0] ahead of both paths and leaves the wide
            // one a 12-byte load behind it
            u[k] = v[k] = 0.0f;
            if (k < n)
                u[k] = pu[k], v[k] = pv[k];
        }
    }
}
// a byte plane (a mask, a segment of an 8-bit image)
__device__ __forceinline__ void fq_load_u8(const unsigned char *p, bool wide, int n, unsigned (&e)[4]) {
    if (wide && n == 4) {
        const unsigned q = *reinterpret_cast<const unsigned *>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            e[k] = (q >> (8 * k)) & 0xffu;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            e[k] = k < n ? p[k] : 0u;
    }
}
// a mask: ok[k] = 0 where the pixel's byte is nonzero
__device__ __forceinline__ void fq_mask_clear(const unsigned char *p, bool wide, int n, unsigned (&ok)[4]) {
    unsigned m[4];
    fq_load_u8(p, wide, n, m);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (m[k])
            ok[k] = 0u;
}

// ------------------------------------------------------------------------------------------------
// Quad stores.
__device__ __forceinline__ void fq_store_f32(float *p, bool wide, int n, const float (&a)[4]) {
    if (wide && n == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        // last element first: in ascending order the compiler sinks the store of a[0] behind both paths and leaves the wide
        // one a 12-byte store in front of it
#pragma unroll
        for (int k = 3; k >= 0; --k)
            if (k < n)
                p[k] = a[k];
    }
}
// the u plane at pu and the v plane `plane` elements behind it
__device__ __forceinline__ void fq_store_flow(float *pu, long long plane, bool wide, int n, const float (&u)[4],
                                              const float (&v)[4]) {
    float *pv = pu + plane;
    if (wide && n == 4) {
        *reinterpret_cast<float4 *>(pu) = make_float4(u[0], u[1], u[2], u[3]);
        *reinterpret_cast<float4 *>(pv) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n)
                pu[k] = u[k], pv[k] = v[k];
    }
}
// 4 flags or bytes (values 0 .. 255) to a byte plane
__device__ __forceinline__ void fq_store_u8(unsigned char *p, bool wide, int n, const unsigned (&e)[4]) {
    if (wide && n == 4) {
        *reinterpret_cast<unsigned *>(p) = e[0] | (e[1] << 8) | (e[2] << 16) | (e[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n)
                p[k] = (unsigned char)e[k];
    }
}
// samples in [0, 255] to elements at .. at + n - 1 of an image of dtype FQ_ELEM_U8 ((uint8)rintf: ties to even), DFX_ELEM_F32,
// or DFX_ELEM_F16 / _BF16 (dfx_planar_half_bits).  dtype is one value per launch.
__device__ __forceinline__ void fq_store_image(void *out, long long at, int dtype, bool wide, int n, const float (&s)[4]) {
    if (dtype == FQ_ELEM_U8) {
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            q[k] = (unsigned)rintf(s[k]);
        fq_store_u8(static_cast<unsigned char *>(out) + at, wide, n, q);
    } else if (dtype == DFX_ELEM_F32) {
        fq_store_f32(static_cast<float *>(out) + at, wide, n, s);
    } else {
        unsigned short *p = static_cast<unsigned short *>(out) + at;
        unsigned q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            q[k] = dfx_planar_half_bits(s[k], dtype);
        if (wide && n == 4) {
            *reinterpret_cast<uint2 *>(p) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n)
                    p[k] = (unsigned short)q[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The engines' merge kernels in planar form: 16-byte loads from the engine's u and v planes (their pitch is a multiple of 64
// floats, so the four floats at a multiple of 4 below w exist), stored through dfx_planar_store4.  su / sv: the planes' first
// pixel.  grid: dfx_planar_merge_grid.
__device__ __forceinline__ void dfx_planar_merge_tile(const DfxPlanarOut &o, int i, const float *su, const float *sv, int w,
                                                      int h, int pitch) {
    const int x = fq_x(), y = fq_y();
    if (x >= w || y >= h)
        return;
    const long long s = (long long)y * pitch + x;
    const float4 a = *reinterpret_cast<const float4 *>(su + s), c = *reinterpret_cast<const float4 *>(sv + s);
    const float u[4] = {a.x, a.y, a.z, a.w}, v[4] = {c.x, c.y, c.z, c.w};
    dfx_planar_store4(o, i, x, y, fq_count(w, x), u, v);
}
static inline dim3 dfx_planar_merge_grid(int w, int h, int n) { return fq_grid(w, h, n); }
#endif
