// flow_colour_kernels.hip — flows as colour images on the device: the Middlebury colour wheel (Baker et al. 2011), unknown
// pixels marked and left out of the normalisation.  The arithmetic is section (0.5.1) of include/dfx.h, float32, every
// operation rounded on its own (the build's -ffp-contract=off), / and sqrtf IEEE; tests/flow_colour_ref.py is the same text in
// NumPy and the two agree byte for byte, and bit for bit in the squared radii.
//
// Two streaming passes with no host synchronisation between them, on the lane quad and the segments of flow_quad.h:
//   k_flowvis_max    : the squared radius of the known pixels, reduced with integer max on the bit patterns (a known r2 is
//                      never negative and never NaN, so the order does not matter) across the wave, the workgroup's four
//                      waves (LDS) and then with one atomic max per workgroup into word i and one into word n.
//   k_flowvis_colour : reads R from those words (or max_rad), colours, marks, blends and stores.  The wheel lies in LDS as 56
//                      float4 {r, g, b, 0} / 255.0f, entry 55 = entry 0, so k1 = k0 + 1 is the text's wrap-around.
// Bytes per pixel: 8 (+ 1 of mask) per pass read, 3 written (+ 1 or 3 of frame read).  No scratch; LDS: 16 bytes / 896 bytes.
#include "flow_colour_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_angle.h"
#include "flow_quad.h"

namespace {

constexpr int FV_MAX_ROWS = 16; // rows per workgroup of the measuring pass: four per wave, one atomic pair per 256 x 16 pixels

struct FlowvisWide { // a lane's 4 elements in one access: wave-uniform
    int flow, mask, out, frame;
};

// pixels x .. x + n - 1 of row y of flow i as they lie in memory: (u, v) and the mask bytes (0 without masks); pixels beyond
// the row's end come back as (0, 0), unmasked.  Loads only: a caller that fetches several rows has all of them in flight.
template <bool MASKED>
__device__ __forceinline__ void fv_fetch(const FlowvisArgs &a, const FlowvisWide &wide, long long i, int x, int y, int n,
                                         float (&u)[4], float (&v)[4], unsigned (&m)[4]) {
    fq_load_flow(a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x, a.plane_stride, wide.flow != 0, n, u, v);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        m[k] = 0u;
    if (MASKED)
        fq_load_u8(a.mask + i * a.mask_stride + (long long)y * a.mask_pitch + x, wide.mask != 0, n, m);
}

// which of the n fetched pixels are known; unknown pixels and those beyond the row's end become (0, 0), not known — nothing
// of the padding or of a NaN goes any further
__device__ __forceinline__ void fv_classify(int n, float (&u)[4], float (&v)[4], const unsigned (&m)[4], bool (&kn)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // false for NaN and for either infinity
        kn[k] = k < n && m[k] == 0u && __builtin_fabsf(u[k]) <= 1e9f && __builtin_fabsf(v[k]) <= 1e9f;
        u[k] = kn[k] ? u[k] : 0.0f;
        v[k] = kn[k] ? v[k] : 0.0f;
    }
}

// grid: (ceil(w / 256), ceil(h / FV_MAX_ROWS), flows).  Every lane reaches the barrier; lanes and rows outside the image
// contribute 0.
template <bool MASKED>
__global__ __launch_bounds__(256) void k_flowvis_max(FlowvisArgs a, FlowvisWide wide) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = fq_x();
    const long long i = (long long)a.i0 + (long long)blockIdx.z;
    constexpr int G = FV_MAX_ROWS / 4;
    const int n = min(4, a.w - x); // <= 0 in lanes right of the image
    float u[G][4], v[G][4];
    unsigned mk[G][4];
    // first every row's loads, then the arithmetic: the loads of all four rows are in flight at once
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int y = fq_y(FV_MAX_ROWS, g);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            u[g][k] = v[g][k] = 0.0f, mk[g][k] = 0u;
        if (n > 0 && y < a.h)
            fv_fetch<MASKED>(a, wide, i, x, y, n, u[g], v[g], mk[g]);
    }
    unsigned best = 0u;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        bool kn[4];
        fv_classify(n, u[g], v[g], mk[g], kn);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float r2 = u[g][k] * u[g][k] + v[g][k] * v[g][k]; // (0, 0) where not known: +0, the maximum's start
            best = max(best, __float_as_uint(r2));
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1)
        best = max(best, (unsigned)__shfl_xor((int)best, m));
    __shared__ unsigned part[4];
    if (lane == 0)
        part[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned b4 = max(max(part[0], part[1]), max(part[2], part[3]));
        if (b4) { // the words start at +0
            unsigned *words = reinterpret_cast<unsigned *>(a.max2);
            atomicMax(words + i, b4);
            atomicMax(words + a.n, b4);
        }
    }
}

// entry k of the wheel as {r, g, b, 0} / 255.0f: the segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
__device__ __forceinline__ float4 fv_wheel_entry(int k) {
    int r, g, b;
    if (k < 15) {
        r = 255, g = 255 * k / 15, b = 0;
    } else if (k < 21) {
        r = 255 - 255 * (k - 15) / 6, g = 255, b = 0;
    } else if (k < 25) {
        r = 0, g = 255, b = 255 * (k - 21) / 4;
    } else if (k < 36) {
        r = 0, g = 255 - 255 * (k - 25) / 11, b = 255;
    } else if (k < 49) {
        r = 255 * (k - 36) / 13, g = 0, b = 255;
    } else {
        r = 255, g = 0, b = 255 - 255 * (k - 49) / 6;
    }
    return make_float4((float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f, 0.0f);
}

// the RGB bytes of a known flow vector under D = R + 2^-23
__device__ __forceinline__ void fv_colour(float u, float v, float D, bool measured, const float4 *wheel, unsigned (&rgb)[3]) {
    const float un = u / D, vn = v / D;
    float rad = sqrtf(un * un + vn * vn);
    if (measured)
        rad = __builtin_fminf(rad, 1.0f);
    const float a = fv_atan2_turns(-vn, -un);
    float fk = (a + 1.0f) * 27.0f;
    fk = __builtin_fminf(__builtin_fmaxf(fk, 0.0f), 54.0f);
    const float fl = floorf(fk);
    const int k0 = (int)fl;
    const float f = fk - fl;
    const float4 w0 = wheel[k0], w1 = wheel[k0 + 1]; // entry 55 is entry 0
    const float c0[3] = {w0.x, w0.y, w0.z}, c1[3] = {w1.x, w1.y, w1.z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float col = (1.0f - f) * c0[c] + f * c1[c];
        col = rad <= 1.0f ? 1.0f - rad * (1.0f - col) : col * 0.75f;
        rgb[c] = (unsigned)__builtin_fminf(__builtin_fmaxf(floorf(255.0f * col), 0.0f), 255.0f);
    }
}

// MASKED: with mask planes; IL: interleaved output (three planes otherwise); BLEND: over a frame.
// grid: (ceil(w / 256), ceil(h / 4), flows).
template <bool MASKED, bool IL, bool BLEND>
__global__ __launch_bounds__(256) void k_flowvis_colour(FlowvisArgs a, FlowvisWide wide) {
    __shared__ float4 wheel[56];
    if (threadIdx.x < 56)
        wheel[threadIdx.x] = fv_wheel_entry(threadIdx.x == 55 ? 0 : (int)threadIdx.x);
    __syncthreads();
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long i = (long long)a.i0 + (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    const bool measured = a.norm != FLOWVIS_NORM_FIXED; // wave-uniform, as R is
    const float R = measured ? sqrtf(a.max2[a.norm == FLOWVIS_NORM_FLOW ? i : (long long)a.n]) : a.max_rad;
    const float D = R + 0x1p-23f;
    float u[4], v[4];
    unsigned mk[4];
    bool kn[4];
    fv_fetch<MASKED>(a, wide, i, x, y, n, u, v, mk);
    fv_classify(n, u, v, mk, kn);
    unsigned o[4][3]; // the pixels' bytes in the output's channel order
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned rgb[3];
        fv_colour(u[k], v[k], D, measured, wheel, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned q = a.bgr ? rgb[2 - c] : rgb[c];
            o[k][c] = kn[k] ? q : (unsigned)a.unknown[c];
        }
    }
    if (BLEND) {
        unsigned fr[4][3];
        const unsigned char *f = a.frame + i * a.frame_image + (long long)y * a.frame_pitch;
        if (a.frame_channels == 1) {
            unsigned e[4];
            fq_load_u8(f + x, wide.frame != 0, n, e);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                fr[k][0] = fr[k][1] = fr[k][2] = e[k];
        } else if (a.frame_planar) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                unsigned e[4];
                fq_load_u8(f + c * a.frame_plane + x, wide.frame != 0, n, e);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    fr[k][c] = e[k];
            }
        } else {
#pragma unroll
            for (int g = 0; g < 3; ++g) { // the interleaved segments of flow_quad.h
                unsigned e[4];
                fq_load_u8(f + fq_seg_offset<3, true>(x, g, 0), wide.frame != 0, fq_seg_count<3, true>(g, n), e);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    fr[fq_seg_pixel<3, true>(g, k)][fq_seg_channel<3, true>(g, k)] = e[k];
            }
        }
        const unsigned al = (unsigned)a.alpha256;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                o[k][c] = (al * o[k][c] + (256u - al) * fr[k][c] + 128u) >> 8;
    }
    unsigned char *d = a.out + i * a.out_image + (long long)y * a.out_pitch;
#pragma unroll
    for (int g = 0; g < 3; ++g) { // the segments of flow_quad.h
        unsigned e[4];
        fq_segment<3, IL>(o, g, e);
        const int m = fq_seg_count<3, IL>(g, n);
        if (m > 0)
            fq_store_u8(d + fq_seg_offset<3, IL>(x, g, a.out_plane), wide.out != 0, m, e);
    }
}

template <bool MASKED, bool IL>
void flowvis_colour_as(hipStream_t s, const dim3 &grid, const FlowvisArgs &a, const FlowvisWide &wide) {
    if (a.frame)
        hipLaunchKernelGGL((k_flowvis_colour<MASKED, IL, true>), grid, dim3(256), 0, s, a, wide);
    else
        hipLaunchKernelGGL((k_flowvis_colour<MASKED, IL, false>), grid, dim3(256), 0, s, a, wide);
}

} // namespace

void flowvis_launch(hipStream_t s, const FlowvisArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    // a lane's 4 elements in one access: the base and every stride a multiple of that access
    FlowvisWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.mask = dfx_bytes4(args.mask, args.mask_pitch, args.mask_stride, 0);
    wide.out = dfx_bytes4(args.out, args.out_pitch, args.out_image, args.planar ? args.out_plane : 0);
    wide.frame = dfx_bytes4(args.frame, args.frame_pitch, args.frame_image,
                            args.frame_channels == 3 && args.frame_planar ? args.frame_plane : 0);
    if (args.max2)
        (void)hipMemsetAsync(args.max2, 0, ((size_t)args.n + 1) * sizeof(float), s);
    // grid.z holds at most FQ_ITEMS_MAX = 65535 flows: more than that go in several launches, every measuring launch before the first colour launch
    const int chunk = FQ_ITEMS_MAX;
    for (int pass = args.max2 ? 0 : 1; pass < 2; ++pass) {
        for (int i0 = 0; i0 < args.n; i0 += chunk) {
            FlowvisArgs a = args;
            a.i0 = i0;
            const unsigned gz = (unsigned)std::min(chunk, args.n - i0);
            if (pass == 0) {
                const dim3 grid = fq_grid(a.w, a.h, (int)gz, FV_MAX_ROWS);
                if (a.mask)
                    hipLaunchKernelGGL((k_flowvis_max<true>), grid, dim3(256), 0, s, a, wide);
                else
                    hipLaunchKernelGGL((k_flowvis_max<false>), grid, dim3(256), 0, s, a, wide);
                continue;
            }
            const dim3 grid = fq_grid(a.w, a.h, (int)gz);
            if (a.mask && !a.planar)
                flowvis_colour_as<true, true>(s, grid, a, wide);
            else if (a.mask)
                flowvis_colour_as<true, false>(s, grid, a, wide);
            else if (!a.planar)
                flowvis_colour_as<false, true>(s, grid, a, wide);
            else
                flowvis_colour_as<false, false>(s, grid, a, wide);
        }
    }
}
