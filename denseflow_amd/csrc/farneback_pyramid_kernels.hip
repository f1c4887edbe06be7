// farneback_pyramid_kernels.hip — the two kernels of -a=farn with dfx_params.farn_fast_pyramids (upstream's
// fastPyramids): k_farn_pyrdown builds a frame's pyramid level from the level below it,
// k_farn_pyrup_flow carries a pair's flow from a level to the next finer one.
//
// Both are streaming 5-tap stencils with the dyadic taps (1, 4, 6, 4, 1) / 16 and nothing to compute beside them, so they
// are laid out for the memory system: a wave owns a column strip and walks down it, the rows of the vertical pass roll
// through registers (every source row is loaded once per wave), the horizontal neighbours come from the neighbouring
// lanes (__shfl_up / __shfl_down: no LDS allocation, no barrier), the first and last lane of a wave are halo lanes that
// only feed their neighbours.  The dominating stream of each kernel moves in 16- or 8-byte accesses: k_farn_pyrdown loads
// four source columns per lane (16 B) and stores two results (8 B), k_farn_pyrup_flow loads one source value per lane and
// component and stores two results per output row (8 B).
// Compiled with -ffp-contract=off: products and sums round separately, left to right, as the reference states them.
#include <hip/hip_runtime.h>

#include "dfx_device.h"
#include "farneback_kernels.h"

namespace {

constexpr float kC0 = 0.0625f, kC1 = 0.25f, kC2 = 0.375f; // taps c0 = c4, c1 = c3, c2
constexpr int kDownCols = 124; // output columns of a wave: lanes 1 .. 62, two each
constexpr int kDownRows = 8;   // output rows a wave walks (2 * 8 + 3 source rows)
constexpr int kUpCols = 62;    // source columns of a wave: lanes 1 .. 62, one each (124 output columns)
constexpr int kUpRows = 8;     // source rows a wave walks (16 output rows)

__device__ __forceinline__ int pyr_reflect101(int x, int last) { // BORDER_REFLECT_101, any x
    x = abs(x) % (2 * last);                                     // period 2 * last; last >= 1
    return x > last ? 2 * last - x : x;
}

struct F4 {
    float x, y, z, w;
};

// source columns q .. q + 3 (q a multiple of 4) of one row, reflected at the plane's edges
__device__ __forceinline__ F4 pyr_load4(const float *row, int q, int sw) {
    F4 r;
    if (q >= 0 && q + 3 < sw) {
        const float4 v = *reinterpret_cast<const float4 *>(row + q); // pitch and plane strides are multiples of 64 floats
        r.x = v.x, r.y = v.y, r.z = v.z, r.w = v.w;
    } else {
        r.x = row[pyr_reflect101(q, sw - 1)];
        r.y = row[pyr_reflect101(q + 1, sw - 1)];
        r.z = row[pyr_reflect101(q + 2, sw - 1)];
        r.w = row[pyr_reflect101(q + 3, sw - 1)];
    }
    return r;
}
// the caller's 8-bit frame: its pitch is the caller's, so single bytes; the (float) is upstream's convertTo, exact
__device__ __forceinline__ F4 pyr_load4(const unsigned char *row, int q, int sw) {
    F4 r;
    if (q >= 0 && q + 3 < sw) {
        r.x = (float)row[q], r.y = (float)row[q + 1], r.z = (float)row[q + 2], r.w = (float)row[q + 3];
    } else {
        r.x = (float)row[pyr_reflect101(q, sw - 1)];
        r.y = (float)row[pyr_reflect101(q + 1, sw - 1)];
        r.z = (float)row[pyr_reflect101(q + 2, sw - 1)];
        r.w = (float)row[pyr_reflect101(q + 3, sw - 1)];
    }
    return r;
}

__device__ __forceinline__ float pyr_tap5(float a, float b, float c, float d, float e) {
    float v = kC0 * a + kC1 * b;
    v = v + kC2 * c;
    v = v + kC1 * d;
    v = v + kC0 * e;
    return v;
}

} // namespace

// dst[z] = pyrDown(src[z]) (B.13): sw x sh -> (sw + 1) / 2 x (sh + 1) / 2, vertical pass first, reflect-101 both ways.
// Lane l of a wave holds source columns q .. q + 3, q = 2 * (124 * strip) - 4 + 4 * l, and produces the output columns q / 2
// and q / 2 + 1 from its own four vertical sums, the last two of lane l - 1 and the first of lane l + 1.
template <class SRC>
__global__ __launch_bounds__(256) void k_farn_pyrdown(const SRC *__restrict__ src, long long src_frame_stride, long long spitch,
                                                      int sw, int sh, float *__restrict__ dst, long long dst_frame_stride,
                                                      int dpitch) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    const int y0 = ((int)blockIdx.y * 4 + wave) * kDownRows;
    if (y0 >= dh)
        return; // the whole wave
    const int y1 = min(y0 + kDownRows, dh);
    const int a0 = (int)blockIdx.x * kDownCols - 2 + 2 * lane; // first output column of this lane
    const int q = 2 * a0;
    const SRC *s = src + (long long)blockIdx.z * src_frame_stride;
    float *d = dst + (long long)blockIdx.z * dst_frame_stride;
    const bool writes = lane >= 1 && lane <= 62 && a0 < dw;

    F4 r0 = pyr_load4(s + (long long)pyr_reflect101(2 * y0 - 2, sh - 1) * spitch, q, sw);
    F4 r1 = pyr_load4(s + (long long)pyr_reflect101(2 * y0 - 1, sh - 1) * spitch, q, sw);
    F4 r2 = pyr_load4(s + (long long)(2 * y0) * spitch, q, sw);
    for (int y = y0; y < y1; ++y) {
        const F4 r3 = pyr_load4(s + (long long)pyr_reflect101(2 * y + 1, sh - 1) * spitch, q, sw);
        const F4 r4 = pyr_load4(s + (long long)pyr_reflect101(2 * y + 2, sh - 1) * spitch, q, sw);
        const float vx = pyr_tap5(r0.x, r1.x, r2.x, r3.x, r4.x);
        const float vy = pyr_tap5(r0.y, r1.y, r2.y, r3.y, r4.y);
        const float vz = pyr_tap5(r0.z, r1.z, r2.z, r3.z, r4.z);
        const float vw = pyr_tap5(r0.w, r1.w, r2.w, r3.w, r4.w);
        const float lz = __shfl_up(vz, 1), lw = __shfl_up(vw, 1); // columns q - 2, q - 1
        const float rx = __shfl_down(vx, 1);                      // column q + 4
        if (writes) {
            const float o0 = pyr_tap5(lz, lw, vx, vy, vz);
            const float o1 = pyr_tap5(vx, vy, vz, vw, rx);
            float *o = d + (long long)y * dpitch + a0;
            if (a0 + 1 < dw)
                *reinterpret_cast<float2 *>(o) = make_float2(o0, o1);
            else
                o[0] = o0;
        }
        r0 = r2, r1 = r3, r2 = r4; // rows 2y + 1 and 2y + 2 are inside the plane whenever row y + 1 is an output row
    }
}

namespace {

struct UpRow { // one source row after the horizontal pass: output columns 2a and 2a + 1 of both components
    float u0, u1, v0, v1;
};

// The horizontal pass of pyrUp on source row r: every lane loads the value at its border index b(a) = min(|a|, sw - 1),
// so the neighbouring lanes hold s[b(a - 1)] and s[b(a + 1)].
__device__ __forceinline__ UpRow pyrup_row(const float *su, const float *sv, int r, int spitch, int ab) {
    const float u = su[(long long)r * spitch + ab], v = sv[(long long)r * spitch + ab];
    const float ul = __shfl_up(u, 1), ur = __shfl_down(u, 1);
    const float vl = __shfl_up(v, 1), vr = __shfl_down(v, 1);
    UpRow t;
    t.u0 = (kC0 * ul + kC2 * u) + kC0 * ur;
    t.u1 = kC1 * u + kC1 * ur;
    t.v0 = (kC0 * vl + kC2 * v) + kC0 * vr;
    t.v1 = kC1 * v + kC1 * vr;
    return t;
}

} // namespace

// flow set dst_set of level c.L = pyrUp(flow set src_set of the coarser level, sw x sh, pitch spitch) * up (B.13):
// c.L.w = 2 * sw and c.L.h = 2 * sh (the engine accepts no other sizes), horizontal pass first, border index
// min(|i|, n - 1), times 4, then times up.  Lane l of a wave holds source column 62 * strip - 1 + l.
__global__ __launch_bounds__(256) void k_farn_pyrup_flow(FarnPairCtx c, int src_set, int dst_set, int sw, int sh, int spitch,
                                                         float up) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int r0 = ((int)blockIdx.y * 4 + wave) * kUpRows;
    if (r0 >= sh)
        return; // the whole wave
    const int r1 = min(r0 + kUpRows, sh);
    const int a = (int)blockIdx.x * kUpCols - 1 + lane;
    const int ab = min(abs(a), sw - 1);
    const int b = (int)blockIdx.z;
    const float *su = c.planes + (long long)b * c.slot_stride + (long long)(FARN_PL_FX0 + 2 * src_set) * c.plane_stride;
    const float *sv = su + c.plane_stride;
    float *du = c.planes + (long long)b * c.slot_stride + (long long)(FARN_PL_FX0 + 2 * dst_set) * c.plane_stride;
    float *dv = du + c.plane_stride;
    const bool writes = lane >= 1 && lane <= 62 && a < sw;

    UpRow tp = pyrup_row(su, sv, min(abs(r0 - 1), sh - 1), spitch, ab);
    UpRow tc = pyrup_row(su, sv, r0, spitch, ab);
    for (int r = r0; r < r1; ++r) {
        const UpRow tn = pyrup_row(su, sv, min(r + 1, sh - 1), spitch, ab);
        if (writes) {
            const long long o = (long long)(2 * r) * c.L.pitch + 2 * a;
            float e0 = (kC0 * tp.u0 + kC2 * tc.u0) + kC0 * tn.u0, e1 = (kC0 * tp.u1 + kC2 * tc.u1) + kC0 * tn.u1;
            float o0 = kC1 * tc.u0 + kC1 * tn.u0, o1 = kC1 * tc.u1 + kC1 * tn.u1;
            *reinterpret_cast<float2 *>(du + o) = make_float2(e0 * 4.0f * up, e1 * 4.0f * up);
            *reinterpret_cast<float2 *>(du + o + c.L.pitch) = make_float2(o0 * 4.0f * up, o1 * 4.0f * up);
            e0 = (kC0 * tp.v0 + kC2 * tc.v0) + kC0 * tn.v0, e1 = (kC0 * tp.v1 + kC2 * tc.v1) + kC0 * tn.v1;
            o0 = kC1 * tc.v0 + kC1 * tn.v0, o1 = kC1 * tc.v1 + kC1 * tn.v1;
            *reinterpret_cast<float2 *>(dv + o) = make_float2(e0 * 4.0f * up, e1 * 4.0f * up);
            *reinterpret_cast<float2 *>(dv + o + c.L.pitch) = make_float2(o0 * 4.0f * up, o1 * 4.0f * up);
        }
        tp = tc, tc = tn;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers

static dim3 pyrdown_grid(int sw, int sh, int n) {
    const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
    return dim3((dw + kDownCols - 1) / kDownCols, (dh + 4 * kDownRows - 1) / (4 * kDownRows), n);
}

void farn_launch_pyrdown(hipStream_t s, const float *src, long long src_frame_stride, int src_pitch, int n_frames, int sw,
                         int sh, float *dst, long long dst_frame_stride, int dst_pitch) {
    hipLaunchKernelGGL(k_farn_pyrdown<float>, pyrdown_grid(sw, sh, n_frames), dim3(256), 0, s, src, src_frame_stride,
                       (long long)src_pitch, sw, sh, dst, dst_frame_stride, dst_pitch);
}

void farn_launch_pyrdown_u8(hipStream_t s, const unsigned char *src, long long src_frame_stride, long long src_pitch,
                            int n_frames, int sw, int sh, float *dst, long long dst_frame_stride, int dst_pitch) {
    hipLaunchKernelGGL(k_farn_pyrdown<unsigned char>, pyrdown_grid(sw, sh, n_frames), dim3(256), 0, s, src, src_frame_stride,
                       src_pitch, sw, sh, dst, dst_frame_stride, dst_pitch);
}

void farn_launch_pyrup_flow(hipStream_t s, const FarnPairCtx &c, int src_set, int dst_set, int prev_w, int prev_h,
                            int prev_pitch, float up) {
    const dim3 grid((prev_w + kUpCols - 1) / kUpCols, (prev_h + 4 * kUpRows - 1) / (4 * kUpRows), c.n_pairs);
    hipLaunchKernelGGL(k_farn_pyrup_flow, grid, dim3(256), 0, s, c, src_set, dst_set, prev_w, prev_h, prev_pitch, up);
}
