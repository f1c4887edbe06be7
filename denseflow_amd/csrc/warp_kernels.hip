// warp_kernels.hip — the backward warp of 8-bit images by a flow, and the photometric error of the result, on the device:
// what a consumer of flow tensors does next with a flow (an occlusion-aware loss, a frame interpolator, a flow filter), and
// mean |I0 - warp(I1, F)|, the quality figure that needs no ground truth.
//
// Image i is sampled at the positions flow i names.  Output pixel (x, y) with flow (fu, fv), all in float32, every operation
// rounded on its own (the build's -ffp-contract=off: no fused multiply-add anywhere below):
//     px = (float)x + fu;  py = (float)y + fv
//     inside = px >= 0 && py >= 0 && px <= W-1 && py <= H-1      (false for NaN and either infinity; tested before any
//                                                                 conversion to int — the test of fb_check_kernels.hip)
//     WARP_BORDER_ZERO : not inside -> every channel's sample is 0.0f
//     WARP_BORDER_CLAMP: px or py NaN -> sample 0.0f; otherwise px = min(max(px, 0), W-1), py likewise (infinities clamp)
//     x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
//     per channel, P = (float)byte: t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s = t + ay*(b - t)
// s lies in [0, 255] (the taps are representable, every rounding is monotone): no clamp on the way out.  Stored: s as
// float32, s through dfx_planar_half_bits as float16 / bfloat16, or q = (uint8)rintf(s) (ties to even).
//     valid = inside (the unclamped test in either mode) && (no occlusion mask || occ[y][x] == 0)
//     statistics of image i, over its pixels with valid == 1: count += 1, sad += sum over channels |ref - q|   (integers)
// tests/warp_ref.py is the same text in NumPy; the two agree bit for bit.
//
// The lane quad, the tap and the segments of flow_quad.h: the taps plain byte loads (the displacement is unbounded: no tile
// to stage), ref read and out written segment by segment, no scratch, registers for eight waves per SIMD.  The statistics
// form lets a workgroup walk WARP_STATS_ROWS rows, sums count and sad per lane in 32 bits (a workgroup's totals are at most
// 256 * 32 and 256 * 32 * 3 * 255 < 2^23), reduces them across the wave with __shfl_xor and across the four waves through
// 32 bytes of LDS, and one lane issues one 64-bit atomicAdd per word whose value it never reads: a 1080p image issues
// 2 * 8 * 34 = 544 of them.  The form without statistics has no loop, no LDS and no barrier.
// Bytes per pixel: 8 of flow, 1 .. 4 C of taps (perfectly cached .. every tap its own sector), C x elem of out, + C of ref,
// + 1 of occ, + 1 of valid where asked for.
#include "warp_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

static_assert(WARP_OUT_U8 == FQ_ELEM_U8 && WARP_BORDER_ZERO == FQ_BORDER_ZERO && WARP_BORDER_CLAMP == FQ_BORDER_CLAMP,
              "flow_quad.h");

namespace {

// which accesses take a lane's 4 elements at once; one value per launch, so every branch on them is wave-uniform
struct WarpWide {
    int flow, ref, out, occ, valid;
};

// the 4 pixels (x .. x + 3, y) of image i; cnt / sad: the lane's statistics (STATS only)
template <int C, bool IL, bool STATS>
__device__ __forceinline__ void warp_quad(const WarpArgs &a, const WarpWide &wide, int x, int y, long long i, unsigned &cnt,
                                          unsigned &sad) {
    const int n = fq_count(a.w, x);
    const float *fu = a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x;
    float u[4], v[4];
    if constexpr (STATS) {
        fq_load_flow(fu, a.plane_stride, wide.flow != 0, n, u, v);
    } else {
        // The quad load of flow_quad.h with its narrow path as selects, the form this kernel had before the header: kept local
        // because it is what measures as before.  With fq_load_flow's narrow loads under a branch the interleaved form without
        // statistics is 3 - 4 % slower on flows of a quarter of the frame and the planar one 1 %, although the wide path, the
        // one that runs, is the same two 16-byte loads either way; the forms with statistics are up to 3 % faster with
        // fq_load_flow and keep it (profiles/flow_quad/README.md).
        const float *fv = fu + a.plane_stride;
        if (wide.flow && n == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(fu);
            const float4 r = *reinterpret_cast<const float4 *>(fv);
            u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
            v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = k < n ? fu[k] : 0.0f;
                v[k] = k < n ? fv[k] : 0.0f;
            }
        }
    }
    const unsigned char *src = a.src + i * a.src_image;
    float s[4][C];
    unsigned ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ok[k] = 0u;
#pragma unroll
        for (int c = 0; c < C; ++c)
            s[k][c] = 0.0f;
        if (k < n) {
            const FqTap t = fq_tap((float)(x + k) + u[k], (float)y + v[k], a.w, a.h, a.border);
            ok[k] = t.inside ? 1u : 0u;
            if (t.take)
                fq_sample_u8<C, IL>(src, a.src_pitch, a.src_plane, t, s[k]);
        }
    }
    if (a.occ)
        fq_mask_clear(a.occ + i * a.occ_stride + (long long)y * a.occ_pitch + x, wide.occ != 0, n, ok);
    if (a.valid)
        fq_store_u8(a.valid + i * a.valid_stride + (long long)y * a.valid_pitch + x, wide.valid != 0, n, ok);
    if (STATS) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            cnt += ok[k]; // 0 beyond the row's end
    }
#pragma unroll
    for (int g = 0; g < C; ++g) { // the segments of flow_quad.h
        float sv[4];
        fq_segment<C, IL>(s, g, sv);
        const int m = fq_seg_count<C, IL>(g, n);
        if (m <= 0)
            continue;
        if (STATS) {
            const unsigned char *r = a.ref + i * a.src_image + (long long)y * a.src_pitch + fq_seg_offset<C, IL>(x, g, a.src_plane);
            unsigned rv[4];
            fq_load_u8(r, wide.ref != 0, m, rv);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < m && ok[fq_seg_pixel<C, IL>(g, e)]) {
                    const int d = (int)rv[e] - (int)(unsigned)rintf(sv[e]);
                    sad += (unsigned)(d < 0 ? -d : d);
                }
        }
        if (a.out) {
            const long long at = i * a.out_image + (long long)y * a.out_pitch + fq_seg_offset<C, IL>(x, g, a.out_plane);
            fq_store_image(a.out, at, a.out_dtype, wide.out != 0, m, sv);
        }
    }
}

// C: channels; IL: interleaved (C == 3 only); STATS: with the statistics.  grid: (ceil(w / 256), ceil(h / rows), images) with
// rows = WARP_STATS_ROWS for STATS, 4 otherwise.  Eight waves per SIMD (64 registers) for every form but the planar 3-channel
// one with statistics: its three plane addresses per tap and the loop's running sums need more than 64 registers (68 as
// compiled now), so it is given 80 (six waves per SIMD) and never spills.
template <int C, bool IL, bool STATS>
__global__ __launch_bounds__(256, (C == 3 && !IL && STATS) ? 6 : 8) void k_warp(WarpArgs a, WarpWide wide) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = fq_x();
    const long long i = (long long)blockIdx.z;
    unsigned cnt = 0u, sad = 0u;
    if constexpr (!STATS) {
        const int y = fq_y();
        if (x < a.w && y < a.h)
            warp_quad<C, IL, false>(a, wide, x, y, i, cnt, sad);
    } else {
#pragma unroll 1
        for (int g = 0; g < WARP_STATS_ROWS / 4; ++g) {
            const int y = fq_y(WARP_STATS_ROWS, g);
            if (x < a.w && y < a.h)
                warp_quad<C, IL, true>(a, wide, x, y, i, cnt, sad);
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            cnt += __shfl_xor(cnt, m);
            sad += __shfl_xor(sad, m);
        }
        __shared__ unsigned part[8];
        if (lane == 0)
            part[wave] = cnt, part[4 + wave] = sad;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned c4 = part[0] + part[1] + part[2] + part[3];
            const unsigned s4 = part[4] + part[5] + part[6] + part[7];
            if (c4)
                atomicAdd(a.stats + 2 * i, (unsigned long long)c4);
            if (s4)
                atomicAdd(a.stats + 2 * i + 1, (unsigned long long)s4);
        }
    }
}

template <int C, bool IL>
void warp_launch_as(hipStream_t s, const WarpArgs &a, const WarpWide &wide) {
    if (a.stats)
        hipLaunchKernelGGL((k_warp<C, IL, true>), fq_grid(a.w, a.h, a.n, WARP_STATS_ROWS), dim3(256), 0, s, a, wide);
    else
        hipLaunchKernelGGL((k_warp<C, IL, false>), fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
}

} // namespace

void warp_launch(hipStream_t s, const WarpArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    const bool three = args.channels == 3, planes = three && args.planar != 0;
    const int eb = args.out_dtype == WARP_OUT_U8 ? 1 : dfx_elem_bytes(args.out_dtype);
    // a lane's 4 elements in one access: the base and every stride a multiple of that access
    WarpWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.ref = dfx_bytes4(args.ref, args.src_pitch, args.src_image, planes ? args.src_plane : 0);
    wide.out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, eb) == 4;
    wide.occ = dfx_bytes4(args.occ, args.occ_pitch, args.occ_stride, 0);
    wide.valid = dfx_bytes4(args.valid, args.valid_pitch, args.valid_stride, 0);
    if (args.stats)
        (void)hipMemsetAsync(args.stats, 0, (size_t)args.n * 2 * sizeof(unsigned long long), s);
    // grid.z holds at most FQ_ITEMS_MAX = 65535 images: more than that go in several launches
    const int chunk = FQ_ITEMS_MAX;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        WarpArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.src += (long long)i0 * args.src_image;
        a.flow += (long long)i0 * args.flow_stride;
        if (a.ref)
            a.ref += (long long)i0 * args.src_image;
        if (a.out)
            a.out = static_cast<unsigned char *>(a.out) + (long long)i0 * args.out_image * eb;
        if (a.occ)
            a.occ += (long long)i0 * args.occ_stride;
        if (a.valid)
            a.valid += (long long)i0 * args.valid_stride;
        if (a.stats)
            a.stats += 2LL * i0;
        if (!three)
            warp_launch_as<1, false>(s, a, wide);
        else if (!planes)
            warp_launch_as<3, true>(s, a, wide);
        else
            warp_launch_as<3, false>(s, a, wide);
    }
}
