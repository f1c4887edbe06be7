// flow_chain_kernels.hip — adjacent flows composed into long-range flows and dense trajectories, on the device: what a
// consumer of flow tensors needs once one pair of frames is not enough (dense trajectories, -s=N flows without a long-range
// estimate, feature propagation over a clip, the seed of a long-range estimate).
//
// F_k is the flow of link k, A the accumulated flow of a pixel (x, y) of the anchor frame, all in float32, every operation
// rounded on its own (the build's -ffp-contract=off: no fused multiply-add anywhere below), subnormals kept.
// A_0 = (+0, +0), valid_0 = 1; per link k:
//     px = (float)x + Au;  py = (float)y + Av
//     inside = px >= 0 && py >= 0 && px <= W-1 && py <= H-1      (false for NaN and either infinity; tested before any
//                                                                 conversion to int — the test of warp_kernels.hip)
//     FC_BORDER_ZERO : take = inside
//     FC_BORDER_CLAMP: take = px, py both not NaN;  px = min(max(px, 0), W-1), py likewise (infinities clamp)
//     x0 = floor(px), y0 = floor(py), ax = px - x0, ay = py - y0, x1 = min(x0+1, W-1), y1 = min(y0+1, H-1)
//     per plane c of F_k, P = that plane: t = P[y0][x0] + ax*(P[y0][x1] - P[y0][x0]); b the same on row y1; s_c = t + ay*(b - t)
//     take:     Au = Au + s_u;  Av = Av + s_v          not take: A unchanged, bit for bit
//     occluded = take && occ && (occ[y0][x0] | (ax > 0 ? occ[y0][x1] : 0) | (ay > 0 ? occ[y1][x0] : 0)
//                                | (ax > 0 && ay > 0 ? occ[y1][x1] : 0)) != 0               (the masks of flow k)
//     valid_{k+1} = valid_k && inside && !occluded
// No link is shortcut: 0 * (inf - x) is NaN and the lerp says so, at link 0 (ax = ay = 0) as anywhere.
// tests/flow_chain_ref.py is the same text in NumPy; the two agree bit for bit (NaN for NaN).
//
// The lane quad and the tap of flow_quad.h, grid.z the anchors.  A lane keeps A and valid of its 4 pixels in registers
// through all L links of its chain (the loop is in the kernel, not unrolled): one launch per call however long the chain,
// and nothing goes through HBM between links unless every link is emitted.  Link 0
// samples the pixel itself: the lane's own 4 elements of rows y and y1 of each plane, and its 4 mask bytes, are one access
// each (plus the one element to the right of them); every later link gathers its 4 taps per plane from global memory (the
// displacement is unbounded: no tile to stage), the two taps of a row as one 8-byte load (FC_PAIR_TAPS; 4-byte aligned, which
// global loads of gfx950 accept) taken at min(x0, W-2) so that it never leaves the row.  No LDS, no barrier, no scratch.
// Bytes per pixel and link: 8 of flow gathered where neighbouring lanes land on neighbouring taps (up to 4 sectors per plane
// where they do not), 1 .. 4 of mask, + 8 of out + 1 of valid per emitted flow.
#include "flow_chain_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

static_assert(FC_BORDER_ZERO == FQ_BORDER_ZERO && FC_BORDER_CLAMP == FQ_BORDER_CLAMP, "flow_quad.h");

#ifndef FC_PAIR_TAPS
#define FC_PAIR_TAPS 1 // 0: every tap a 4-byte load of its own (kept for profiles/flow_chain's A/B)
#endif

namespace {

// which accesses take a lane's 4 elements at once, and whether a row's two taps are one load; one value per launch, so
// every branch on them is wave-uniform
struct FcWide {
    int flow, occ, out, valid, pair;
};

// r[0 .. n-1] = row[x .. x+n-1] (one access where wide and n == 4), r[4] = row[min(x+4, w-1)] where n == 4.  The quad load of
// flow_quad.h with a fifth element and a compiler barrier that only this kernel needs: kept here, not in the shared loader.
__device__ __forceinline__ void fc_row5(const float *row, int x, int n, int w, bool wide, float (&r)[5]) {
    if (wide && n == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(row + x);
        r[0] = q.x, r[1] = q.y, r[2] = q.z, r[3] = q.w;
    } else {
        // an index the compiler cannot equate with the one above: it would otherwise hoist this path's first load out of
        // both paths and leave the wide one a 12-byte load behind it
        int xs = x;
        asm volatile("" : "+v"(xs));
#pragma unroll
        for (int e = 0; e < 4; ++e)
            r[e] = e < n ? row[xs + e] : 0.0f;
    }
    r[4] = n == 4 ? row[min(x + 4, w - 1)] : 0.0f;
}

// the tap to the right of element e of a lane's row: element min(x+e+1, w-1)
__device__ __forceinline__ float fc_right(const float (&r)[5], int e, int n) {
    return e == 3 ? r[4] : (e + 1 < n ? r[e + 1] : r[e]);
}

// the taps row[x0], row[x1]; xb = min(x0, w-2) is the pair's base (x1 == x0 only in the last column)
__device__ __forceinline__ void fc_taps(const float *row, int x0, int x1, int xb, bool pair, float &p0, float &p1) {
    if (pair) {
        float q[2];
        __builtin_memcpy(q, row + xb, sizeof q);
        p0 = x0 == x1 ? q[1] : q[0];
        p1 = q[1];
    } else {
        p0 = row[x0];
        p1 = row[x1];
    }
}

// one link of one pixel: fu the u plane of the link's flow, oc its mask
template <bool OCC>
__device__ __forceinline__ void fc_step(const FcArgs &a, bool pair, const float *fu, const unsigned char *oc, int xe, int y,
                                        float &au, float &av, unsigned &ok) {
    const FqTap t = fq_tap((float)xe + au, (float)y + av, a.w, a.h, a.border);
    bool good = t.inside;
    if (t.take) {
        const int xb = min(t.x0, a.w - 2);
        const float *r0 = fu + (long long)t.y0 * a.row_pitch, *r1 = fu + (long long)t.y1 * a.row_pitch;
        float p00, p01, p10, p11;
        fc_taps(r0, t.x0, t.x1, xb, pair, p00, p01);
        fc_taps(r1, t.x0, t.x1, xb, pair, p10, p11);
        const float su = fq_lerp(p00, p01, p10, p11, t.ax, t.ay);
        fc_taps(r0 + a.plane_stride, t.x0, t.x1, xb, pair, p00, p01);
        fc_taps(r1 + a.plane_stride, t.x0, t.x1, xb, pair, p10, p11);
        const float sv = fq_lerp(p00, p01, p10, p11, t.ax, t.ay);
        au = au + su;
        av = av + sv;
        if (OCC) {
            const unsigned char *o0 = oc + (long long)t.y0 * a.occ_pitch, *o1 = oc + (long long)t.y1 * a.occ_pitch;
            const unsigned m00 = o0[t.x0], m01 = o0[t.x1], m10 = o1[t.x0], m11 = o1[t.x1];
            const unsigned m =
                m00 | (t.ax > 0.0f ? m01 : 0u) | (t.ay > 0.0f ? m10 : 0u) | (t.ax > 0.0f && t.ay > 0.0f ? m11 : 0u);
            good = good && m == 0u;
        }
    }
    ok = (ok != 0u && good) ? 1u : 0u;
}

// the lane's n pixels of output flow o and of its valid plane
__device__ __forceinline__ void fc_emit(const FcArgs &a, const FcWide &wide, long long o, int x, int y, int n, const float (&au)[4],
                                        const float (&av)[4], const unsigned (&ok)[4]) {
    fq_store_flow(a.out + o * a.out_stride + (long long)y * a.out_pitch + x, a.out_plane, wide.out != 0, n, au, av);
    if (a.valid)
        fq_store_u8(a.valid + o * a.valid_stride + (long long)y * a.valid_pitch + x, wide.valid != 0, n, ok);
}

// OCC: with occlusion masks; ALL: every link's A is emitted (FC_ALL), not only the last.  grid: (ceil(w / 256), ceil(h / 4),
// anchors).  Eight waves per SIMD (64 registers) in every form.
template <bool OCC, bool ALL>
__global__ __launch_bounds__(256, 8) void k_flow_chain(FcArgs a, FcWide wide) {
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long j = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    long long link = (long long)a.first + j * a.anchor_step; // the flow this link reads
    const long long o0 = ALL ? j * a.length : j;            // the chain's first output flow
    float au[4], av[4];
    unsigned ok[4];
    {
        // link 0: the position is the pixel itself (ax = ay = +0, always inside); the lerp is still the lerp
        const int y1 = min(y + 1, a.h - 1);
        const float *r0 = a.flow + link * a.flow_stride + (long long)y * a.row_pitch;
        const float *r1 = a.flow + link * a.flow_stride + (long long)y1 * a.row_pitch;
        float t0[5], t1[5];
        fc_row5(r0, x, n, a.w, wide.flow != 0, t0);
        fc_row5(r1, x, n, a.w, wide.flow != 0, t1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            au[e] = e < n ? 0.0f + fq_lerp(t0[e], fc_right(t0, e, n), t1[e], fc_right(t1, e, n), 0.0f, 0.0f) : 0.0f;
        fc_row5(r0 + a.plane_stride, x, n, a.w, wide.flow != 0, t0);
        fc_row5(r1 + a.plane_stride, x, n, a.w, wide.flow != 0, t1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            av[e] = e < n ? 0.0f + fq_lerp(t0[e], fc_right(t0, e, n), t1[e], fc_right(t1, e, n), 0.0f, 0.0f) : 0.0f;
            ok[e] = e < n ? 1u : 0u;
        }
        if (OCC)
            fq_mask_clear(a.occ + link * a.occ_stride + (long long)y * a.occ_pitch + x, wide.occ != 0, n, ok);
    }
    if (ALL)
        fc_emit(a, wide, o0, x, y, n, au, av, ok);
#pragma unroll 1
    for (int k = 1; k < a.length; ++k) {
        link += a.hop;
        const float *fu = a.flow + link * a.flow_stride;
        const unsigned char *oc = OCC ? a.occ + link * a.occ_stride : nullptr;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n)
                fc_step<OCC>(a, wide.pair != 0, fu, oc, x + e, y, au[e], av[e], ok[e]);
        if (ALL)
            fc_emit(a, wide, o0 + k, x, y, n, au, av, ok);
    }
    if (!ALL)
        fc_emit(a, wide, o0, x, y, n, au, av, ok);
}

template <bool OCC, bool ALL>
void fc_launch_as(hipStream_t s, const FcArgs &a, const FcWide &wide) {
    hipLaunchKernelGGL((k_flow_chain<OCC, ALL>), fq_grid(a.w, a.h, a.anchors), dim3(256), 0, s, a, wide);
}

} // namespace

void fc_launch(hipStream_t s, const FcArgs &args) {
    if (args.anchors <= 0 || args.length <= 0 || args.w <= 0 || args.h <= 0)
        return;
    const bool all = args.emit == FC_ALL;
    // a lane's 4 elements in one access: the base and every stride a multiple of that access
    FcWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.occ = dfx_bytes4(args.occ, args.occ_pitch, args.occ_stride);
    wide.out = dfx_planar_vec(args.out, args.out_stride, args.out_plane, args.out_pitch) == 4;
    wide.valid = dfx_bytes4(args.valid, args.valid_pitch, args.valid_stride);
    wide.pair = FC_PAIR_TAPS && args.w >= 2;
    // grid.z holds at most FQ_ITEMS_MAX = 65535 anchors: more than that go in several launches
    const int chunk = FQ_ITEMS_MAX;
    const long long per = all ? args.length : 1; // output flows per anchor
    for (int j0 = 0; j0 < args.anchors; j0 += chunk) {
        FcArgs a = args;
        a.anchors = std::min(chunk, args.anchors - j0);
        a.first = (int)(args.first + (long long)j0 * args.anchor_step);
        a.out += (long long)j0 * per * args.out_stride;
        if (a.valid)
            a.valid += (long long)j0 * per * args.valid_stride;
        if (args.occ) {
            if (all)
                fc_launch_as<true, true>(s, a, wide);
            else
                fc_launch_as<true, false>(s, a, wide);
        } else {
            if (all)
                fc_launch_as<false, true>(s, a, wide);
            else
                fc_launch_as<false, false>(s, a, wide);
        }
    }
}
