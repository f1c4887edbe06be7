// global_motion_kernels.hip — how much of a flow is the camera, and what the flow is without it: per flow a robust fit of
// the dominant motion (a translation or a 6-parameter affine map), the flow with that motion removed (the "warped flow" of
// the TSN line of work), and the mask of the pixels that do not follow it.  include/dfx.h (dfx_global_motion_device) states
// the arithmetic; tests/global_motion_ref.py is the same text in NumPy; the two agree bit for bit.  In short, per flow:
//     xc = 2x - (W-1), yc = 2y - (H-1)                         doubled, centred integer coordinates
//     ok = |u| < 4096 && |v| < 4096 && (no mask || mask == 0)  false for NaN and either infinity
//     round k: inlier = ok && (k == 0 || ru*ru + rv*rv <= t_k*t_k),  ru = u - ((p0 + p1*xf) + p2*yf), rv likewise (float32,
//              every operation rounded on its own: the build's -ffp-contract=off), p the model of round k - 1
//     twelve int64 sums over the inliers of 1, xc, yc, xc^2, xc yc, yc^2 and of q, xc q, yc q for q = (int)rintf(u * 256)
//     and (int)rintf(v * 256); a closed-form solve in float64 (one lane); p = (float)P
// The sums are integers so that they do not depend on the order in which 272 workgroups (1080p) add them: a float
// reduction by atomics would give another model on every run, and the inlier set of the next round with it.
//
// k_gm_accumulate<model, first_round> is one round, on the lane quad of flow_quad.h.  A workgroup walks a
// band of GM_BAND_ROWS rows at fixed columns, wave w the rows w, w + 4, ..: a lane's four columns never change, so it keeps
// per column only the 32-bit count, sum of yc, sum of qu and sum of qv of its at most 8 rows (|q| <= 2^20: below 2^23), and
// over its columns together the sums of yc^2 (32-bit: 32 terms below 2^26), yc*qu and yc*qv (64-bit, one 32 x 32 -> 64
// multiply-add per row, not per pixel); the x moments are those partials times xc, once after the loop.  The twelve
// 64-bit words are reduced across the wave by __shfl_xor, across the four waves through 384 bytes of LDS, and lanes 0 .. 11
// issue one 64-bit agent-scope atomic add each (none for a zero) on the record's working words.  Then the workgroup takes the
// flow's ticket with the protocol of end_segment_tile (tvl1_device_common.h): the adding wave drains its memory counter,
// one lane takes the ticket by an agent-scope atomic, and the flow's last arriver reads the twelve words with agent-scope
// 8-byte atomic loads (8-byte agent atomics on both sides: nothing depends on dispatch order or on the XCD a workgroup runs
// on).  That lane solves, writes p, a, inliers[k] and status, copies the sums out, and zeroes the working words and the
// ticket for the next round, which is the next launch on the stream: no host synchronisation between rounds.
// k_gm_apply subtracts the final model from every pixel and writes the mask; a lane reads its four pixels before it writes
// them, so out may be the flow itself.  No scratch; the accumulate kernel keeps registers for six waves per SIMD, the apply
// kernel for eight.
// Bytes per pixel: 8 of flow (+ 1 of mask) per round; the apply pass 8 (+ 1) read, 8 of out and 1 of moving written.
#include "global_motion_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

namespace {

#define GM_AGENT __HIP_MEMORY_SCOPE_AGENT

// which accesses take a lane's 4 elements at once; one value per call, so every branch on them is wave-uniform
struct GmWide {
    int flow, mask, out, moving;
};

struct GmQuad {
    float u[4], v[4];
    unsigned ok[4]; // 0 beyond the row's end
};

// the 4 pixels (x .. x + 3, y) of flow i: the values and the ok test
__device__ __forceinline__ void gm_load(const GmArgs &a, const GmWide &wide, int x, int y, long long i, GmQuad &q) {
    const int n = fq_count(a.w, x);
    fq_load_flow(a.flow + i * a.flow_stride + (long long)y * a.row_pitch + x, a.plane_stride, wide.flow != 0, n, q.u, q.v);
#pragma unroll
    for (int k = 0; k < 4; ++k) // false for NaN and for either infinity
        q.ok[k] = (k < n && __builtin_fabsf(q.u[k]) < 4096.0f && __builtin_fabsf(q.v[k]) < 4096.0f) ? 1u : 0u;
    if (a.mask)
        fq_mask_clear(a.mask + i * a.mask_stride + (long long)y * a.mask_pitch + x, wide.mask != 0, n, q.ok);
}

struct GmModel {
    float p[6];
};

// the residual of one pixel against the model, every operation on its own
__device__ __forceinline__ void gm_residual(const GmModel &m, float u, float v, float xf, float yf, float &ru, float &rv) {
    ru = u - ((m.p[0] + m.p[1] * xf) + m.p[2] * yf);
    rv = v - ((m.p[3] + m.p[4] * xf) + m.p[5] * yf);
}

// One lane, once per flow and round: the solve of include/dfx.h in float64, every operation on its own, in its order.
template <int MODEL>
__device__ __forceinline__ void gm_close_round(dfx_gm_result *r, const long long (&s)[GM_SUMS], int round, int rounds, int w,
                                               int h, bool first) {
    const double S1 = (double)s[0], Sx = (double)s[1], Sy = (double)s[2], Sxx = (double)s[3], Sxy = (double)s[4];
    const double Syy = (double)s[5], Su = (double)s[6], Sxu = (double)s[7], Syu = (double)s[8], Sv = (double)s[9];
    const double Sxv = (double)s[10], Syv = (double)s[11];
    double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool degenerate;
    if (MODEL == GM_TRANSLATION) {
        degenerate = S1 < 1.0;
        if (!degenerate) {
            P[0] = Su / S1 / 256.0;
            P[3] = Sv / S1 / 256.0;
        }
    } else {
        const double c00 = Sxx * Syy - Sxy * Sxy;
        const double c01 = Sy * Sxy - Sx * Syy;
        const double c02 = Sx * Sxy - Sy * Sxx;
        const double c11 = S1 * Syy - Sy * Sy;
        const double c12 = Sx * Sy - S1 * Sxy;
        const double c22 = S1 * Sxx - Sx * Sx;
        const double det = (S1 * c00 + Sx * c01) + Sy * c02;
        degenerate = S1 < 3.0 || !(det > 0.0);
        if (!degenerate) {
            const double d = det * 256.0;
            P[0] = ((c00 * Su + c01 * Sxu) + c02 * Syu) / d;
            P[1] = ((c01 * Su + c11 * Sxu) + c12 * Syu) / d;
            P[2] = ((c02 * Su + c12 * Sxu) + c22 * Syu) / d;
            P[3] = ((c00 * Sv + c01 * Sxv) + c02 * Syv) / d;
            P[4] = ((c01 * Sv + c11 * Sxv) + c12 * Syv) / d;
            P[5] = ((c02 * Sv + c12 * Sxv) + c22 * Syv) / d;
        }
    }
    if (degenerate) { // the previous model stays (all zero before round 0: the record was zeroed)
        r->status |= 1u << round;
    } else {
        const double wm = (double)(w - 1), hm = (double)(h - 1);
#pragma unroll
        for (int o = 0; o < 6; o += 3) {
            r->a[o] = (P[o] - P[o + 1] * wm) - P[o + 2] * hm;
            r->a[o + 1] = 2.0 * P[o + 1];
            r->a[o + 2] = 2.0 * P[o + 2];
        }
#pragma unroll
        for (int j = 0; j < 6; ++j)
            r->p[j] = (float)P[j];
    }
    r->inliers[round] = (uint64_t)s[0];
    if (first) {
        r->valid = (uint64_t)s[0];
        r->rounds = (uint32_t)rounds;
    }
#pragma unroll
    for (int j = 0; j < GM_SUMS; ++j)
        r->sums[j] = s[j];
}

// One round of flow blockIdx.z.  grid: (ceil(w / 256), ceil(h / GM_BAND_ROWS), flows).  tt = t_k * t_k.  The twelve 64-bit words
// of the reduction on top of the loop's partials need 76 registers: compiled for 80 (six waves per SIMD), never spilling.
template <int MODEL, bool FIRST>
__global__ __launch_bounds__(256, 6) void k_gm_accumulate(GmArgs a, GmWide wide, int round, float tt) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int x = fq_x();
    const long long i = (long long)blockIdx.z;
    dfx_gm_result *res = a.result + i;
    GmModel m;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        m.p[j] = FIRST ? 0.0f : res->p[j]; // written by the launch before this one
    int c[4] = {0, 0, 0, 0}, sy[4] = {0, 0, 0, 0}, su[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};
    unsigned syy = 0u;
    long long syu = 0, syv = 0;
    float xf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        xf[k] = (float)(2 * (x + k) - (a.w - 1));
#pragma unroll 1
    for (int g = 0; g < GM_BAND_ROWS / 4; ++g) {
        const int y = fq_y(GM_BAND_ROWS, g);
        if (x < a.w && y < a.h) {
            GmQuad q;
            gm_load(a, wide, x, y, i, q);
            const int yc = 2 * y - (a.h - 1);
            const float yf = (float)yc;
            int rc = 0, rqu = 0, rqv = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool in = q.ok[k] != 0u;
                if (!FIRST) {
                    float ru, rv;
                    gm_residual(m, q.u[k], q.v[k], xf[k], yf, ru, rv);
                    in = in && ru * ru + rv * rv <= tt;
                }
                // an excluded pixel's value may be NaN or huge: converted only where it counts
                const int qu = in ? (int)rintf(q.u[k] * 256.0f) : 0, qv = in ? (int)rintf(q.v[k] * 256.0f) : 0;
                const int one = in ? 1 : 0;
                c[k] += one, sy[k] += in ? yc : 0, su[k] += qu, sv[k] += qv;
                rc += one, rqu += qu, rqv += qv;
            }
            syy += (unsigned)(yc * yc) * (unsigned)rc;
            syu += (long long)yc * (long long)rqu;
            syv += (long long)yc * (long long)rqv;
        }
    }
    long long v[GM_SUMS];
#pragma unroll
    for (int j = 0; j < GM_SUMS; ++j)
        v[j] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { // all zero for the lanes beyond the row's end
        const long long xc = (long long)(2 * (x + k) - (a.w - 1));
        v[0] += c[k], v[1] += xc * c[k], v[2] += sy[k], v[3] += xc * xc * c[k], v[4] += xc * sy[k];
        v[6] += su[k], v[7] += xc * su[k], v[9] += sv[k], v[10] += xc * sv[k];
    }
    v[5] = (long long)syy, v[8] = syu, v[11] = syv;
#pragma unroll
    for (int j = 0; j < GM_SUMS; ++j) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
            v[j] += __shfl_xor(v[j], s);
    }
    __shared__ long long part[4][GM_SUMS];
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < GM_SUMS; ++j)
            part[wave][j] = v[j];
    }
    __syncthreads();
    if (wave != 0)
        return;
    unsigned long long *work = reinterpret_cast<unsigned long long *>(res->work);
    if (lane < GM_SUMS) {
        const long long t = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
        if (t != 0)
            (void)__hip_atomic_fetch_add(work + lane, (unsigned long long)t, __ATOMIC_RELAXED, GM_AGENT);
    }
    // the adds are at the device's coherence point before the ticket is taken
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane != 0)
        return;
    const unsigned long long nblk = (unsigned long long)gridDim.x * gridDim.y;
    const unsigned long long old = __hip_atomic_fetch_add(work + GM_SUMS, 1ull, __ATOMIC_RELAXED, GM_AGENT);
    if (old != nblk - 1ull)
        return;
    asm volatile("" ::: "memory");
    long long s[GM_SUMS];
#pragma unroll
    for (int j = 0; j < GM_SUMS; ++j)
        s[j] = (long long)__hip_atomic_load(work + j, __ATOMIC_RELAXED, GM_AGENT);
    gm_close_round<MODEL>(res, s, round, a.rounds, a.w, a.h, FIRST);
#pragma unroll
    for (int j = 0; j <= GM_SUMS; ++j) // the next round starts from zero sums and a zero ticket
        __hip_atomic_store(work + j, 0ull, __ATOMIC_RELAXED, GM_AGENT);
}

// The flow minus the final model, and the pixels that do not follow it.  grid: (ceil(w / 256), ceil(h / 4), flows).
__global__ __launch_bounds__(256, 8) void k_gm_apply(GmArgs a, GmWide wide, float tt) {
    const int x = fq_x(), y = fq_y();
    const long long i = (long long)blockIdx.z;
    if (x >= a.w || y >= a.h)
        return;
    GmModel m;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        m.p[j] = a.result[i].p[j];
    GmQuad q;
    gm_load(a, wide, x, y, i, q);
    const int n = fq_count(a.w, x);
    const float yf = (float)(2 * y - (a.h - 1));
    float ru[4], rv[4];
    unsigned mv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        gm_residual(m, q.u[k], q.v[k], (float)(2 * (x + k) - (a.w - 1)), yf, ru[k], rv[k]);
        mv[k] = (q.ok[k] != 0u && ru[k] * ru[k] + rv[k] * rv[k] <= tt) ? 0u : 1u;
    }
    if (a.out)
        fq_store_flow(a.out + i * a.out_stride + (long long)y * a.out_pitch + x, a.out_plane, wide.out != 0, n, ru, rv);
    if (a.moving)
        fq_store_u8(a.moving + i * a.moving_stride + (long long)y * a.moving_pitch + x, wide.moving != 0, n, mv);
}

template <int MODEL>
void gm_round(hipStream_t s, const GmArgs &a, const GmWide &wide, dim3 grid, int round, float tt) {
    if (round == 0)
        hipLaunchKernelGGL((k_gm_accumulate<MODEL, true>), grid, dim3(256), 0, s, a, wide, round, tt);
    else
        hipLaunchKernelGGL((k_gm_accumulate<MODEL, false>), grid, dim3(256), 0, s, a, wide, round, tt);
}

} // namespace

void gm_launch(hipStream_t s, const GmArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    GmWide wide;
    wide.flow = dfx_planar_vec(args.flow, args.flow_stride, args.plane_stride, args.row_pitch) == 4;
    wide.mask = dfx_bytes4(args.mask, args.mask_pitch, args.mask_stride);
    wide.out = args.out && dfx_planar_vec(args.out, args.out_stride, args.out_plane, args.out_pitch) == 4;
    wide.moving = dfx_bytes4(args.moving, args.moving_pitch, args.moving_stride);
    (void)hipMemsetAsync(args.result, 0, (size_t)args.n * sizeof(dfx_gm_result), s);
    // t_k = thr multiplied rounds - 1 - k times by growth, in float32
    float tt[GM_MAX_ROUNDS];
    for (int k = 0; k < args.rounds; ++k) {
        float t = args.thr;
        for (int j = 0; j < args.rounds - 1 - k; ++j)
            t = t * args.growth;
        tt[k] = t * t;
    }
    // grid.z holds at most FQ_ITEMS_MAX = 65535 flows: more than that go in several launches
    const int chunk = FQ_ITEMS_MAX;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        GmArgs a = args;
        a.n = std::min(chunk, args.n - i0);
        a.flow += (long long)i0 * args.flow_stride;
        a.result += i0;
        if (a.mask)
            a.mask += (long long)i0 * args.mask_stride;
        if (a.out)
            a.out += (long long)i0 * args.out_stride;
        if (a.moving)
            a.moving += (long long)i0 * args.moving_stride;
        const dim3 grid = fq_grid(a.w, a.h, a.n, GM_BAND_ROWS);
        for (int k = 0; k < a.rounds; ++k) {
            if (a.model == GM_TRANSLATION)
                gm_round<GM_TRANSLATION>(s, a, wide, grid, k, tt[k]);
            else
                gm_round<GM_AFFINE>(s, a, wide, grid, k, tt[k]);
        }
        if (a.out || a.moving)
            hipLaunchKernelGGL(k_gm_apply, fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide, args.thr * args.thr);
    }
}
