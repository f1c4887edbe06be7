// flow_hist_kernels.hip — motion descriptors of flows on the device: per spatial cell the orientation histogram of the flow (HOF)
// and of the spatial derivatives of u and of v (MBHx, MBHy), Dalal et al. 2006 and the descriptors of Wang et al.'s dense
// trajectories.  The arithmetic is section (0.5.2) of include/dfx.h, float32, every operation rounded on its own (the build's
// -ffp-contract=off), the normalisation float64; tests/flow_hist_ref.py is the same text in NumPy and the two agree exactly in
// the integer sums and bit for bit in the float values.
//
// One launch does everything.  A workgroup is the lane quad of flow_quad.h, 256 threads on 256 pixels of a row, 4 pixels per
// lane, and walks `bands` bands of `cell` rows; 256 and the band's height are multiples of the cell, so the workgroup owns the
// 256 / cell cells of a band whole and nothing leaves it through an atomic on global memory.  Per band:
//   accumulate : wave w takes the cell / 4 rows w * cell / 4 .. of the band, top to bottom.  With MBH it holds three rows
//                (y - 1, y, y + 1, clamped) in registers and rolls them, so a band of R rows per wave costs R + 2 row loads per
//                plane and not 3 R; x - 1 and x + 4 come from the neighbouring lanes (one cross-lane move each), lanes 0 and 63
//                load theirs from memory.  A quad's 4 pixels lie in one cell: runs of pixels with the same first slot are
//                added up in registers and go to LDS as one 64-bit atomic add per slot, zero weights as none.
//   normalise  : (norm != NONE) thread t < cells * channels forms T or sqrt(E) of one cell and channel in float64 into LDS.
//   store      : thread t takes the words t, t + 256, .. of the band's cells — the order they have in d_sums, so those stores
//                are contiguous — stores the sum and / or the float value, and clears the word for the next band.
// LDS: 64 cells x 49 slots x 8 bytes = 25088 bytes of sums + 64 x 3 x 8 = 1536 bytes of denominators.  No scratch, no global
// atomics, no workspace, no zeroing pass.  Bytes per pixel: 8 read (+ 1 of mask), times (R + 2) / R with MBH, from L2 for the
// two extra rows where the neighbouring wave or band has just read them.
//
// Why no address can leave its range, for every bit pattern of the inputs:
//   - a pixel's u, v reach the arithmetic only where it is known (unmasked, |u|, |v| <= 1e9: false for NaN and both
//     infinities); otherwise they are replaced by 0 at the load, so every gx, gy is finite (at most 2e9 in magnitude), m is
//     finite, and atan2_turns of finite arguments is finite;
//   - the slot k0 is nevertheless clamped as an unsigned integer to bins - 1 (a no-op under the text: a is in [-1, 1], so fk
//     is in [0, bins] and bins wraps to 0), the still slot is the constant `bins` and is formed in the HOF channel only, and k1
//     is formed from the clamped k0: every slot is below its channel's length, every channel ends at or below D <= 49;
//   - the cell of a lane is (lane * 4) / cell < 64, a function of the lane alone: LDS words are below 64 * D <= 3136;
//   - rows are clamped to 0 .. H - 1 and columns to 0 .. W - 1 before they form an address; lanes right of the image load
//     nothing; the store phase runs over cells * D words with cx0 + cells <= CW and cy < CH.
#include "flow_hist_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_angle.h"
#include "flow_quad.h"

namespace {

constexpr int FH_CELLS = 64;    // cells of a band in a workgroup, at most: 256 / 4
constexpr int FH_WG_ROWS = 32;  // rows a workgroup walks: 32 / cell bands

// one row of a lane: its 4 pixels and the pixels left and right of them (x - 1 and x + 4, from memory in lanes 0 and 63
// only), unknown pixels and those outside the row as (0, 0), not known
struct FhRow {
    float u[4], v[4];
    bool kn[4];
    float ue[2], ve[2]; // [0]: x - 1, [1]: x + 4
    bool ke[2];
};

__device__ __forceinline__ bool fh_known(unsigned m, float u, float v) {
    return m == 0u && __builtin_fabsf(u) <= 1e9f && __builtin_fabsf(v) <= 1e9f; // false for NaN and for either infinity
}

// row y (0 <= y < h) of flow i.  EDGES: also x - 1 / x + 4 in lanes 0 / 63 where they lie inside the row.
template <bool MASKED, bool EDGES>
__device__ __forceinline__ void fh_load_row(const FhArgs &a, long long i, int x, int y, int n, int lane, FhRow &r) {
    unsigned m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r.u[k] = r.v[k] = 0.0f, m[k] = 0u;
    const float *pu = a.flow + i * a.flow_stride + (long long)y * a.row_pitch;
    const unsigned char *pm = MASKED ? a.mask + i * a.mask_stride + (long long)y * a.mask_pitch : nullptr;
    if (n > 0) {
        fq_load_flow(pu + x, a.plane_stride, a.wide_flow != 0, n, r.u, r.v);
        if (MASKED)
            fq_load_u8(pm + x, a.wide_mask != 0, n, m);
    }
    float ue[2] = {0.0f, 0.0f}, ve[2] = {0.0f, 0.0f};
    unsigned me[2] = {1u, 1u};
    if (EDGES) {
        if (lane == 0 && x > 0 && x - 1 < a.w) {
            ue[0] = pu[x - 1], ve[0] = pu[a.plane_stride + x - 1];
            me[0] = MASKED ? pm[x - 1] : 0u;
        }
        if (lane == 63 && x + 4 < a.w) {
            ue[1] = pu[x + 4], ve[1] = pu[a.plane_stride + x + 4];
            me[1] = MASKED ? pm[x + 4] : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.kn[k] = k < n && fh_known(m[k], r.u[k], r.v[k]);
        r.u[k] = r.kn[k] ? r.u[k] : 0.0f;
        r.v[k] = r.kn[k] ? r.v[k] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        r.ke[e] = fh_known(me[e], ue[e], ve[e]);
        r.ue[e] = r.ke[e] ? ue[e] : 0.0f;
        r.ve[e] = r.ke[e] ? ve[e] : 0.0f;
    }
}

// the text's binning of one finite vector: first slot k0 < bins and the two weights, which add up to Q; *m is its magnitude
__device__ __forceinline__ void fh_bin(float gx, float gy, int bins, float hb, float fb, int &k0, long long &w0, long long &w1,
                                       float &m) {
    m = sqrtf(gx * gx + gy * gy);
    const float ang = fv_atan2_turns(gy, gx);
    const long long Q = (long long)rintf(m * 256.0f);
    float fk = ang * hb;
    if (fk < 0.0f)
        fk = fk + fb;
    const float fl = floorf(fk);
    int k = (int)fl;
    float f = fk - fl;
    if (k == bins)
        k = 0, f = 0.0f;
    k0 = (int)min((unsigned)k, (unsigned)(bins - 1)); // a no-op under the text; the LDS address does not rest on that
    const int F = (int)rintf(f * 256.0f);
    w1 = (Q * (long long)F + 128) >> 8;
    w0 = Q - w1;
}

// w0 to slot k of a channel's words, w1 to the slot after it (k < bins), or w0 alone to the still slot (k == bins, w1 == 0)
__device__ __forceinline__ void fh_flush(unsigned long long *chan, int bins, int k, long long w0, long long w1) {
    if (w0)
        atomicAdd(chan + k, (unsigned long long)w0);
    if (w1)
        atomicAdd(chan + (k + 1 >= bins ? 0 : k + 1), (unsigned long long)w1);
}

// the 4 pixels of a lane into one channel of their cell: runs of equal first slots as one pair of adds
template <bool STILL>
__device__ __forceinline__ void fh_add(unsigned long long *chan, int bins, float hb, float fb, float thr, const float (&gx)[4],
                                       const float (&gy)[4], const bool (&part)[4]) {
    int k[4];
    long long w0[4], w1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float m;
        fh_bin(gx[j], gy[j], bins, hb, fb, k[j], w0[j], w1[j], m);
        if (STILL && m <= thr)
            k[j] = bins, w0[j] = 256, w1[j] = 0;
        if (!part[j])
            w0[j] = 0, w1[j] = 0;
    }
    int ck = k[0];
    long long c0 = w0[0], c1 = w1[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        if (k[j] == ck || (w0[j] | w1[j]) == 0) { // nothing to add joins any run
            c0 += w0[j], c1 += w1[j];
        } else {
            fh_flush(chan, bins, ck, c0, c1);
            ck = k[j], c0 = w0[j], c1 = w1[j];
        }
    }
    fh_flush(chan, bins, ck, c0, c1);
}

// KINDS: FH_KIND_* bits; MASKED: with mask planes.  grid: (ceil(w / 256), ceil(CH / bands), flows).
template <int KINDS, bool MASKED>
__global__ __launch_bounds__(256) void k_flow_hist(FhArgs a) {
    constexpr bool HOF = (KINDS & FH_KIND_HOF) != 0, MBX = (KINDS & FH_KIND_MBHX) != 0, MBY = (KINDS & FH_KIND_MBHY) != 0;
    constexpr bool MBH = MBX || MBY;
    constexpr int NCH = (HOF ? 1 : 0) + (MBX ? 1 : 0) + (MBY ? 1 : 0);
    __shared__ unsigned long long acc[FH_CELLS * FH_MAX_SLOTS];
    __shared__ double den[FH_CELLS * 3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = fq_x();
    const int n = min(4, a.w - x); // <= 0 in lanes right of the image
    const long long i = (long long)a.i0 + (long long)blockIdx.z;
    const int bins = a.bins, D = a.d;
    const float fb = (float)bins, hb = 0.5f * fb;
    const int R = a.cell >> 2; // rows of a band per wave
    const int per = 256 >> a.cell_log2;
    const int cx0 = (int)blockIdx.x * per;
    const int cells = min(per, a.cw - cx0);
    const int words = cells * D;
    // the channels' first slots and lengths
    const int len0 = HOF ? bins + 1 : bins;
    const int base1 = len0, base2 = len0 + bins;
    const int bx = MBX ? (HOF ? base1 : 0) : 0, by = MBY ? (NCH == 3 ? base2 : NCH == 2 ? base1 : 0) : 0;

    for (int t = tid; t < FH_CELLS * D; t += 256)
        acc[t] = 0ull;
    __syncthreads();
    unsigned long long *mine = acc + ((lane * 4) >> a.cell_log2) * D; // the lane's cell: below 64

    for (int b = 0; b < a.bands; ++b) {
        const int cy = (int)blockIdx.y * a.bands + b;
        if (cy >= a.ch) // the same in every thread
            break;
        const int y0 = cy * a.cell + wave * R;
        if (y0 < a.h) { // wave-uniform: the cross-lane moves below have all 64 lanes
            FhRow prev, cur, next;
            fh_load_row<MASKED, MBH>(a, i, x, y0, n, lane, cur);
            if (MBH)
                fh_load_row<MASKED, false>(a, i, x, max(y0 - 1, 0), n, lane, prev);
            for (int r = 0; r < R; ++r) {
                const int y = y0 + r;
                if (y >= a.h)
                    break;
                if (HOF)
                    fh_add<true>(mine, bins, hb, fb, a.still_thr, cur.u, cur.v, cur.kn);
                if (MBH) {
                    fh_load_row<MASKED, MBH>(a, i, x, min(y + 1, a.h - 1), n, lane, next);
                    // x - 1 of pixel 0 and x + 1 of pixel 3: the neighbouring lanes' pixels 3 and 0, memory in lanes 0 and 63
                    float ul = __shfl_up(cur.u[3], 1), vl = __shfl_up(cur.v[3], 1);
                    float ur = __shfl_down(cur.u[0], 1), vr = __shfl_down(cur.v[0], 1);
                    bool kl = __shfl_up((int)cur.kn[3], 1) != 0, kr = __shfl_down((int)cur.kn[0], 1) != 0;
                    if (lane == 0)
                        ul = cur.ue[0], vl = cur.ve[0], kl = cur.ke[0];
                    if (lane == 63)
                        ur = cur.ue[1], vr = cur.ve[1], kr = cur.ke[1];
                    float gxu[4], gyu[4], gxv[4], gyv[4];
                    bool part[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        // the clamped columns: pixel 0 of the row is its own left neighbour, pixel W - 1 its own right one
                        const bool first = x + k == 0, last = x + k + 1 >= a.w;
                        const float lu = first ? cur.u[k] : (k == 0 ? ul : cur.u[k > 0 ? k - 1 : 0]);
                        const float lv = first ? cur.v[k] : (k == 0 ? vl : cur.v[k > 0 ? k - 1 : 0]);
                        const bool lk = first ? cur.kn[k] : (k == 0 ? kl : cur.kn[k > 0 ? k - 1 : 0]);
                        const float ru = last ? cur.u[k] : (k == 3 ? ur : cur.u[k < 3 ? k + 1 : 3]);
                        const float rv = last ? cur.v[k] : (k == 3 ? vr : cur.v[k < 3 ? k + 1 : 3]);
                        const bool rk = last ? cur.kn[k] : (k == 3 ? kr : cur.kn[k < 3 ? k + 1 : 3]);
                        part[k] = cur.kn[k] && lk && rk && prev.kn[k] && next.kn[k];
                        gxu[k] = ru - lu, gyu[k] = next.u[k] - prev.u[k];
                        gxv[k] = rv - lv, gyv[k] = next.v[k] - prev.v[k];
                    }
                    if (MBX)
                        fh_add<false>(mine + bx, bins, hb, fb, 0.0f, gxu, gyu, part);
                    if (MBY)
                        fh_add<false>(mine + by, bins, hb, fb, 0.0f, gxv, gyv, part);
                    prev = cur;
                    cur = next;
                } else if (r + 1 < R && y + 1 < a.h) {
                    fh_load_row<MASKED, false>(a, i, x, y + 1, n, lane, cur);
                }
            }
        }
        __syncthreads();
        if (a.out && a.norm != FH_NORM_NONE) {
            if (tid < cells * NCH) {
                const int c = tid / NCH, chn = tid - c * NCH;
                const int base = chn == 0 ? 0 : chn == 1 ? base1 : base2;
                const int len = chn == 0 ? len0 : bins;
                const unsigned long long *s = acc + c * D + base;
                double dv;
                if (a.norm == FH_NORM_L2) {
                    double E = 0.0;
                    for (int k = 0; k < len; ++k) {
                        const double sv = (double)(long long)s[k];
                        E = E + sv * sv;
                    }
                    dv = sqrt(E);
                } else {
                    long long T = 0;
                    for (int k = 0; k < len; ++k)
                        T += (long long)s[k];
                    dv = (double)T;
                }
                den[c * 3 + chn] = dv;
            }
            __syncthreads();
        }
        for (int t = tid; t < words; t += 256) {
            const long long S = (long long)acc[t];
            acc[t] = 0ull;
            if (a.sums)
                a.sums[i * a.sums_stride + ((long long)cy * a.cw + cx0) * D + t] = S;
            if (a.out) {
                const int c = t / D, slot = t - c * D;
                const int chn = slot < base1 ? 0 : slot < base2 ? 1 : 2;
                const double sv = (double)S;
                double val;
                if (a.norm == FH_NORM_NONE) {
                    val = sv / 256.0;
                } else {
                    const double dv = den[c * 3 + chn];
                    val = dv > 0.0 ? sv / dv : 0.0;
                    if (a.norm == FH_NORM_L1_SQRT)
                        val = sqrt(val);
                }
                a.out[i * a.out_flow + (long long)slot * a.out_slot + (long long)cy * a.out_row + (long long)(cx0 + c) * a.out_col] =
                    (float)val;
            }
        }
        __syncthreads();
    }
}

template <int KINDS>
void fh_launch_as(hipStream_t s, const dim3 &grid, const FhArgs &a) {
    if (a.mask)
        hipLaunchKernelGGL((k_flow_hist<KINDS, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_flow_hist<KINDS, false>), grid, dim3(256), 0, s, a);
}

} // namespace

void fh_launch(hipStream_t s, const FhArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    FhArgs a = args;
    a.cell_log2 = a.cell == 4 ? 2 : a.cell == 8 ? 3 : a.cell == 16 ? 4 : 5;
    a.cw = (a.w + a.cell - 1) / a.cell, a.ch = (a.h + a.cell - 1) / a.cell;
    a.d = fh_slots(a.kinds, a.bins);
    a.bands = FH_WG_ROWS / a.cell;
    // a lane's 4 elements in one access: the base and every stride a multiple of that access
    a.wide_flow = dfx_planar_vec(a.flow, a.flow_stride, a.plane_stride, a.row_pitch) == 4;
    a.wide_mask = dfx_bytes4(a.mask, a.mask_pitch, a.mask_stride, 0);
    const dim3 grid0((unsigned)((a.w + 255) / 256), (unsigned)((a.ch + a.bands - 1) / a.bands), 1);
    // grid.z holds at most FQ_ITEMS_MAX = 65535 flows: more than that go in several launches
    const int chunk = FQ_ITEMS_MAX;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        a.i0 = i0;
        const dim3 grid(grid0.x, grid0.y, (unsigned)std::min(chunk, args.n - i0));
        switch (a.kinds) {
        case 1: fh_launch_as<1>(s, grid, a); break;
        case 2: fh_launch_as<2>(s, grid, a); break;
        case 3: fh_launch_as<3>(s, grid, a); break;
        case 4: fh_launch_as<4>(s, grid, a); break;
        case 5: fh_launch_as<5>(s, grid, a); break;
        case 6: fh_launch_as<6>(s, grid, a); break;
        default: fh_launch_as<7>(s, grid, a); break;
        }
    }
}
