// interpolate_kernels.hip — the frame at time t between two frames, from the frames and their flows, on the device: what the
// projection, the fill and the warp were built for (Baker et al. 2011), in one call and with no intermediate leaving the
// workspace.
//
// All float operations are float32, each rounded on its own (the build's -ffp-contract=off), t1 = 1.0f - t.  Per pair:
//   1. project   (G0, H0) = the projection of F01 with t, scale -t, min_weight, occ_fwd: fp_launch's out and hole planes;
//                with F10: (G1, H1) = the projection of F10 with t1, scale -t1, occ_bwd;
//                without:  (G1, H1) = the projection of F01 with t, scale t1: the same sums normalised with a second scale
//                (fp_renormalise), so H1 = H0.
//   2. fill      (Gf_k, Hf_k) = (G_k, H_k) after fill_passes passes of fm_launch in FM_FILL, mask_out fed back as the mask.
//   3. synthesise, per output pixel (x, y) and side k, (gu, gv) = Gf_k(x, y):
//                px = (float)x + gu;  py = (float)y + gv;  inside_k and the bilinear sample s_k of I_k: the text of
//                warp_kernels.hip, word for word
//                prim_k = H_k == 0 && inside_k;   cand_k = Hf_k == 0 && inside_k
//                (w0, w1) = prim_0 || prim_1 ? (prim_0, prim_1) : (cand_0, cand_1)
//                o = s0 + t*(s1 - s0) (both) | s_k (only w_k) | P0 + t*(P1 - P0) (neither; P the pixel's own bytes)
//                o = fminf(fmaxf(o, 0), 255);  stored (uint8)rintf(o) or o
//                source = 0 both, 1 frame 0 only, 2 frame 1 only, 3 neither, + 4 where the second tier decided (never on 3)
// tests/interpolate_ref.py is the same text in NumPy; the device equals it bit for bit.
//
// Workspace of a wave of k pairs, every region 16-byte aligned, rows of the planes WP = round_up(W, 4) apart so that a
// lane's 4 pixels are one aligned access whatever W is (the padding columns are read and never used):
//   sums   k x W x H x 3 64-bit words: the two projections of a wave use them one after the other
//   GA     2k flows (flow 2 i + k of pair i, side k), planar: the projections' out; GB its ping-pong twin (fill_passes > 0)
//   H      2k hole planes; MA (fill_passes > 0), MB (fill_passes > 1): the masks the fill passes hand on
// so every fill pass is one launch over 2k flows, and the synthesis reads Gf from GA or GB and Hf from H, MA or MB,
// whichever the last pass wrote.
//
// k_interp_synth: the lane quad, the tap and the segments of flow_quad.h, grid.z the pairs of the wave.  Per lane: four
// 16-byte loads (Gf_0, Gf_1: u and v), two 4-byte loads of H and, in the FILLED form only, two of Hf; up to 8 byte taps per
// channel (the displacement is unbounded: no tile to stage); the pixel's own bytes only where neither frame is usable; one
// store per output segment and one of source.
// No LDS, no barrier, no scratch.  Bytes per pixel: 16 of flow, 2 or 4 of masks, 2 .. 8 C of taps, C x elem of out, 1 of source.
#include "interpolate_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"
#include "flow_median_kernels.h"
#include "flow_project_kernels.h"

namespace {

static_assert(INTERP_OUT_U8 == FQ_ELEM_U8 && INTERP_OUT_F32 == DFX_ELEM_F32 && INTERP_TILE_W == 256 && INTERP_TILE_H == 4,
              "flow_quad.h");

struct IsArgs {
    const unsigned char *img0, *img1;
    const float *g;                   // Gf: flow 2 i + side of pair i
    const unsigned char *hole, *fill; // H and Hf: plane 2 i + side; fill is read by the FILLED form only
    void *out;
    unsigned char *source;
    int n, w, h, wp;
    int out_dtype, wide_out, wide_source;
    float t;
    long long img_pitch, img_plane, img_image;
    long long out_pitch, out_plane, out_image;
    long long source_pitch, source_stride;
};

// the bilinear samples of the 4 pixels (x .. x + 3, y) of one side at p + g(p), and bit k of the result: inside.  gu: the
// lane's 4 elements of Gf's u plane in the workspace, where rows are padded so that they are always one access.
template <int C, bool IL>
__device__ __forceinline__ unsigned is_sample(const IsArgs &a, const unsigned char *img, const float *gu, int x, int y, int n,
                                              float (&s)[4][C]) {
    float u[4], v[4];
    fq_load_flow(gu, (long long)a.wp * a.h, true, 4, u, v);
    unsigned in = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            s[k][c] = 0.0f;
        if (k < n) {
            const FqTap t = fq_tap((float)(x + k) + u[k], (float)y + v[k], a.w, a.h, FQ_BORDER_ZERO);
            if (t.inside) {
                in |= 1u << k;
                fq_sample_u8<C, IL>(img, a.img_pitch, a.img_plane, t, s[k]);
            }
        }
    }
    return in;
}

// C: channels; IL: interleaved (C == 3 only); FILLED: fill_passes > 0, the second tier exists.
// grid: fq_grid(w, h, pairs of the wave, INTERP_TILE_H)
template <int C, bool IL, bool FILLED>
__global__ __launch_bounds__(256, 4) void k_interp_synth(IsArgs a) {
    constexpr int XS = IL ? C : 1;
    const int x = fq_x(), y = fq_y(INTERP_TILE_H);
    if (x >= a.w || y >= a.h)
        return;
    const long long i = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    const long long pp = (long long)a.wp * a.h, at = (long long)y * a.wp + x;
    const unsigned char *i0 = a.img0 + i * a.img_image, *i1 = a.img1 + i * a.img_image;
    float s0[4][C], s1[4][C];
    const unsigned in0 = is_sample<C, IL>(a, i0, a.g + (2 * i) * 2 * pp + at, x, y, n, s0);
    const unsigned in1 = is_sample<C, IL>(a, i1, a.g + (2 * i + 1) * 2 * pp + at, x, y, n, s1);
    // the workspace's mask planes: always one access
    unsigned h0[4], h1[4], f0[4] = {0u, 0u, 0u, 0u}, f1[4] = {0u, 0u, 0u, 0u};
    fq_load_u8(a.hole + (2 * i) * pp + at, true, 4, h0);
    fq_load_u8(a.hole + (2 * i + 1) * pp + at, true, 4, h1);
    if constexpr (FILLED) {
        fq_load_u8(a.fill + (2 * i) * pp + at, true, 4, f0);
        fq_load_u8(a.fill + (2 * i + 1) * pp + at, true, 4, f1);
    }
    const long long cs = IL ? 1 : a.img_plane;
    float o[4][C];
    unsigned code[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ins0 = (in0 >> k) & 1u, ins1 = (in1 >> k) & 1u;
        const bool prim0 = h0[k] == 0u && ins0, prim1 = h1[k] == 0u && ins1;
        const bool first = prim0 || prim1;
        bool w0 = prim0, w1 = prim1;
        if (FILLED && !first) {
            w0 = f0[k] == 0u && ins0;
            w1 = f1[k] == 0u && ins1;
        }
        code[k] = w0 ? (w1 ? 0u : 1u) : (w1 ? 2u : 3u);
        if (FILLED && !first && (w0 || w1))
            code[k] += 4u;
        if (k < n && !w0 && !w1) {
            // neither frame is usable: the plain blend of the pixel's own bytes, read here only
            const long long own = (long long)y * a.img_pitch + (long long)(x + k) * XS;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const long long co = C == 1 ? 0 : c * cs;
                const float p0 = (float)i0[own + co], p1 = (float)i1[own + co];
                o[k][c] = p0 + a.t * (p1 - p0);
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
                o[k][c] = (w0 && w1) ? s0[k][c] + a.t * (s1[k][c] - s0[k][c]) : (w1 ? s1[k][c] : s0[k][c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
            o[k][c] = __builtin_fminf(__builtin_fmaxf(o[k][c], 0.0f), 255.0f);
    }
    if (a.source)
        fq_store_u8(a.source + i * a.source_stride + (long long)y * a.source_pitch + x, a.wide_source != 0, n, code);
    if (!a.out)
        return;
#pragma unroll
    for (int g = 0; g < C; ++g) { // the segments of flow_quad.h
        float sv[4];
        fq_segment<C, IL>(o, g, sv);
        const int m = fq_seg_count<C, IL>(g, n);
        if (m <= 0)
            continue;
        const long long to = i * a.out_image + (long long)y * a.out_pitch + fq_seg_offset<C, IL>(x, g, a.out_plane);
        fq_store_image(a.out, to, a.out_dtype, a.wide_out != 0, m, sv);
    }
}

template <int C, bool IL>
void is_launch_as(hipStream_t s, const IsArgs &a, bool filled) {
    const dim3 grid = fq_grid(a.w, a.h, a.n, INTERP_TILE_H);
    if (filled)
        hipLaunchKernelGGL((k_interp_synth<C, IL, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_interp_synth<C, IL, false>), grid, dim3(256), 0, s, a);
}

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// the byte sizes of the regions of a wave of k pairs, in the order they lie in: sums, GA, GB, H, MA, MB
struct InterpLayout {
    size_t sums, g, gb, hole, ma, mb;
    size_t total() const { return sums + g + gb + hole + ma + mb; }
};

InterpLayout interp_layout(int w, int h, int fill_passes, size_t k) {
    const size_t wp = ((size_t)w + 3) & ~(size_t)3, pp = wp * (size_t)h;
    InterpLayout l;
    l.sums = up16(k * (size_t)w * (size_t)h * FP_WORDS * sizeof(unsigned long long));
    l.g = up16(k * 2 * 2 * pp * sizeof(float));
    l.gb = fill_passes > 0 ? l.g : 0;
    l.hole = up16(k * 2 * pp);
    l.ma = fill_passes > 0 ? l.hole : 0;
    l.mb = fill_passes > 1 ? l.hole : 0;
    return l;
}

} // namespace

size_t interp_work_bytes(int w, int h, int fill_passes) {
    if (w <= 0 || h <= 0 || fill_passes < 0 || fill_passes > INTERP_MAX_PASSES)
        return 0;
    return interp_layout(w, h, fill_passes, 1).total() + 8; // + 8: the base is taken up to 16 bytes
}

void interp_launch(hipStream_t s, const InterpArgs &args) {
    const size_t per_pair = interp_work_bytes(args.w, args.h, args.fill_passes);
    if (args.n <= 0 || per_pair == 0 || args.work_bytes < per_pair)
        return;
    // grid.z holds at most FQ_ITEMS_MAX = 65535 flows: a wave's 2k flows go in one launch of every pass
    const int k = (int)std::min<size_t>(std::min<size_t>((size_t)args.n, args.work_bytes / per_pair), FQ_ITEMS_MAX / 2);
    const int w = args.w, h = args.h;
    const long long wp = (w + 3) & ~3, pp = wp * h;
    const InterpLayout l = interp_layout(w, h, args.fill_passes, (size_t)k);
    unsigned char *base = reinterpret_cast<unsigned char *>(((size_t)args.work + 15) & ~(size_t)15);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(base);
    float *ga = reinterpret_cast<float *>(base + l.sums), *gb = reinterpret_cast<float *>(base + l.sums + l.g);
    unsigned char *hole = base + l.sums + l.g + l.gb, *ma = hole + l.hole, *mb = ma + l.ma;
    const float t = args.t, t1 = 1.0f - t;
    const bool three = args.channels == 3, planes = three && args.planar != 0;
    const int eb = args.out_dtype == INTERP_OUT_U8 ? 1 : 4;
    for (int i0 = 0; i0 < args.n; i0 += k) {
        const int m = std::min(k, args.n - i0);
        // 1. the projections: side 0 into flow 2 i, side 1 into flow 2 i + 1 of GA and H
        FpArgs p{};
        p.flow = args.fwd + (long long)i0 * args.flow_stride;
        p.occ = args.occ_fwd ? args.occ_fwd + (long long)i0 * args.occ_stride : nullptr;
        p.out = ga, p.hole = hole, p.work = sums;
        p.n = m, p.w = w, p.h = h;
        p.t = t, p.sc = (double)(-t) / 256.0;
        p.wmin = fp_wmin(args.min_weight);
        p.row_pitch = args.row_pitch, p.plane_stride = args.plane_stride, p.flow_stride = args.flow_stride;
        p.occ_pitch = args.occ_pitch, p.occ_stride = args.occ_stride;
        p.out_pitch = wp, p.out_plane = pp, p.out_stride = 4 * pp;
        p.hole_pitch = wp, p.hole_stride = 2 * pp;
        fp_launch(s, p, m);
        if (args.bwd) {
            p.flow = args.bwd + (long long)i0 * args.flow_stride;
            p.occ = args.occ_bwd ? args.occ_bwd + (long long)i0 * args.occ_stride : nullptr;
            p.out = ga + 2 * pp, p.hole = hole + pp;
            p.t = t1, p.sc = (double)(-t1) / 256.0;
            fp_launch(s, p, m);
        } else {
            p.out = ga + 2 * pp, p.hole = hole + pp;
            p.sc = (double)t1 / 256.0;
            fp_renormalise(s, p);
        }
        // 2. the fill: every pass one launch over the wave's 2 m flows
        float *src = ga, *dst = gb;
        unsigned char *mask = hole, *mask_out = ma;
        for (int pass = 0; pass < args.fill_passes; ++pass) {
            FmArgs f{};
            f.flow = src, f.mask = mask, f.out = dst, f.mask_out = mask_out;
            f.n = 2 * m, f.w = w, f.h = h;
            f.ksize = args.ksize, f.mode = FM_FILL;
            f.row_pitch = wp, f.plane_stride = pp, f.flow_stride = 2 * pp;
            f.mask_pitch = wp, f.mask_stride = pp;
            f.out_pitch = wp, f.out_plane = pp, f.out_stride = 2 * pp;
            f.mask_out_pitch = wp, f.mask_out_stride = pp;
            fm_launch(s, f);
            std::swap(src, dst);
            mask = mask_out;
            mask_out = mask == ma ? mb : ma;
        }
        // 3. the synthesis
        IsArgs a{};
        a.img0 = args.img0 + (long long)i0 * args.img_image, a.img1 = args.img1 + (long long)i0 * args.img_image;
        a.g = src, a.hole = hole, a.fill = mask;
        a.out = args.out ? static_cast<unsigned char *>(args.out) + (long long)i0 * args.out_image * eb : nullptr;
        a.source = args.source ? args.source + (long long)i0 * args.source_stride : nullptr;
        a.n = m, a.w = w, a.h = h, a.wp = (int)wp;
        a.out_dtype = args.out_dtype, a.t = t;
        a.wide_out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, eb) == 4;
        a.wide_source = args.source && (((unsigned long long)(size_t)args.source | (unsigned long long)args.source_pitch |
                                         (unsigned long long)args.source_stride) & 3) == 0;
        a.img_pitch = args.img_pitch, a.img_plane = args.img_plane, a.img_image = args.img_image;
        a.out_pitch = args.out_pitch, a.out_plane = args.out_plane, a.out_image = args.out_image;
        a.source_pitch = args.source_pitch, a.source_stride = args.source_stride;
        const bool filled = args.fill_passes > 0;
        if (!three)
            is_launch_as<1, false>(s, a, filled);
        else if (!planes)
            is_launch_as<3, true>(s, a, filled);
        else
            is_launch_as<3, false>(s, a, filled);
    }
}
