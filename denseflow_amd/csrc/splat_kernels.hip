// splat_kernels.hip — forward warp (splat) of images and float payloads along planar flows on the device: frame 0 as seen at
// time t of F_{0->1}, and with it its labels, a depth plane or a feature map; the pixels nothing lands on are holes.  The
// scatter is that of flow_scatter.h — its skip rules, landing test, importance, taps, weights and window — with a payload of C
// channels beside the weight:
//     payload, 8-bit source:   q_c = the byte
//     payload, float32 source: skip unless every channel has fabsf(v_c) <= 32768.f (false for NaN);  q_c = (int)rintf(v_c * 256.f)
//     Wsum[tap] += wt;   S_c[tap] += wt * q_c      (64-bit, two's-complement wrap)
// and per target pixel, after all sources of the image:
//     hole = Wsum < Wmin;  r_c = (double)S_c / (double)Wsum (mean) or (double)S_c / 16777216.0 (sum), times 1.0/256.0 for a
//     float32 source;  out = (float)r_c or (uint8_t)llrint(r_c);  a hole is +0 / byte 0 (zero) or not written at all (keep)
//     coverage = (float)((double)Wsum / 16777216.0)
// All float operations are float32, each rounded on its own (the build's -ffp-contract=off), subnormals kept.
// tests/splat_ref.py is the same text in NumPy, and the device equals it bit for bit.
//
// Passes per wave of images, all on one stream with nothing between them:
//   k_fs_zero          the zero pass of flow_scatter.hip over the wave's words;
//   k_splat_scatter    fs_scatter_tile, grid.z the images of the wave; one instantiation per channel count and source form
//                      (8-bit planes: gray and planar 3; 8-bit interleaved 3: three byte loads; float32 planes 1 .. 4);
//                      importance and occ are wave-uniform runtime branches.  SPLAT_LDS_WINDOW 0: every add is a 64-bit global
//                      atomic, up to 4 (1 + C) per source pixel.  SPLAT_LDS_WINDOW 1: through the 48 x 16 pixel window in LDS
//                      (768 (1 + C) words: 12 / 18 / 24 / 30 KiB), flushed in rows of 384 (1 + C) contiguous bytes.
//   k_splat_normalise  the lane quad of flow_quad.h: a lane's 4 (1 + C) words as 16-byte loads where the workspace base is
//                      16-byte aligned and W (1 + C) is even (8-byte loads otherwise), the image, the hole mask and the
//                      coverage through its quad stores; with keep, a quad that holds a hole stores its other pixels singly.
#include "splat_kernels.h"

#ifndef SPLAT_LDS_WINDOW
#define SPLAT_LDS_WINDOW 1 // 0: the plain global-atomic scatter (kept for profiles/splat's A/B)
#endif

namespace {

typedef unsigned long long u64;

enum : int { SP_U8 = 0, SP_U8_IL = 1, SP_F32 = 2 }; // source forms: byte planes, interleaved bytes, float planes

struct SplatWide : FsWide {};

// C: channels; SRC: the source form; LDSW: through the LDS window.  grid: fs_scatter_grid
template <int C, int SRC, bool LDSW>
__global__ __launch_bounds__(FS_THREADS) void k_splat_scatter(SplatArgs a) {
    __shared__ u64 win[LDSW ? fs_window_words(1 + C) : 1];
    fs_scatter_tile<1 + C, LDSW>(win, a, a.imp != nullptr, a.occ != nullptr, [&](const FsLanding &, long long f, int x, int y, int (&q)[C]) {
        bool live = true;
        if (SRC == SP_F32) {
            const float *p = static_cast<const float *>(a.src) + f * a.src_image + (long long)y * a.src_pitch + x;
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                v[c] = p[C == 1 ? 0 : c * a.src_plane];
                live = live && __builtin_fabsf(v[c]) <= 32768.0f; // false for NaN: skipped, not clamped
            }
#pragma unroll
            for (int c = 0; c < C; ++c)
                q[c] = live ? (int)rintf(v[c] * 256.0f) : 0;
        } else {
            const unsigned char *p = static_cast<const unsigned char *>(a.src) + f * a.src_image + (long long)y * a.src_pitch +
                                     (SRC == SP_U8_IL ? C * x : x);
#pragma unroll
            for (int c = 0; c < C; ++c)
                q[c] = (int)p[SRC == SP_U8_IL ? (long long)c : (C == 1 ? 0ll : c * a.src_plane)];
        }
        return live;
    });
}

// C: channels; IL: the output's pixels are interleaved.  grid: fq_grid(w, h, images of the wave)
template <int C, bool IL>
__global__ __launch_bounds__(256) void k_splat_normalise(SplatArgs a, SplatWide wide) {
    constexpr int WORDS = 1 + C;
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const long long f = (long long)blockIdx.z;
    const int n = fq_count(a.w, x);
    u64 q[4 * WORDS];
    fs_load_quad<WORDS>(a, f, x, y, wide.work != 0, n, q);
    const double post = a.src_f32 ? 0.00390625 : 1.0; // 1.0 / 256.0
    float s[4][C], oc[4];
    unsigned oh[4];
    unsigned holes = 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const FsPixel p = fs_pixel(q[WORDS * e], a.wmin);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double sc = (double)(long long)q[WORDS * e + 1 + c];
            double r = a.sum ? sc / 16777216.0 : sc / p.d;
            r = p.hole ? 0.0 : r * post;
            s[e][c] = a.out_u8 ? (float)(unsigned)rint(r) : (float)r; // rint on [0, 255]: llrint's value, ties to even
        }
        oh[e] = p.hole ? 1u : 0u;
        holes |= (e < n && p.hole) ? 1u : 0u;
        oc[e] = p.cov;
    }
    if (a.out) {
        const int dtype = a.out_u8 ? FQ_ELEM_U8 : DFX_ELEM_F32;
        const long long row = f * a.out_image + (long long)y * a.out_pitch;
        if (a.keep && holes) {
            // the hole pixels stay as the caller left them: the others go one element at a time
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= n || oh[e])
                    continue;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const long long at = row + (IL ? (long long)((x + e) * C + c) : (C == 1 ? 0ll : c * a.out_plane) + x + e);
                    if (a.out_u8)
                        static_cast<unsigned char *>(a.out)[at] = (unsigned char)(unsigned)s[e][c];
                    else
                        static_cast<float *>(a.out)[at] = s[e][c];
                }
            }
        } else {
#pragma unroll
            for (int g = 0; g < C; ++g) { // the segments of flow_quad.h
                float sv[4];
                fq_segment<C, IL>(s, g, sv);
                const int m = fq_seg_count<C, IL>(g, n);
                if (m <= 0)
                    continue;
                fq_store_image(a.out, row + fq_seg_offset<C, IL>(x, g, C == 1 ? 0ll : a.out_plane), dtype, wide.out != 0, m, sv);
            }
        }
    }
    fs_store_masks(a, wide, f, x, y, n, oh, oc);
}

template <int C, int SRC>
void sp_scatter_as(hipStream_t s, const SplatArgs &a) {
    hipLaunchKernelGGL((k_splat_scatter<C, SRC, SPLAT_LDS_WINDOW != 0>), fs_scatter_grid(a), dim3(FS_THREADS), 0, s, a);
}

void sp_scatter(hipStream_t s, const SplatArgs &a) {
    if (!a.src_f32) {
        if (a.channels == 1)
            sp_scatter_as<1, SP_U8>(s, a);
        else if (a.interleaved)
            sp_scatter_as<3, SP_U8_IL>(s, a);
        else
            sp_scatter_as<3, SP_U8>(s, a);
    } else if (a.channels == 1) {
        sp_scatter_as<1, SP_F32>(s, a);
    } else if (a.channels == 2) {
        sp_scatter_as<2, SP_F32>(s, a);
    } else if (a.channels == 3) {
        sp_scatter_as<3, SP_F32>(s, a);
    } else {
        sp_scatter_as<4, SP_F32>(s, a);
    }
}

template <int C, bool IL>
void sp_normalise_as(hipStream_t s, const SplatArgs &a, const SplatWide &wide) {
    hipLaunchKernelGGL((k_splat_normalise<C, IL>), fq_grid(a.w, a.h, a.n), dim3(256), 0, s, a, wide);
}

void sp_normalise(hipStream_t s, const SplatArgs &a, const SplatWide &wide) {
    if (a.interleaved)
        sp_normalise_as<3, true>(s, a, wide);
    else if (a.channels == 1)
        sp_normalise_as<1, false>(s, a, wide);
    else if (a.channels == 2)
        sp_normalise_as<2, false>(s, a, wide);
    else if (a.channels == 3)
        sp_normalise_as<3, false>(s, a, wide);
    else
        sp_normalise_as<4, false>(s, a, wide);
}

SplatWide sp_wide(const SplatArgs &args) {
    const bool planes = args.channels > 1 && !args.interleaved;
    SplatWide wide = fs_wide<SplatWide>(args, splat_words(args.channels));
    wide.out = args.out && dfx_planar_vec(args.out, args.out_image, planes ? args.out_plane : 0, args.out_pitch, args.out_u8 ? 1 : 4) == 4;
    return wide;
}

} // namespace

void splat_launch(hipStream_t s, const SplatArgs &args, long long images_per_wave) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0 || images_per_wave <= 0 || args.channels < 1 || args.channels > SPLAT_MAX_CHANNELS)
        return;
    const SplatWide wide = sp_wide(args);
    const long long per_image = (long long)args.w * args.h * splat_words(args.channels); // words
    const int chunk = (int)std::min<long long>(images_per_wave, FQ_ITEMS_MAX);                   // grid.z holds at most FQ_ITEMS_MAX = 65535 images
    const long long src_bytes = args.src_f32 ? 4 : 1, out_bytes = args.out_u8 ? 1 : 4;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        SplatArgs a = args;
        fs_step(a, args, i0, chunk);
        a.src = static_cast<const unsigned char *>(args.src) + (long long)i0 * args.src_image * src_bytes;
        if (a.out)
            a.out = static_cast<unsigned char *>(args.out) + (long long)i0 * args.out_image * out_bytes;
        fs_zero(s, a.work, per_image * a.n);
        sp_scatter(s, a);
        sp_normalise(s, a, wide);
    }
}
