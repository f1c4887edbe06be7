// splat_kernels.h — launcher of the forward warp (splat) of images and float payloads along planar flows with integer sums
// (splat_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "flow_scatter.h"

enum : int { SPLAT_MAX_CHANNELS = 4 };

// 64-bit words per pixel of the workspace of a payload of `channels`: Wsum, then S_0 .. S_{channels-1}, pixel after pixel
inline int splat_words(int channels) { return 1 + channels; }

// Source image i of w x h pixels and `channels` channels lies at src + i * src_image (elements: bytes of an 8-bit source,
// floats of a float32 one), rows src_pitch apart; the channels of a pixel next to each other (interleaved, 8-bit with 3
// channels only) or in planes src_plane apart.  flow, imp, occ, hole, cov, wmin and work are FsSource's (flow_scatter.h; work:
// splat_words(channels) * w * h words per image of a wave).  out (may be nullptr): the source's channels and layout, bytes
// (out_u8) or floats, strides in elements.
struct SplatArgs : FsSource {
    const void *src;
    void *out;
    int channels;    // 1 .. 4
    int src_f32;     // 0: bytes, q = the byte; 1: floats, q = (int)rintf(v * 256.f), skipped unless every |v| <= 32768
    int interleaved; // 1: 8-bit, 3 channels, H x W x 3 (source and output alike)
    int out_u8;      // 1: (uint8_t)llrint(r); 0: (float)r
    int sum;         // 0: r = S / Wsum; 1: r = S / 2^24
    int keep;        // 1: the hole pixels of out are not written
    long long src_pitch, src_plane, src_image; // elements of the source
    long long out_pitch, out_plane, out_image; // elements of the output
};

// Enqueues on s, per wave of min(images_per_wave, 65535) images: zero the wave's words, scatter, normalise.  Nothing for
// n <= 0.  Every bound of include/dfx.h's dfx_splat_device is the caller's to check.
void splat_launch(hipStream_t s, const SplatArgs &a, long long images_per_wave);
