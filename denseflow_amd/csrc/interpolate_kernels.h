// interpolate_kernels.h — launcher of the frame interpolation at time t from two frames and their flows
// (interpolate_kernels.hip): two forward projections, the hole fill, and the synthesis pass.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

enum : int { INTERP_OUT_F32 = 0, INTERP_OUT_U8 = 3 }; // = DFX_PLANAR_F32 / DFX_WARP_U8 of include/dfx.h
enum : int { INTERP_MAX_PASSES = 16 };
enum : int { INTERP_TILE_W = 256, INTERP_TILE_H = 4 }; // pixels of a frame one workgroup of the synthesis pass owns

// n pairs of 8-bit images of w x h pixels and `channels` (1 or 3) bytes per pixel.  Pair i: frame 0 at img0 + i * img_image,
// frame 1 at img1 + i * img_image; interleaved (channels == 3 && !planar): pixel (x, y) channel c at y * img_pitch + 3 * x + c;
// otherwise channel c is a plane at c * img_plane, rows img_pitch apart (bytes).  fwd / bwd (bwd may be nullptr): planar
// float32 flows, flow i's u plane at + i * flow_stride, v plane plane_stride behind it, rows row_pitch apart (floats).
// occ_fwd / occ_bwd (each may be nullptr): byte planes, plane i at + i * occ_stride.  out (may be nullptr) lies as the images
// do with strides of its own, in elements of out_dtype; source (may be nullptr): byte planes, plane i at + i * source_stride.
// work: interp_work_bytes() bytes per pair of a wave, 8-byte aligned.
struct InterpArgs {
    const unsigned char *img0, *img1;
    const float *fwd, *bwd;
    const unsigned char *occ_fwd, *occ_bwd;
    void *out;
    unsigned char *source;
    void *work;
    size_t work_bytes;
    int n, w, h;
    int channels, planar, out_dtype;
    float t, min_weight;
    int fill_passes, ksize;
    long long img_pitch, img_plane, img_image;      // bytes
    long long row_pitch, plane_stride, flow_stride; // floats
    long long occ_pitch, occ_stride;                // bytes
    long long out_pitch, out_plane, out_image;      // elements of out_dtype
    long long source_pitch, source_stride;          // bytes
};

// The workspace one pair needs: the sums of one projection (the two projections of a wave use them one after the other),
// the two projected flows and, with fill passes, their ping-pong twins, the two hole planes and, with fill passes, one or
// two mask planes per side; rows padded to a multiple of 4 pixels and every region to 16 bytes.
size_t interp_work_bytes(int w, int h, int fill_passes);

// Enqueues on s, per wave of min(n, work_bytes / interp_work_bytes, 32767) pairs: the projections (fp_launch), fill_passes
// fills over the 2k flows of the wave as one batch (fm_launch), the synthesis.  Nothing for n <= 0.  Every bound of
// include/dfx.h's dfx_interpolate_device is the caller's to check.
void interp_launch(hipStream_t s, const InterpArgs &a);
