// prepare_kernels.h — launcher of the frame-preparation kernel (prepare_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

// 0: same size (colour conversion only), 1: exact 2x decimation (INTER_AREA fast path), 2: INTER_LINEAR
int prepare_mode(int sw, int sh, int dw, int dh);

// n source frames (sw x sh, `channels` = 1 gray or 3 colour) -> n gray frames of dw x dh.  Colour: B, G, R interleaved, or
// (rgb) R, G, B, or (planar) three byte planes plane_stride bytes apart (0: src_pitch * sh) with src_pitch the row pitch of
// one plane.
void prepare_launch(hipStream_t s, const unsigned char *d_src, long long src_pitch, long long src_frame_stride, int sw,
                    int sh, int channels, int n, unsigned char *d_dst, long long dst_pitch, long long dst_frame_stride,
                    int dw, int dh, int rgb = 0, int planar = 0, long long plane_stride = 0);

// n BGR frames (sw x sh, interleaved) -> n BGR frames of dw x dh: cv::resize(INTER_LINEAR) of every channel on its own.
// The buffers are device allocations (their first byte 4-byte aligned): rows are read as aligned dwords.
void prepare_bgr_launch(hipStream_t s, const unsigned char *d_src, long long src_pitch, long long src_frame_stride, int sw,
                        int sh, int n, unsigned char *d_dst, long long dst_pitch, long long dst_frame_stride, int dw,
                        int dh);
