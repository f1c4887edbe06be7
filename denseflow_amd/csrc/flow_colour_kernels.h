// flow_colour_kernels.h — launcher of the colour coding of flows (flow_colour_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

enum : int { FLOWVIS_NORM_FIXED = 0, FLOWVIS_NORM_FLOW = 1, FLOWVIS_NORM_BATCH = 2 }; // = DFX_COLOUR_NORM_* of include/dfx.h

// n planar float32 flows (flow i: a u plane at flow + i * flow_stride, its v plane plane_stride behind it, rows row_pitch
// apart, in floats: the layout of dfx_calc_batch_planar_device), optionally n mask planes (mask i at mask + i * mask_stride,
// mask_pitch bytes per row; nonzero = unknown), the n + 1 words of squared radii, the n colour images (image i at out + i *
// out_image bytes; interleaved: rows of 3 W bytes out_pitch apart; planar: three planes out_plane apart) and optionally n
// frames to blend over (1 or 3 channels, interleaved or planar, with strides of their own).
struct FlowvisArgs {
    const float *flow;
    const unsigned char *mask;  // may be nullptr
    float *max2;                // n + 1 words M2_0 .. M2_{n-1}, MB2; may be nullptr with FLOWVIS_NORM_FIXED: no measuring pass
    unsigned char *out;
    const unsigned char *frame; // may be nullptr: no blend
    int n, w, h;
    int i0;                     // the launch's first flow (set by the launcher: grid.z holds at most 65535 of them)
    long long row_pitch, plane_stride, flow_stride;    // floats
    long long mask_pitch, mask_stride;                 // bytes
    long long out_pitch, out_plane, out_image;         // bytes
    long long frame_pitch, frame_plane, frame_image;   // bytes
    int norm;                   // FLOWVIS_NORM_*
    float max_rad;              // R of FLOWVIS_NORM_FIXED
    int bgr;                    // the output's (and a 3-channel frame's) channel order: 0 = RGB, 1 = BGR
    int planar;                 // the output's layout: 0 = interleaved, 1 = three planes
    int frame_channels;         // 1 or 3
    int frame_planar;           // a 3-channel frame's layout
    int alpha256;               // 0 .. 256
    unsigned char unknown[3];   // the bytes of an unknown pixel, in the output's channel order
};

// Enqueues on s (nothing for n <= 0): with max2, its zeroing and the measuring pass; then the colour pass, which reads R from
// max2 on the device.  Every bound of include/dfx.h's dfx_flow_colour_device is the caller's to check.
void flowvis_launch(hipStream_t s, const FlowvisArgs &a);
