// flow_chain_kernels.h — launcher of the composition of adjacent planar flows into long-range flows and dense trajectories
// (flow_chain_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

enum : int { FC_LAST = 0, FC_ALL = 1 };               // = DFX_CHAIN_LAST / DFX_CHAIN_ALL of include/dfx.h
enum : int { FC_BORDER_ZERO = 0, FC_BORDER_CLAMP = 1 }; // = DFX_WARP_BORDER_* of include/dfx.h

// Planar float32 flows of w x h pixels.  Flow i: u plane at flow + i * flow_stride, v plane plane_stride behind it, rows
// row_pitch apart (floats).  Link k of anchor j reads flow first + j * anchor_step + k * hop.  out holds anchors * E flows,
// E = emit == FC_ALL ? length : 1, output j * E + e laid out as the flows are with strides of its own.  occ (may be nullptr):
// one byte plane per flow, plane i at + i * occ_stride, occ_pitch bytes per row.  valid (may be nullptr): one byte plane per
// output flow, strides of its own.
struct FcArgs {
    const float *flow;
    const unsigned char *occ;
    float *out;
    unsigned char *valid;
    int w, h;
    int first, hop, length, anchors, anchor_step, emit, border;
    long long row_pitch, plane_stride, flow_stride; // floats
    long long occ_pitch, occ_stride;                // bytes
    long long out_pitch, out_plane, out_stride;     // floats
    long long valid_pitch, valid_stride;            // bytes
};

// Enqueues on s one launch per 65535 anchors, however long the chains.  Nothing for anchors <= 0.  Every bound of
// include/dfx.h's dfx_flow_chain_device, the range of the link indices among them, is the caller's to check.
void fc_launch(hipStream_t s, const FcArgs &a);
