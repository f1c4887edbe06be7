// dfx_pipeline.h — what the C ABI's entry points (dfx_api.cpp) hand to the FlowBuffer driver (dfx_pipeline.cpp).
#pragma once

#include "dfx_internal.h"

// Where the frames of a FlowBuffer are: host pointers (host mode) or one device array (device mode).
struct InSpec {
    const uint8_t *const *frames = nullptr; // host mode: one pointer per frame, frame_pitch bytes per row
    size_t frame_pitch = 0;
    const uint8_t *d_frames = nullptr; // device mode: frame i at d_frames + i * d_frame_stride, d_pitch bytes per row
    size_t d_pitch = 0, d_frame_stride = 0;
    // Caller-supplied initial flows (dfx_calc_batch_init*), one per output flow in output order; all unset: none.
    //   host mode  : init[i] = rows of interleaved (u, v) floats, init_pitch bytes per row
    //   device mode: d_init + i * d_init_stride, interleaved dense rows — or (init_planar) a u plane there and a v plane
    //                d_init_plane_stride behind it, rows d_init_row_pitch apart (all in floats)
    const float *const *init = nullptr;
    size_t init_pitch = 0;
    const float *d_init = nullptr;
    size_t d_init_stride = 0, d_init_row_pitch = 0, d_init_plane_stride = 0;
    bool init_planar = false;
    bool seeded() const { return init != nullptr || d_init != nullptr; }
    static InSpec host(const uint8_t *const *frames, size_t frame_pitch) {
        InSpec in;
        in.frames = frames, in.frame_pitch = frame_pitch;
        return in;
    }
    static InSpec device(const uint8_t *d_frames, size_t pitch, size_t frame_stride) {
        InSpec in;
        in.d_frames = d_frames, in.d_pitch = pitch, in.d_frame_stride = frame_stride;
        return in;
    }
};

// Where the flows of a FlowBuffer go: float (u, v) fields, float u and v planes, or planes bounded to 8 bits on the device.
struct OutSpec {
    bool quantized = false;
    double lo = 0, hi = 0;
    // float output
    float *const *flows = nullptr; // host mode: one pointer per flow, out_pitch bytes per row
    size_t out_pitch = 0;
    float *d_flows = nullptr; // device mode: flow i dense at d_flows + i*d_flow_stride
    size_t d_flow_stride = 0;
    // planar float output (dfx_calc_batch_planar*): every engine's last kernel writes a u and a v plane per flow, raw
    // (norm_bound = 0) or clamped to +-norm_bound and divided by it
    bool planar = false;
    float norm_bound = 0.f;
    int elem = 0; // DFX_ELEM_* (dfx_device.h): float32 planes, or float16 / bfloat16 ones (dfx_calc_batch_planar_as*)
    void *const *flows_u = nullptr, *const *flows_v = nullptr; // host mode: one pointer per plane, out_pitch bytes per row
    void *d_planar = nullptr; // device mode: u plane of flow i at d_planar + i*d_flow_stride, v plane d_plane_stride behind
    size_t d_row_pitch = 0, d_plane_stride = 0; // it, rows d_row_pitch apart (all in elements of `elem`)
    // both directions of every pair in one call (dfx_calc_batch_bidir_device: device mode, raw float32 planes): d_planar takes
    // the flows of `step`, d_planar_bwd — same three strides — those of -step; with mask pointers the forward-backward check
    // (fb_check_kernels.hip) of (fwd, bwd) goes to d_occ_fwd and that of (bwd, fwd) to d_occ_bwd, mask plane i at
    // + i*d_occ_stride bytes, occ_pitch bytes per row
    bool bidir = false;
    float *d_planar_bwd = nullptr;
    uint8_t *d_occ_fwd = nullptr, *d_occ_bwd = nullptr;
    size_t occ_pitch = 0, d_occ_stride = 0;
    float alpha1 = 0.f, alpha2 = 0.f;
    // 8-bit output
    uint8_t *const *img_x = nullptr, *const *img_y = nullptr; // host mode: one pointer per plane
    size_t img_pitch = 0;                                     // bytes per row (host and device mode)
    uint8_t *d_img_x = nullptr, *d_img_y = nullptr;           // device mode: plane i at + i*d_img_stride
    size_t d_img_stride = 0;
    // the -st=png scheme (implies quantized; lo / hi unused): planes scaled by the reference's per-flow adaptive bounds,
    // which go to bounds[2 * i] = {bound_x, bound_y} (host mode: filled when the call returns) or d_bounds (device mode)
    bool png = false;
    double *bounds = nullptr, *d_bounds = nullptr;
    // JPEG output (host mode; implies quantized): one file per plane into jpg_x[i] / jpg_y[i] (jpg_capacity bytes each)
    bool jpeg = false;
    int quality = 95;
    uint8_t *const *jpg_x = nullptr, *const *jpg_y = nullptr;
    size_t jpg_capacity = 0;
    uint32_t *size_x = nullptr, *size_y = nullptr;
};

// One FlowBuffer through the handle's engine.  ticket != nullptr (dfx_submit_*): the call returns when the device work is
// done and every batch but the last has been handed over; dfx_wait(*ticket) awaits the rest.  Consumes dfx_next_segments;
// after an error nothing is in flight.
int dfx_run_flowbuffer(dfx_context *c, const InSpec &in, int n_frames, int step, const OutSpec &out, uint64_t *ticket);

// staging that the single-stage entry points of dfx_api.cpp share with the driver
int dfx_ensure_img_staging(dfx_context *c, int need);      // d_img: `need` x planes, then the y planes, per parity
int dfx_ensure_png(dfx_context *c, int need);              // scratch and mapped bounds of the -st=png scheme
int dfx_ensure_jpeg(dfx_context *c, int pairs, int quality); // dfx_context::jpeg for batches of `pairs` pairs
// The encode of planes already in c->d_img[q] (x planes from index 0, y planes from y_first) into c->jpeg's parity q
int dfx_launch_jpeg(dfx_context *c, int q, int n_planes, int n_x, int y_first);
