// dfx_api.cpp — the C ABI of include/dfx.h: argument checking, the thin entry points, statistics and memory helpers.
// The FlowBuffer driver is dfx_pipeline.cpp, colour frame extraction dfx_frames.cpp; the algorithms live in *_engine.cpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dfx_pipeline.h"
#include "fb_check_kernels.h"
#include "flow_chain_kernels.h"
#include "flow_colour_kernels.h"
#include "flow_hist_kernels.h"
#include "flow_project_kernels.h"
#include "flow_median_kernels.h"
#include "global_motion_kernels.h"
#include "interpolate_kernels.h"
#include "jpeg_kernels.h"
#include "plane_warp_kernels.h"
#include "prepare_kernels.h"
#include "quantize_kernels.h"
#include "splat_kernels.h"
#include "warp_kernels.h"

namespace {

thread_local std::string g_create_error;

int fail_create(int code, const std::string &msg) {
    g_create_error = msg;
    return code;
}

void default_params(dfx_params *p) {
    std::memset(p, 0, sizeof *p);
    // cv::cuda::OpticalFlowDual_TVL1::create() defaults
    p->tvl1_tau = 0.25;
    p->tvl1_lambda = 0.15;
    p->tvl1_theta = 0.3;
    p->tvl1_nscales = 5;
    p->tvl1_warps = 5;
    p->tvl1_epsilon = 0.01;
    p->tvl1_iterations = 300;
    p->tvl1_scale_step = 0.8;
    p->tvl1_gamma = 0.0;
    // cv::cuda::FarnebackOpticalFlow::create() defaults
    p->farn_num_levels = 5;
    p->farn_pyr_scale = 0.5;
    p->farn_win_size = 13;
    p->farn_num_iters = 10;
    p->farn_poly_n = 5;
    p->farn_poly_sigma = 1.1;
    p->farn_flags = 0;
    p->farn_window = DFX_FARN_WINDOW_BOX;
    p->farn_fast_pyramids = 0;
    // cuda::BroxOpticalFlow::create(0.197f, 50.0f, 0.8f, 10, 77, 10): src/denseflow_gpu.cpp:303
    p->brox_alpha = 0.197f;
    p->brox_gamma = 50.0f;
    p->brox_scale_factor = 0.8f;
    p->brox_inner_iterations = 10;
    p->brox_outer_iterations = 77;
    p->brox_solver_iterations = 10;
}

} // namespace

// ================================================================================================
// C ABI

extern "C" {

int dfx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

void dfx_default_params(dfx_params *p) {
    if (p)
        default_params(p);
}

int dfx_algo_from_name(const char *name, dfx_algo *out) {
    if (!name)
        return DFX_ERR_UNKNOWN_ALGO;
    if (!std::strcmp(name, "tvl1")) {
        if (out)
            *out = DFX_ALGO_TVL1;
        return DFX_OK;
    }
    if (!std::strcmp(name, "farn")) {
        if (out)
            *out = DFX_ALGO_FARN;
        return DFX_OK;
    }
    if (!std::strcmp(name, "brox")) {
        if (out)
            *out = DFX_ALGO_BROX;
        return DFX_OK;
    }
    if (!std::strcmp(name, "nv"))
        return DFX_ERR_NV_DISABLED;
    return DFX_ERR_UNKNOWN_ALGO;
}

const char *dfx_algo_error_message(int status, const char *name, char *buf, size_t buflen) {
    if (!buf || buflen == 0)
        return "";
    if (status == DFX_ERR_NV_DISABLED)
        snprintf(buf, buflen, "NV hardware flow not enabled, pls recompile"); // src/denseflow_gpu.cpp:296
    else if (status == DFX_ERR_UNKNOWN_ALGO)
        snprintf(buf, buflen, "unknown optical algorithm %s", name ? name : ""); // src/denseflow_gpu.cpp:336
    else
        buf[0] = 0;
    return buf;
}

int dfx_create(dfx_handle *out, int device, dfx_algo algo, int width, int height, const dfx_params *params) {
    if (!out)
        return fail_create(DFX_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (width < 1 || height < 1 || width > 32768 || height > 32768)
        return fail_create(DFX_ERR_INVALID, "invalid frame size");
    if (algo != DFX_ALGO_TVL1 && algo != DFX_ALGO_FARN && algo != DFX_ALGO_BROX && algo != DFX_ALGO_FRAMES)
        return fail_create(DFX_ERR_INVALID, "invalid algorithm id");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail_create(DFX_ERR_NO_DEVICE, "no HIP device available (this engine has no CPU fallback)");
    if (device < 0 || device >= n)
        return fail_create(DFX_ERR_INVALID, "device index out of range");

    dfx_context *c = new dfx_context();
    c->device = device;
    c->algo = algo;
    c->W = width;
    c->H = height;
    if (params)
        c->prm = *params;
    else
        default_params(&c->prm);

    auto init = [&]() -> int {
        HIPCHK(c, hipSetDevice(device));
        if (c->prm.blocking_sync) {
            // The runtime's waits spin unless the DEVICE is set to blocking scheduling: hipEventBlockingSync alone left the
            // waiting thread at 100 % CPU (profiles/round4/pmc/blocking_sync_ab.txt).  A process that has already fixed the
            // device's flags (an error here) keeps its own choice.
            (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
            (void)hipGetLastError();
        }
        HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->d2h_stream, hipStreamNonBlocking));
        for (auto &e : c->ev_h2d)
            HIPCHK(c, hipEventCreateWithFlags(&e, dfx_event_flags(c, false)));
        for (auto &e : c->ev_compute)
            HIPCHK(c, hipEventCreateWithFlags(&e, dfx_event_flags(c, false)));
        for (auto &e : c->ev_d2h)
            HIPCHK(c, hipEventCreateWithFlags(&e, dfx_event_flags(c, false)));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_t0, dfx_event_flags(c, true)));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_t1, dfx_event_flags(c, true)));
        if (c->prm.blocking_sync)
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_block, dfx_event_flags(c, false)));
        if (algo == DFX_ALGO_TVL1)
            c->engine = dfx_make_tvl1_engine(c);
        else if (algo == DFX_ALGO_FARN)
            c->engine = dfx_make_farneback_engine(c);
        else if (algo == DFX_ALGO_BROX)
            c->engine = dfx_make_brox_engine(c);
        else
            c->engine = dfx_make_frames_engine(c);
        return c->engine->create();
    };
    const int rc = init();
    if (rc != DFX_OK) {
        g_create_error = c->get_err();
        dfx_destroy(c);
        return rc;
    }
    *out = c;
    return DFX_OK;
}

int dfx_set_size(dfx_handle h, int width, int height) {
    if (!h)
        return DFX_ERR_INVALID;
    if (width < 1 || height < 1 || width > 32768 || height > 32768) // refused: nothing of the handle changes
        return dfx_fail(h, DFX_ERR_INVALID, "invalid frame size");
    // everything outstanding first: deferred tails hold sizes and buffers of the current geometry
    (void)dfx_finish_tails(h, 0, -1);
    h->clear_segments();
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->copy_stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->d2h_stream));
    // the current size again takes the same path: the engine is re-planned and its control state restarts
    const int rc = h->engine->set_size(width, height); // plan + ensure capacity; a failure leaves the engine as it was
    if (rc != DFX_OK)
        return rc;
    h->W = width;
    h->H = height;
    dfx_pipeline_resized(h);
    dfx_colour_resized(h);
    h->default_source();
    return DFX_OK;
}

size_t dfx_device_bytes(dfx_handle h) {
    if (!h)
        return 0;
    const auto &j = h->jpeg;
    size_t n = h->engine ? h->engine->device_bytes() : 0;
    n += 2 * (h->u8_bytes + h->flow_bytes + h->src_bytes + h->img_bytes + h->seed_bytes);
    n += h->d_png_scratch ? quant_png_scratch_bytes(h->png_slots) : 0;
    n += (j.d_tab ? sizeof(JpegTables) : 0) + j.blocks_cap * (sizeof(short) + sizeof(unsigned)) + j.planes_cap * 16 +
         (j.d_hdr ? 16 : 0) + 2 * j.capacity;
    return n + h->colour.device_bytes;
}

namespace {
// dfx_next_segments applies to the NEXT calc / submit call only, whether that call succeeds or not (include/dfx.h).  The
// list is consumed inside dfx_run_flowbuffer, which a call rejected by its wrapper's argument checks never reaches: every
// public entry point holds one of these, so a rejected call cannot leave the list armed for an unrelated later one.
struct SegmentsScope {
    dfx_context *c;
    explicit SegmentsScope(dfx_context *ctx) : c(ctx) {}
    ~SegmentsScope() {
        if (c)
            c->clear_segments();
    }
    void hand_over() { c = nullptr; } // another entry point takes over (dfx_calc -> dfx_calc_batch)
};
// |step| for the wrappers' early size computations; INT_MIN (whose negation is not an int) saturates, and the body
// rejects it with every other out-of-range step.
inline int abs_step(int step) { return step == INT_MIN ? INT_MAX : std::abs(step); }
// frame_pitch of a host-pointer call: checked against the handle's input rows, unless a dfx_next_segments_src declaration
// is pending (every clip then has its own pitch, checked when it was declared, and the call's is ignored)
inline bool pitch_too_small(dfx_handle h, size_t frame_pitch) {
    return h->next_seg_fmt.empty() && frame_pitch < h->in_row_bytes();
}
// pitch / frame_stride of a device-resident call against the handle's input frames (for a channels-first source: the row
// pitch of one plane, and three planes src_plane_stride apart that must not overlap)
inline bool device_frames_too_small(dfx_handle h, size_t pitch, size_t frame_stride) {
    if (pitch < h->in_row_bytes())
        return true;
    const size_t span = h->in_frame_span(pitch);
    return span == 0 || frame_stride < span;
}
// the device-resident forms have one format for the whole array
inline bool src_segments_pending(dfx_handle h) { return !h->next_seg_fmt.empty(); }
} // namespace

int dfx_calc(dfx_handle h, const uint8_t *a, size_t a_pitch, const uint8_t *b, size_t b_pitch, float *flow_uv,
             size_t out_pitch) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (!a || !b || !flow_uv)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frame or flow pointer");
    const size_t rb = h->in_row_bytes();
    const int rows = h->in_h();
    if (a_pitch < rb || b_pitch < rb)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    if (a_pitch != b_pitch) { // dfx_calc_batch takes one pitch: repack both frames densely
        std::vector<uint8_t> ta(rb * rows), tb(rb * rows);
        for (int y = 0; y < rows; ++y) {
            std::memcpy(ta.data() + (size_t)y * rb, a + (size_t)y * a_pitch, rb);
            std::memcpy(tb.data() + (size_t)y * rb, b + (size_t)y * b_pitch, rb);
        }
        const uint8_t *fr[2] = {ta.data(), tb.data()};
        float *fl[1] = {flow_uv};
        seg_scope.hand_over();
        return dfx_calc_batch(h, fr, rb, 2, 1, fl, out_pitch);
    }
    const uint8_t *fr[2] = {a, b};
    float *fl[1] = {flow_uv};
    seg_scope.hand_over();
    return dfx_calc_batch(h, fr, a_pitch, 2, 1, fl, out_pitch);
}

namespace {
// The checked bodies of the host-pointer entry points: ticket = nullptr is the blocking dfx_calc_batch* form, otherwise
// the dfx_submit_batch* form.
// a dfx_submit_* call without a ticket: refused, and it was the call a pending dfx_next_segments applied to
int null_ticket(dfx_handle h) {
    SegmentsScope seg_scope(h);
    return dfx_fail(h, DFX_ERR_INVALID, "NULL ticket");
}

int float_entry(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                float *const *flows_uv, size_t out_pitch, uint64_t *ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !flows_uv))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames or flows array");
    if (M > 0 && (pitch_too_small(h, frame_pitch) || out_pitch < (size_t)h->W * 8))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    OutSpec out;
    out.flows = flows_uv;
    out.out_pitch = out_pitch;
    return dfx_run_flowbuffer(h, InSpec::host(frames, frame_pitch), n_frames, step, out, ticket);
}

int u8_entry(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step, double lower_bound,
             double upper_bound, uint8_t *const *img_x, uint8_t *const *img_y, size_t img_pitch, uint64_t *ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !img_x || !img_y))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames or image plane array");
    if (M > 0 && (pitch_too_small(h, frame_pitch) || img_pitch < (size_t)h->W))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    OutSpec out;
    out.quantized = true;
    out.lo = lower_bound, out.hi = upper_bound;
    out.img_x = img_x, out.img_y = img_y, out.img_pitch = img_pitch;
    return dfx_run_flowbuffer(h, InSpec::host(frames, frame_pitch), n_frames, step, out, ticket);
}

// the -st=png scheme (src/common.cpp:18-46, 66-71): planes scaled by the per-flow adaptive bounds + the bounds
int png_entry(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step, uint8_t *const *img_x,
              uint8_t *const *img_y, size_t img_pitch, double *bounds_xy, uint64_t *ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !img_x || !img_y || !bounds_xy))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames, image plane array or bounds array");
    if (M > 0 && (pitch_too_small(h, frame_pitch) || img_pitch < (size_t)h->W))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    OutSpec out;
    out.quantized = out.png = true;
    out.img_x = img_x, out.img_y = img_y, out.img_pitch = img_pitch, out.bounds = bounds_xy;
    return dfx_run_flowbuffer(h, InSpec::host(frames, frame_pitch), n_frames, step, out, ticket);
}

int jpeg_entry(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step, double lower_bound,
               double upper_bound, int quality, uint8_t *const *jpg_x, uint8_t *const *jpg_y, size_t jpg_capacity,
               uint32_t *size_x, uint32_t *size_y, uint64_t *ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !jpg_x || !jpg_y || !size_x || !size_y))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames, JPEG buffer or size array");
    if (M > 0 && pitch_too_small(h, frame_pitch))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    if (quality < 1 || quality > 100)
        return dfx_fail(h, DFX_ERR_INVALID, "JPEG quality must be 1..100");
    if (h->W > 65535 || h->H > 65535)
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "JPEG: frame larger than 65535 pixels");
    OutSpec out;
    out.quantized = out.jpeg = true;
    out.lo = lower_bound, out.hi = upper_bound;
    out.quality = quality;
    out.jpg_x = jpg_x, out.jpg_y = jpg_y, out.jpg_capacity = jpg_capacity;
    out.size_x = size_x, out.size_y = size_y;
    return dfx_run_flowbuffer(h, InSpec::host(frames, frame_pitch), n_frames, step, out, ticket);
}
} // namespace

int dfx_calc_batch(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                   float *const *flows_uv, size_t out_pitch) {
    return float_entry(h, frames, frame_pitch, n_frames, step, flows_uv, out_pitch, nullptr);
}

int dfx_submit_batch(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                     float *const *flows_uv, size_t out_pitch, uint64_t *ticket) {
    if (h && !ticket)
        return null_ticket(h);
    return float_entry(h, frames, frame_pitch, n_frames, step, flows_uv, out_pitch, ticket);
}

int dfx_calc_batch_u8(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                      double lower_bound, double upper_bound, uint8_t *const *img_x, uint8_t *const *img_y,
                      size_t img_pitch) {
    return u8_entry(h, frames, frame_pitch, n_frames, step, lower_bound, upper_bound, img_x, img_y, img_pitch, nullptr);
}

int dfx_submit_batch_u8(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                        double lower_bound, double upper_bound, uint8_t *const *img_x, uint8_t *const *img_y,
                        size_t img_pitch, uint64_t *ticket) {
    if (h && !ticket)
        return null_ticket(h);
    return u8_entry(h, frames, frame_pitch, n_frames, step, lower_bound, upper_bound, img_x, img_y, img_pitch, ticket);
}

int dfx_calc_batch_png(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                       uint8_t *const *img_x, uint8_t *const *img_y, size_t img_pitch, double *bounds_xy) {
    return png_entry(h, frames, frame_pitch, n_frames, step, img_x, img_y, img_pitch, bounds_xy, nullptr);
}

int dfx_submit_batch_png(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                         uint8_t *const *img_x, uint8_t *const *img_y, size_t img_pitch, double *bounds_xy,
                         uint64_t *ticket) {
    if (h && !ticket)
        return null_ticket(h);
    return png_entry(h, frames, frame_pitch, n_frames, step, img_x, img_y, img_pitch, bounds_xy, ticket);
}

int dfx_calc_batch_jpeg(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                        double lower_bound, double upper_bound, int quality, uint8_t *const *jpg_x,
                        uint8_t *const *jpg_y, size_t jpg_capacity, uint32_t *size_x, uint32_t *size_y) {
    return jpeg_entry(h, frames, frame_pitch, n_frames, step, lower_bound, upper_bound, quality, jpg_x, jpg_y,
                      jpg_capacity, size_x, size_y, nullptr);
}

int dfx_submit_batch_jpeg(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                          double lower_bound, double upper_bound, int quality, uint8_t *const *jpg_x,
                          uint8_t *const *jpg_y, size_t jpg_capacity, uint32_t *size_x, uint32_t *size_y,
                          uint64_t *ticket) {
    if (h && !ticket)
        return null_ticket(h);
    return jpeg_entry(h, frames, frame_pitch, n_frames, step, lower_bound, upper_bound, quality, jpg_x, jpg_y,
                      jpg_capacity, size_x, size_y, ticket);
}

int dfx_calc_batch_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                          int step, float *d_flows, size_t flow_stride_floats) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_flows))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or flows");
    if (M > 0 && (device_frames_too_small(h, pitch, frame_stride) ||
                  flow_stride_floats < (size_t)h->W * h->H * 2))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    OutSpec out;
    out.d_flows = d_flows;
    out.d_flow_stride = flow_stride_floats;
    return dfx_run_flowbuffer(h, InSpec::device(d_frames, pitch, frame_stride), n_frames, step, out, nullptr);
}

namespace {
// norm_bound of the planar forms: 0 (raw) or a bound that is a positive finite float
bool planar_bound_ok(double norm_bound) {
    if (norm_bound == 0.0)
        return true;
    const float b = (float)norm_bound;
    return std::isfinite(norm_bound) && norm_bound > 0.0 && std::isfinite(b) && b > 0.0f;
}
const char *const kPlanarBound = "norm_bound must be 0 (raw values) or a positive finite float";
const char *const kPlanarDtype = "dtype must be DFX_PLANAR_F32, DFX_PLANAR_F16 or DFX_PLANAR_BF16";
inline bool planar_dtype_ok(int dtype) { return dtype >= DFX_PLANAR_F32 && dtype <= DFX_PLANAR_BF16; }
// the stride rules of the device-resident planar forms, in elements.  The products cannot overflow: W, H <= 32768, and a
// stride that passes the check before it is what the next one multiplies
inline bool planar_strides_bad(dfx_handle h, size_t row_pitch, size_t plane_stride, size_t flow_stride) {
    return row_pitch < (size_t)h->W || row_pitch > ((size_t)1 << 40) || plane_stride < (size_t)h->H * row_pitch ||
           plane_stride > ((size_t)1 << 60) || flow_stride < 2 * plane_stride;
}
const char *const kPlanarStrides = "planar output: row_pitch_floats >= W, plane_stride_floats >= H * row_pitch_floats and "
                                   "flow_stride_floats >= 2 * plane_stride_floats are required";
const char *const kPlanarStridesAs = "planar output: row_pitch >= W, plane_stride >= H * row_pitch and flow_stride >= 2 * "
                                     "plane_stride (in elements of dtype) are required";

// the three planar forms behind their float32 and typed entry points; `typed` only chooses the text of a stride refusal
int planar_host(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step, double norm_bound,
                int dtype, void *const *flows_u, void *const *flows_v, size_t out_pitch) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (!planar_dtype_ok(dtype))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarDtype);
    if (!planar_bound_ok(norm_bound))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarBound);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !flows_u || !flows_v))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames or flow plane arrays");
    if (M > 0 && (pitch_too_small(h, frame_pitch) || out_pitch < (size_t)h->W * dfx_elem_bytes(dtype)))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    OutSpec out;
    out.planar = true;
    out.norm_bound = (float)norm_bound;
    out.elem = dtype;
    out.flows_u = flows_u, out.flows_v = flows_v;
    out.out_pitch = out_pitch;
    return dfx_run_flowbuffer(h, InSpec::host(frames, frame_pitch), n_frames, step, out, nullptr);
}

int planar_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames, int step,
                  double norm_bound, int dtype, bool typed, void *d_out, size_t row_pitch, size_t plane_stride,
                  size_t flow_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (!planar_dtype_ok(dtype))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarDtype);
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    if (!planar_bound_ok(norm_bound))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarBound);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_out))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or flow planes");
    if (M > 0 && device_frames_too_small(h, pitch, frame_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    if (M > 0 && planar_strides_bad(h, row_pitch, plane_stride, flow_stride))
        return dfx_fail(h, DFX_ERR_INVALID, typed ? kPlanarStridesAs : kPlanarStrides);
    OutSpec out;
    out.planar = true;
    out.norm_bound = (float)norm_bound;
    out.elem = dtype;
    out.d_planar = d_out;
    out.d_row_pitch = row_pitch, out.d_plane_stride = plane_stride, out.d_flow_stride = flow_stride;
    return dfx_run_flowbuffer(h, InSpec::device(d_frames, pitch, frame_stride), n_frames, step, out, nullptr);
}
} // namespace

int dfx_calc_batch_planar(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                          double norm_bound, float *const *flows_u, float *const *flows_v, size_t out_pitch) {
    return planar_host(h, frames, frame_pitch, n_frames, step, norm_bound, DFX_PLANAR_F32, (void *const *)flows_u,
                       (void *const *)flows_v, out_pitch);
}

int dfx_calc_batch_planar_as(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                             double norm_bound, int dtype, void *const *flows_u, void *const *flows_v, size_t out_pitch) {
    return planar_host(h, frames, frame_pitch, n_frames, step, norm_bound, dtype, flows_u, flows_v, out_pitch);
}

int dfx_calc_batch_planar_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                                 int step, double norm_bound, float *d_out, size_t row_pitch_floats,
                                 size_t plane_stride_floats, size_t flow_stride_floats) {
    return planar_device(h, d_frames, pitch, frame_stride, n_frames, step, norm_bound, DFX_PLANAR_F32, false, d_out,
                         row_pitch_floats, plane_stride_floats, flow_stride_floats);
}

int dfx_calc_batch_planar_as_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                                    int step, double norm_bound, int dtype, void *d_out, size_t row_pitch,
                                    size_t plane_stride, size_t flow_stride) {
    return planar_device(h, d_frames, pitch, frame_stride, n_frames, step, norm_bound, dtype, true, d_out, row_pitch,
                         plane_stride, flow_stride);
}

// ---- both directions of every pair in one call, and the forward-backward check of two flows ----
namespace {
// alpha1 / alpha2 of the check: finite and not negative
inline bool fb_alpha_ok(float a) { return std::isfinite(a) && a >= 0.0f; }
const char *const kFbAlpha = "alpha1 and alpha2 must be finite and >= 0";
const char *const kPlanarStridesOut = "output flows: out_row_pitch_floats >= W, out_plane_stride_floats >= H * out_row_pitch_floats "
                                      "and out_flow_stride_floats >= 2 * out_plane_stride_floats are required";

// The stride rule of one plane per item — a mask or any other (n, H, W) plane of bytes or floats: DFX_OK where the plane is
// absent or its strides span it, else the refusal.  The text names the descriptor's fields: "<what> planes:
// <field>_pitch<unit> >= W ...", unit "_floats" where the strides count floats.
int plane_check(dfx_handle h, bool present, size_t pitch, size_t stride, const char *what, const char *field,
                const char *unit = "") {
    if (!present || !(pitch < (size_t)h->W || pitch > ((size_t)1 << 40) || stride < pitch * (size_t)h->H))
        return DFX_OK;
    const std::string p = std::string(field) + "_pitch" + unit, s = std::string(field) + "_stride" + unit;
    return dfx_fail(h, DFX_ERR_INVALID, std::string(what) + " planes: " + p + " >= W and " + s + " >= H * " + p + " are required");
}

// What every call on finished flows opens with.  True: go on.  False: return *status, a refusal or — an empty batch —
// DFX_OK.  has_desc: the descriptor is not NULL (a call without one says true).
bool post_begin(dfx_handle h, bool has_desc, int n, int *status) {
    *status = DFX_ERR_INVALID;
    if (!h)
        return false;
    (void)dfx_finish_tails(h, 0, -1);
    if (h->algo == DFX_ALGO_FRAMES)
        *status = dfx_fail(h, DFX_ERR_UNSUPPORTED, "a DFX_ALGO_FRAMES handle computes no flow");
    else if (!has_desc)
        *status = dfx_fail(h, DFX_ERR_INVALID, "NULL descriptor");
    else if (n < 0)
        *status = dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    else
        *status = DFX_OK;
    return *status == DFX_OK && n != 0;
}
extern "C++" { // (this file is one extern "C" block, which takes no template)
template <class Desc>
bool post_begin(dfx_handle h, const Desc *d, int *status) {
    return post_begin(h, d != nullptr, d ? d->n : 0, status);
}

// What dfx_flow_project_device and dfx_splat_device check alike (their descriptors name these fields alike), in three pieces
// so that each call keeps the order of its refusals: the outputs and the parameters (scale: 0 from a call that has none);
// the workspace, of per_item bytes an item (`sizer` names the call that gives them); the planes, with the call's own outputs
// (out_bad: their strides do not span them) between occ and hole.  scatter_fill: the FsSource fields of either descriptor.
template <class Desc>
int scatter_check_params(dfx_handle h, const Desc *d, float scale) {
    if (!d->d_out && !d->d_hole && !d->d_coverage)
        return dfx_fail(h, DFX_ERR_INVALID, "one of d_out, d_hole and d_coverage is required");
    if (!std::isfinite(d->t) || d->t == 0.0f)
        return dfx_fail(h, DFX_ERR_INVALID, "t must be finite and nonzero");
    if (!std::isfinite(scale))
        return dfx_fail(h, DFX_ERR_INVALID, "scale must be finite");
    if (!std::isfinite(d->min_weight) || !(d->min_weight >= 0.0f))
        return dfx_fail(h, DFX_ERR_INVALID, "min_weight must be finite and >= 0");
    return DFX_OK;
}
template <class Desc>
int scatter_check_work(dfx_handle h, const Desc *d, size_t per_item, const char *sizer) {
    if ((size_t)d->d_work % 8 != 0)
        return dfx_fail(h, DFX_ERR_INVALID, "d_work must be 8-byte aligned");
    if (d->work_bytes < per_item)
        return dfx_fail(h, DFX_ERR_INVALID, std::string("work_bytes must be at least ") + sizer);
    return DFX_OK;
}
template <class Desc>
int scatter_check_planes(dfx_handle h, const Desc *d, bool out_bad, const char *out_text) {
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, d->d_importance != nullptr, d->importance_pitch_floats, d->importance_stride_floats, "importance",
                            "importance", "_floats"))
        return e;
    if (int e = plane_check(h, d->d_occ != nullptr, d->occ_pitch, d->occ_stride, "mask", "occ"))
        return e;
    if (out_bad)
        return dfx_fail(h, DFX_ERR_INVALID, out_text);
    if (int e = plane_check(h, d->d_hole != nullptr, d->hole_pitch, d->hole_stride, "hole", "hole"))
        return e;
    return plane_check(h, d->d_coverage != nullptr, d->coverage_pitch_floats, d->coverage_stride_floats, "coverage", "coverage",
                       "_floats");
}
template <class Desc>
void scatter_fill(FsSource &a, dfx_handle h, const Desc *d) {
    a.flow = d->d_flow, a.imp = d->d_importance, a.occ = d->d_occ, a.hole = d->d_hole, a.cov = d->d_coverage;
    a.work = static_cast<unsigned long long *>(d->d_work);
    a.n = d->n, a.w = h->W, a.h = h->H, a.t = d->t, a.wmin = fp_wmin(d->min_weight);
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.imp_pitch = (long long)d->importance_pitch_floats, a.imp_stride = (long long)d->importance_stride_floats;
    a.occ_pitch = (long long)d->occ_pitch, a.occ_stride = (long long)d->occ_stride;
    a.hole_pitch = (long long)d->hole_pitch, a.hole_stride = (long long)d->hole_stride;
    a.cov_pitch = (long long)d->coverage_pitch_floats, a.cov_stride = (long long)d->coverage_stride_floats;
}
}

// ... and what it closes with: the launches' errors, the stream drained.
int post_finish(dfx_handle h) {
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DFX_OK;
}
} // namespace

int dfx_calc_batch_bidir_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                                int step, float *d_fwd, float *d_bwd, size_t row_pitch_floats, size_t plane_stride_floats,
                                size_t flow_stride_floats, float alpha1, float alpha2, uint8_t *d_occ_fwd,
                                uint8_t *d_occ_bwd, size_t occ_pitch, size_t occ_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (h->algo == DFX_ALGO_FRAMES)
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "a DFX_ALGO_FRAMES handle computes no flow");
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    if (step == 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n_frames must be >= 0 and step non-zero");
    if ((d_occ_fwd == nullptr) != (d_occ_bwd == nullptr))
        return dfx_fail(h, DFX_ERR_INVALID, "both mask pointers or neither (NULL, NULL: no check)");
    const bool check = d_occ_fwd != nullptr;
    if (check && (!fb_alpha_ok(alpha1) || !fb_alpha_ok(alpha2)))
        return dfx_fail(h, DFX_ERR_INVALID, kFbAlpha);
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_fwd || !d_bwd))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or flow planes");
    if (M > 0 && device_frames_too_small(h, pitch, frame_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    if (M > 0 && planar_strides_bad(h, row_pitch_floats, plane_stride_floats, flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, M > 0 && check, occ_pitch, occ_stride, "mask", "occ"))
        return e;
    OutSpec out;
    out.planar = out.bidir = true;
    out.elem = DFX_PLANAR_F32;
    out.d_planar = d_fwd, out.d_planar_bwd = d_bwd;
    out.d_row_pitch = row_pitch_floats, out.d_plane_stride = plane_stride_floats, out.d_flow_stride = flow_stride_floats;
    out.d_occ_fwd = d_occ_fwd, out.d_occ_bwd = d_occ_bwd, out.occ_pitch = occ_pitch, out.d_occ_stride = occ_stride;
    out.alpha1 = alpha1, out.alpha2 = alpha2;
    return dfx_run_flowbuffer(h, InSpec::device(d_frames, pitch, frame_stride), n_frames, step, out, nullptr);
}

int dfx_fb_check_device(dfx_handle h, const float *d_fwd, const float *d_bwd, size_t row_pitch_floats,
                        size_t plane_stride_floats, size_t flow_stride_floats, int n, float alpha1, float alpha2,
                        uint8_t *d_occ, size_t occ_pitch, size_t occ_stride, float *d_err, size_t err_pitch_floats,
                        size_t err_stride_floats) {
    int st;
    if (!post_begin(h, true, n, &st))
        return st;
    if (!d_fwd || !d_bwd || !d_occ)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or mask planes");
    if (planar_strides_bad(h, row_pitch_floats, plane_stride_floats, flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, true, occ_pitch, occ_stride, "mask", "occ"))
        return e;
    if (int e = plane_check(h, d_err != nullptr, err_pitch_floats, err_stride_floats, "err", "err", "_floats"))
        return e;
    if (!fb_alpha_ok(alpha1) || !fb_alpha_ok(alpha2))
        return dfx_fail(h, DFX_ERR_INVALID, kFbAlpha);
    HIPCHK(h, hipSetDevice(h->device));
    FbCheckArgs a{};
    a.dir[0].f = d_fwd, a.dir[0].b = d_bwd, a.dir[0].occ = d_occ, a.dir[0].err = d_err;
    a.dirs = 1, a.n = n, a.w = h->W, a.h = h->H;
    a.row_pitch = (long long)row_pitch_floats, a.plane_stride = (long long)plane_stride_floats;
    a.flow_stride = (long long)flow_stride_floats;
    a.occ_pitch = (long long)occ_pitch, a.occ_stride = (long long)occ_stride;
    a.err_pitch = (long long)err_pitch_floats, a.err_stride = (long long)err_stride_floats;
    a.alpha1 = alpha1, a.alpha2 = alpha2;
    fb_check_launch(h->stream, a);
    return post_finish(h);
}

// ---- the backward warp of 8-bit images by a flow (warp_kernels.hip) ----
namespace {
// rows of P elements, optionally three planes, images: the stride rules of the source, reference and output images
bool warp_image_strides_bad(dfx_handle h, bool interleaved3, bool planes, size_t pitch, size_t plane, size_t image) {
    const size_t row = (size_t)h->W * (interleaved3 ? 3 : 1);
    if (pitch < row || pitch > ((size_t)1 << 40))
        return true;
    if (planes)
        return plane < (size_t)h->H * pitch || plane > ((size_t)1 << 58) || image < 3 * plane;
    return image < (size_t)h->H * pitch;
}
} // namespace

int dfx_warp_device(dfx_handle h, const dfx_warp_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_src || !d->d_flow)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device images or flows");
    if (!d->d_out && !d->d_valid && !d->d_stats)
        return dfx_fail(h, DFX_ERR_INVALID, "nothing asked for: d_out, d_valid and d_stats are all NULL");
    if (d->d_stats && !d->d_ref)
        return dfx_fail(h, DFX_ERR_INVALID, "d_stats needs d_ref");
    if (d->channels != 1 && d->channels != 3)
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be 1 or 3");
    if (d->channels == 3 && d->layout != DFX_SRC_INTERLEAVED && d->layout != DFX_SRC_PLANAR)
        return dfx_fail(h, DFX_ERR_INVALID, "layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR");
    if (d->border != DFX_WARP_BORDER_ZERO && d->border != DFX_WARP_BORDER_CLAMP)
        return dfx_fail(h, DFX_ERR_INVALID, "border must be DFX_WARP_BORDER_ZERO or DFX_WARP_BORDER_CLAMP");
    if (d->out_dtype < DFX_PLANAR_F32 || d->out_dtype > DFX_WARP_U8)
        return dfx_fail(h, DFX_ERR_INVALID, "out_dtype must be DFX_PLANAR_F32, DFX_PLANAR_F16, DFX_PLANAR_BF16 or DFX_WARP_U8");
    const bool planes = d->channels == 3 && d->layout == DFX_SRC_PLANAR, il3 = d->channels == 3 && !planes;
    if (warp_image_strides_bad(h, il3, planes, d->src_pitch, d->src_plane_stride, d->src_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "source images: a pitch or stride smaller than what it spans");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (d->d_out && warp_image_strides_bad(h, il3, planes, d->out_pitch, d->out_plane_stride, d->out_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "warped images: a pitch or stride smaller than what it spans");
    if (int e = plane_check(h, d->d_occ != nullptr, d->occ_pitch, d->occ_stride, "mask", "occ"))
        return e;
    if (int e = plane_check(h, d->d_valid != nullptr, d->valid_pitch, d->valid_stride, "valid", "valid"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    WarpArgs a{};
    a.src = d->d_src, a.ref = d->d_ref, a.flow = d->d_flow, a.out = d->d_out, a.occ = d->d_occ, a.valid = d->d_valid;
    a.stats = reinterpret_cast<unsigned long long *>(d->d_stats);
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.channels = d->channels, a.planar = planes ? 1 : 0, a.border = d->border, a.out_dtype = d->out_dtype;
    a.src_pitch = (long long)d->src_pitch, a.src_plane = (long long)d->src_plane_stride;
    a.src_image = (long long)d->src_image_stride;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.out_pitch = (long long)d->out_pitch, a.out_plane = (long long)d->out_plane_stride;
    a.out_image = (long long)d->out_image_stride;
    a.occ_pitch = (long long)d->occ_pitch, a.occ_stride = (long long)d->occ_stride;
    a.valid_pitch = (long long)d->valid_pitch, a.valid_stride = (long long)d->valid_stride;
    warp_launch(h->stream, a);
    return post_finish(h);
}

// ---- the global (camera) motion of a flow: robust fit and removal (global_motion_kernels.hip) ----
int dfx_global_motion_device(dfx_handle h, const dfx_gm_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_flow || !d->d_result)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or result records");
    if ((size_t)d->d_result % 8 != 0)
        return dfx_fail(h, DFX_ERR_INVALID, "d_result must be 8-byte aligned");
    if (d->model != DFX_GM_TRANSLATION && d->model != DFX_GM_AFFINE)
        return dfx_fail(h, DFX_ERR_INVALID, "model must be DFX_GM_TRANSLATION or DFX_GM_AFFINE");
    if (d->rounds < 1 || d->rounds > GM_MAX_ROUNDS)
        return dfx_fail(h, DFX_ERR_INVALID, "rounds must be 1 .. 8");
    if (!std::isfinite(d->thr) || !(d->thr > 0.0f))
        return dfx_fail(h, DFX_ERR_INVALID, "thr must be finite and > 0");
    if (!std::isfinite(d->growth) || !(d->growth >= 1.0f))
        return dfx_fail(h, DFX_ERR_INVALID, "growth must be finite and >= 1");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, d->d_mask != nullptr, d->mask_pitch, d->mask_stride, "mask", "mask"))
        return e;
    if (d->d_out && planar_strides_bad(h, d->out_row_pitch_floats, d->out_plane_stride_floats, d->out_flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStridesOut);
    if (int e = plane_check(h, d->d_moving != nullptr, d->moving_pitch, d->moving_stride, "moving", "moving"))
        return e;
    if (h->W > GM_MAX_SIDE || h->H > GM_MAX_SIDE)
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "the integer sums are bounded for frames of at most 8192 x 8192");
    HIPCHK(h, hipSetDevice(h->device));
    GmArgs a{};
    a.flow = d->d_flow, a.mask = d->d_mask, a.out = d->d_out, a.moving = d->d_moving, a.result = d->d_result;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.model = d->model, a.rounds = d->rounds, a.thr = d->thr, a.growth = d->growth;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.mask_pitch = (long long)d->mask_pitch, a.mask_stride = (long long)d->mask_stride;
    a.out_pitch = (long long)d->out_row_pitch_floats, a.out_plane = (long long)d->out_plane_stride_floats;
    a.out_stride = (long long)d->out_flow_stride_floats;
    a.moving_pitch = (long long)d->moving_pitch, a.moving_stride = (long long)d->moving_stride;
    gm_launch(h->stream, a);
    return post_finish(h);
}

// ---- median filter and occlusion fill of flows, mask-aware (flow_median_kernels.hip) ----
int dfx_flow_median_device(dfx_handle h, const dfx_median_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_flow || !d->d_out)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or output flows");
    if (d->ksize != 3 && d->ksize != 5)
        return dfx_fail(h, DFX_ERR_INVALID, "ksize must be 3 or 5");
    if (d->mode != DFX_MEDIAN_ALL && d->mode != DFX_MEDIAN_FILL)
        return dfx_fail(h, DFX_ERR_INVALID, "mode must be DFX_MEDIAN_ALL or DFX_MEDIAN_FILL");
    if (!d->d_mask && (d->mode == DFX_MEDIAN_FILL || d->d_mask_out))
        return dfx_fail(h, DFX_ERR_INVALID, "DFX_MEDIAN_FILL and d_mask_out need d_mask");
    if (d->d_out == d->d_flow || (d->d_mask_out && d->d_mask_out == d->d_mask))
        return dfx_fail(h, DFX_ERR_INVALID, "a stencil cannot run in place: d_out != d_flow and d_mask_out != d_mask are required");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (planar_strides_bad(h, d->out_row_pitch_floats, d->out_plane_stride_floats, d->out_flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStridesOut);
    if (int e = plane_check(h, d->d_mask != nullptr, d->mask_pitch, d->mask_stride, "mask", "mask"))
        return e;
    if (int e = plane_check(h, d->d_mask_out != nullptr, d->mask_out_pitch, d->mask_out_stride, "output mask", "mask_out"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    FmArgs a{};
    a.flow = d->d_flow, a.mask = d->d_mask, a.out = d->d_out, a.mask_out = d->d_mask_out;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.ksize = d->ksize, a.mode = d->mode;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.mask_pitch = (long long)d->mask_pitch, a.mask_stride = (long long)d->mask_stride;
    a.out_pitch = (long long)d->out_row_pitch_floats, a.out_plane = (long long)d->out_plane_stride_floats;
    a.out_stride = (long long)d->out_flow_stride_floats;
    a.mask_out_pitch = (long long)d->mask_out_pitch, a.mask_out_stride = (long long)d->mask_out_stride;
    fm_launch(h->stream, a);
    return post_finish(h);
}

// ---- adjacent flows chained into long-range flows and dense trajectories (flow_chain_kernels.hip) ----
int dfx_flow_chain_device(dfx_handle h, const dfx_chain_desc *d) {
    // post_begin's checks by hand: anchors < 0 is refused between n < 0 and the empty batch
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (h->algo == DFX_ALGO_FRAMES)
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "a DFX_ALGO_FRAMES handle computes no flow");
    if (!d)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL descriptor");
    if (d->n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (d->anchors < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "anchors must be >= 0");
    if (d->n == 0 || d->anchors == 0)
        return DFX_OK;
    if (!d->d_flow || !d->d_out)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or output flows");
    if (d->hop == 0 || d->length < 1 || d->anchor_step < 1)
        return dfx_fail(h, DFX_ERR_INVALID, "hop != 0, length >= 1 and anchor_step >= 1 are required");
    {
        // the link indices are monotone in j and in k: the four corners bound them all
        const long long j1 = (long long)(d->anchors - 1) * d->anchor_step, k1 = (long long)(d->length - 1) * d->hop;
        const long long lo = (long long)d->first + std::min(k1, 0LL), hi = (long long)d->first + j1 + std::max(k1, 0LL);
        if (lo < 0 || hi >= (long long)d->n)
            return dfx_fail(h, DFX_ERR_INVALID, "a link index first + j * anchor_step + k * hop lies outside [0, n)");
    }
    if (d->emit != DFX_CHAIN_LAST && d->emit != DFX_CHAIN_ALL)
        return dfx_fail(h, DFX_ERR_INVALID, "emit must be DFX_CHAIN_LAST or DFX_CHAIN_ALL");
    if (d->border != DFX_WARP_BORDER_ZERO && d->border != DFX_WARP_BORDER_CLAMP)
        return dfx_fail(h, DFX_ERR_INVALID, "border must be DFX_WARP_BORDER_ZERO or DFX_WARP_BORDER_CLAMP");
    if (d->d_out == d->d_flow)
        return dfx_fail(h, DFX_ERR_INVALID, "a chain cannot run in place: d_out != d_flow is required");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (planar_strides_bad(h, d->out_row_pitch_floats, d->out_plane_stride_floats, d->out_flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStridesOut);
    if (int e = plane_check(h, d->d_occ != nullptr, d->occ_pitch, d->occ_stride, "mask", "occ"))
        return e;
    if (int e = plane_check(h, d->d_valid != nullptr, d->valid_pitch, d->valid_stride, "valid", "valid"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    FcArgs a{};
    a.flow = d->d_flow, a.occ = d->d_occ, a.out = d->d_out, a.valid = d->d_valid;
    a.w = h->W, a.h = h->H;
    a.first = d->first, a.hop = d->hop, a.length = d->length, a.anchors = d->anchors, a.anchor_step = d->anchor_step;
    a.emit = d->emit, a.border = d->border;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.occ_pitch = (long long)d->occ_pitch, a.occ_stride = (long long)d->occ_stride;
    a.out_pitch = (long long)d->out_row_pitch_floats, a.out_plane = (long long)d->out_plane_stride_floats;
    a.out_stride = (long long)d->out_flow_stride_floats;
    a.valid_pitch = (long long)d->valid_pitch, a.valid_stride = (long long)d->valid_stride;
    fc_launch(h->stream, a);
    return post_finish(h);
}

// ---- forward projection of flows: inverse and time-t flows, holes marked (flow_project_kernels.hip) ----
size_t dfx_flow_project_work_bytes(dfx_handle h) {
    if (!h)
        return 0;
    return (size_t)h->W * (size_t)h->H * FP_WORDS * sizeof(unsigned long long);
}

int dfx_flow_project_device(dfx_handle h, const dfx_project_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_flow || !d->d_work)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or workspace");
    if (int e = scatter_check_params(h, d, d->scale))
        return e;
    if (d->d_out == d->d_flow)
        return dfx_fail(h, DFX_ERR_INVALID, "a projection cannot run in place: d_out != d_flow is required");
    const size_t per_flow = dfx_flow_project_work_bytes(h);
    if (int e = scatter_check_work(h, d, per_flow, "dfx_flow_project_work_bytes"))
        return e;
    const bool out_bad = d->d_out && planar_strides_bad(h, d->out_row_pitch_floats, d->out_plane_stride_floats, d->out_flow_stride_floats);
    if (int e = scatter_check_planes(h, d, out_bad, kPlanarStridesOut))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    FpArgs a{};
    scatter_fill(a, h, d);
    a.out = d->d_out, a.sc = (double)d->scale / 256.0;
    a.out_pitch = (long long)d->out_row_pitch_floats, a.out_plane = (long long)d->out_plane_stride_floats;
    a.out_stride = (long long)d->out_flow_stride_floats;
    fp_launch(h->stream, a, (long long)(d->work_bytes / per_flow));
    return post_finish(h);
}

// ---- frame interpolation at time t from two frames and their flows (interpolate_kernels.hip) ----
size_t dfx_interpolate_work_bytes(dfx_handle h, const dfx_interp_desc *d) {
    if (!h || !d)
        return 0;
    return interp_work_bytes(h->W, h->H, d->fill_passes);
}

int dfx_interpolate_device(dfx_handle h, const dfx_interp_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_img0 || !d->d_img1 || !d->d_fwd || !d->d_work)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device images, forward flows or workspace");
    if (!d->d_out && !d->d_source)
        return dfx_fail(h, DFX_ERR_INVALID, "nothing asked for: d_out and d_source are both NULL");
    if (d->d_occ_bwd && !d->d_bwd)
        return dfx_fail(h, DFX_ERR_INVALID, "d_occ_bwd needs d_bwd");
    if (!std::isfinite(d->t) || !(d->t > 0.0f) || !(d->t < 1.0f))
        return dfx_fail(h, DFX_ERR_INVALID, "t must be finite and inside (0, 1)");
    if (!std::isfinite(d->min_weight) || !(d->min_weight >= 0.0f))
        return dfx_fail(h, DFX_ERR_INVALID, "min_weight must be finite and >= 0");
    if (d->fill_passes < 0 || d->fill_passes > INTERP_MAX_PASSES)
        return dfx_fail(h, DFX_ERR_INVALID, "fill_passes must be 0 .. 16");
    if (d->ksize != 3 && d->ksize != 5)
        return dfx_fail(h, DFX_ERR_INVALID, "ksize must be 3 or 5");
    if (d->out_dtype != DFX_PLANAR_F32 && d->out_dtype != DFX_WARP_U8)
        return dfx_fail(h, DFX_ERR_INVALID, "out_dtype must be DFX_PLANAR_F32 or DFX_WARP_U8");
    if (d->channels != 1 && d->channels != 3)
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be 1 or 3");
    if (d->channels == 3 && d->layout != DFX_SRC_INTERLEAVED && d->layout != DFX_SRC_PLANAR)
        return dfx_fail(h, DFX_ERR_INVALID, "layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR");
    if ((size_t)d->d_work % 8 != 0)
        return dfx_fail(h, DFX_ERR_INVALID, "d_work must be 8-byte aligned");
    if (d->work_bytes < dfx_interpolate_work_bytes(h, d))
        return dfx_fail(h, DFX_ERR_INVALID, "work_bytes must be at least dfx_interpolate_work_bytes");
    const bool planes = d->channels == 3 && d->layout == DFX_SRC_PLANAR, il3 = d->channels == 3 && !planes;
    if (warp_image_strides_bad(h, il3, planes, d->img_pitch, d->img_plane_stride, d->img_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "images: a pitch or stride smaller than what it spans");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, d->d_occ_fwd || d->d_occ_bwd, d->occ_pitch, d->occ_stride, "mask", "occ"))
        return e;
    if (d->d_out && warp_image_strides_bad(h, il3, planes, d->out_pitch, d->out_plane_stride, d->out_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "interpolated images: a pitch or stride smaller than what it spans");
    if (int e = plane_check(h, d->d_source != nullptr, d->source_pitch, d->source_stride, "source", "source"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    InterpArgs a{};
    a.img0 = d->d_img0, a.img1 = d->d_img1, a.fwd = d->d_fwd, a.bwd = d->d_bwd;
    a.occ_fwd = d->d_occ_fwd, a.occ_bwd = d->d_occ_bwd;
    a.out = d->d_out, a.source = d->d_source, a.work = d->d_work, a.work_bytes = d->work_bytes;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.channels = d->channels, a.planar = planes ? 1 : 0, a.out_dtype = d->out_dtype;
    a.t = d->t, a.min_weight = d->min_weight, a.fill_passes = d->fill_passes, a.ksize = d->ksize;
    a.img_pitch = (long long)d->img_pitch, a.img_plane = (long long)d->img_plane_stride;
    a.img_image = (long long)d->img_image_stride;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.occ_pitch = (long long)d->occ_pitch, a.occ_stride = (long long)d->occ_stride;
    a.out_pitch = (long long)d->out_pitch, a.out_plane = (long long)d->out_plane_stride;
    a.out_image = (long long)d->out_image_stride;
    a.source_pitch = (long long)d->source_pitch, a.source_stride = (long long)d->source_stride;
    interp_launch(h->stream, a);
    return post_finish(h);
}

// ---- flows as colour images: the Middlebury wheel, unknown pixels marked (flow_colour_kernels.hip) ----
int dfx_flow_colour_device(dfx_handle h, const dfx_colour_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_flow || !d->d_out)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or colour images");
    if (d->norm != DFX_COLOUR_NORM_FIXED && d->norm != DFX_COLOUR_NORM_FLOW && d->norm != DFX_COLOUR_NORM_BATCH)
        return dfx_fail(h, DFX_ERR_INVALID, "norm must be DFX_COLOUR_NORM_FIXED, DFX_COLOUR_NORM_FLOW or DFX_COLOUR_NORM_BATCH");
    if (d->norm == DFX_COLOUR_NORM_FIXED && !(std::isfinite(d->max_rad) && d->max_rad >= 1e-6f && d->max_rad <= 1e9f))
        return dfx_fail(h, DFX_ERR_INVALID, "max_rad must be finite and in [1e-6, 1e9]");
    if (d->norm != DFX_COLOUR_NORM_FIXED && !d->d_max2)
        return dfx_fail(h, DFX_ERR_INVALID, "a measured norm needs d_max2");
    if (d->order != DFX_SRC_BGR && d->order != DFX_SRC_RGB)
        return dfx_fail(h, DFX_ERR_INVALID, "order must be DFX_SRC_BGR or DFX_SRC_RGB");
    if (d->layout != DFX_SRC_INTERLEAVED && d->layout != DFX_SRC_PLANAR)
        return dfx_fail(h, DFX_ERR_INVALID, "layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, d->d_mask != nullptr, d->mask_pitch, d->mask_stride, "mask", "mask"))
        return e;
    const bool planes = d->layout == DFX_SRC_PLANAR;
    if (warp_image_strides_bad(h, !planes, planes, d->out_pitch, d->out_plane_stride, d->out_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "colour images: a pitch or stride smaller than what it spans");
    bool fplanes = false;
    if (d->d_frame) {
        if (d->frame_channels != 1 && d->frame_channels != 3)
            return dfx_fail(h, DFX_ERR_INVALID, "frame_channels must be 1 or 3");
        if (d->frame_channels == 3 && d->frame_layout != DFX_SRC_INTERLEAVED && d->frame_layout != DFX_SRC_PLANAR)
            return dfx_fail(h, DFX_ERR_INVALID, "frame_layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR");
        fplanes = d->frame_channels == 3 && d->frame_layout == DFX_SRC_PLANAR;
        if (warp_image_strides_bad(h, d->frame_channels == 3 && !fplanes, fplanes, d->frame_pitch, d->frame_plane_stride,
                                   d->frame_image_stride))
            return dfx_fail(h, DFX_ERR_INVALID, "frames: a pitch or stride smaller than what it spans");
        if (d->alpha256 < 0 || d->alpha256 > 256)
            return dfx_fail(h, DFX_ERR_INVALID, "alpha256 must be 0 .. 256");
    }
    HIPCHK(h, hipSetDevice(h->device));
    FlowvisArgs a{};
    a.flow = d->d_flow, a.mask = d->d_mask, a.max2 = d->d_max2, a.out = d->d_out, a.frame = d->d_frame;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.mask_pitch = (long long)d->mask_pitch, a.mask_stride = (long long)d->mask_stride;
    a.out_pitch = (long long)d->out_pitch, a.out_plane = (long long)d->out_plane_stride;
    a.out_image = (long long)d->out_image_stride;
    a.norm = d->norm, a.max_rad = d->max_rad;
    a.bgr = d->order == DFX_SRC_BGR ? 1 : 0, a.planar = planes ? 1 : 0;
    a.unknown[0] = d->unknown[0], a.unknown[1] = d->unknown[1], a.unknown[2] = d->unknown[2];
    if (d->d_frame) {
        a.frame_channels = d->frame_channels, a.frame_planar = fplanes ? 1 : 0, a.alpha256 = d->alpha256;
        a.frame_pitch = (long long)d->frame_pitch, a.frame_plane = (long long)d->frame_plane_stride;
        a.frame_image = (long long)d->frame_image_stride;
    }
    flowvis_launch(h->stream, a);
    return post_finish(h);
}

// ---- motion descriptors of flows: HOF and MBH cell histograms (flow_hist_kernels.hip) ----
int dfx_flow_hist_device(dfx_handle h, const dfx_hist_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_flow)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows");
    if (!d->d_sums && !d->d_out)
        return dfx_fail(h, DFX_ERR_INVALID, "nothing asked for: d_sums and d_out are both NULL");
    if (d->kinds < 1 || d->kinds > 7)
        return dfx_fail(h, DFX_ERR_INVALID, "kinds must be a bit set of DFX_HIST_HOF, DFX_HIST_MBHX and DFX_HIST_MBHY: 1 .. 7");
    if (d->bins < 2 || d->bins > FH_MAX_BINS)
        return dfx_fail(h, DFX_ERR_INVALID, "bins must be 2 .. 16");
    if (d->cell != 4 && d->cell != 8 && d->cell != 16 && d->cell != 32)
        return dfx_fail(h, DFX_ERR_INVALID, "cell must be 4, 8, 16 or 32");
    if (d->norm < DFX_HIST_NORM_NONE || d->norm > DFX_HIST_NORM_L2)
        return dfx_fail(h, DFX_ERR_INVALID, "norm must be DFX_HIST_NORM_NONE, _L1, _L1_SQRT or _L2");
    if (!std::isfinite(d->still_thr))
        return dfx_fail(h, DFX_ERR_INVALID, "still_thr must be finite");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (int e = plane_check(h, d->d_mask != nullptr, d->mask_pitch, d->mask_stride, "mask", "mask"))
        return e;
    if ((size_t)d->d_sums % 8 != 0)
        return dfx_fail(h, DFX_ERR_INVALID, "d_sums must be 8-byte aligned");
    const size_t cw = ((size_t)h->W + d->cell - 1) / d->cell, ch = ((size_t)h->H + d->cell - 1) / d->cell;
    if (d->d_sums && d->sums_stride < ch * cw * (size_t)fh_slots(d->kinds, d->bins))
        return dfx_fail(h, DFX_ERR_INVALID, "sums_stride must be at least CH * CW * D");
    HIPCHK(h, hipSetDevice(h->device));
    FhArgs a{};
    a.flow = d->d_flow, a.mask = d->d_mask, a.sums = reinterpret_cast<long long *>(d->d_sums), a.out = d->d_out;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.mask_pitch = (long long)d->mask_pitch, a.mask_stride = (long long)d->mask_stride;
    a.sums_stride = (long long)d->sums_stride;
    a.out_slot = (long long)d->out_slot_stride_floats, a.out_col = (long long)d->out_col_stride_floats;
    a.out_row = (long long)d->out_row_stride_floats, a.out_flow = (long long)d->out_flow_stride_floats;
    a.kinds = d->kinds, a.bins = d->bins, a.cell = d->cell, a.norm = d->norm, a.still_thr = d->still_thr;
    fh_launch(h->stream, a);
    return post_finish(h);
}

// ---- forward warp (splat) of images and float payloads along a flow (splat_kernels.hip) ----
namespace {
// float32 payload planes: rows of W floats, `channels` planes (more than one only), images
bool splat_f32_strides_bad(dfx_handle h, int channels, size_t pitch, size_t plane, size_t image) {
    if (pitch < (size_t)h->W || pitch > ((size_t)1 << 40))
        return true;
    if (channels > 1)
        return plane < (size_t)h->H * pitch || plane > ((size_t)1 << 58) || image < (size_t)channels * plane;
    return image < (size_t)h->H * pitch;
}
inline bool splat_channels_ok(int src_dtype, int channels) {
    return src_dtype == DFX_WARP_U8 ? (channels == 1 || channels == 3) : (channels >= 1 && channels <= SPLAT_MAX_CHANNELS);
}
} // namespace

size_t dfx_splat_work_bytes(dfx_handle h, int channels) {
    if (!h || channels < 1 || channels > SPLAT_MAX_CHANNELS)
        return 0;
    return (size_t)h->W * (size_t)h->H * (size_t)splat_words(channels) * sizeof(unsigned long long);
}

int dfx_splat_device(dfx_handle h, const dfx_splat_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_src || !d->d_flow || !d->d_work)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device sources, flows or workspace");
    if (int e = scatter_check_params(h, d, 0.0f))
        return e;
    if (d->src_dtype != DFX_WARP_U8 && d->src_dtype != DFX_PLANAR_F32)
        return dfx_fail(h, DFX_ERR_INVALID, "src_dtype must be DFX_WARP_U8 or DFX_PLANAR_F32");
    const bool f32 = d->src_dtype == DFX_PLANAR_F32;
    if (!splat_channels_ok(d->src_dtype, d->channels))
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be 1 or 3 for an 8-bit source and 1 .. 4 for a float32 one");
    if (d->channels > 1 && (f32 ? d->layout != DFX_SRC_PLANAR : (d->layout != DFX_SRC_INTERLEAVED && d->layout != DFX_SRC_PLANAR)))
        return dfx_fail(h, DFX_ERR_INVALID, "layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR; a float32 source is planar");
    if (d->mode != DFX_SPLAT_MEAN && d->mode != DFX_SPLAT_SUM)
        return dfx_fail(h, DFX_ERR_INVALID, "mode must be DFX_SPLAT_MEAN or DFX_SPLAT_SUM");
    if (d->hole_mode != DFX_SPLAT_HOLE_ZERO && d->hole_mode != DFX_SPLAT_HOLE_KEEP)
        return dfx_fail(h, DFX_ERR_INVALID, "hole_mode must be DFX_SPLAT_HOLE_ZERO or DFX_SPLAT_HOLE_KEEP");
    if (d->out_dtype != DFX_WARP_U8 && d->out_dtype != DFX_PLANAR_F32)
        return dfx_fail(h, DFX_ERR_INVALID, "out_dtype must be DFX_WARP_U8 or DFX_PLANAR_F32");
    if (d->out_dtype == DFX_WARP_U8 && (f32 || d->mode != DFX_SPLAT_MEAN))
        return dfx_fail(h, DFX_ERR_INVALID, "out_dtype DFX_WARP_U8 needs an 8-bit source and DFX_SPLAT_MEAN");
    if (d->d_out == d->d_src)
        return dfx_fail(h, DFX_ERR_INVALID, "a splat cannot run in place: d_out != d_src is required");
    const size_t per_image = dfx_splat_work_bytes(h, d->channels);
    if (int e = scatter_check_work(h, d, per_image, "dfx_splat_work_bytes"))
        return e;
    const bool planes = d->channels > 1 && d->layout == DFX_SRC_PLANAR, il3 = d->channels == 3 && !planes;
    if (f32 ? splat_f32_strides_bad(h, d->channels, d->src_pitch, d->src_plane_stride, d->src_image_stride)
            : warp_image_strides_bad(h, il3, planes, d->src_pitch, d->src_plane_stride, d->src_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "sources: a pitch or stride smaller than what it spans");
    const bool out_bad = d->d_out && (f32 ? splat_f32_strides_bad(h, d->channels, d->out_pitch, d->out_plane_stride, d->out_image_stride)
                                          : warp_image_strides_bad(h, il3, planes, d->out_pitch, d->out_plane_stride, d->out_image_stride));
    if (int e = scatter_check_planes(h, d, out_bad, "splatted images: a pitch or stride smaller than what it spans"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    SplatArgs a{};
    scatter_fill(a, h, d);
    a.src = d->d_src, a.out = d->d_out;
    a.channels = d->channels, a.src_f32 = f32 ? 1 : 0, a.interleaved = il3 ? 1 : 0;
    a.out_u8 = d->out_dtype == DFX_WARP_U8 ? 1 : 0, a.sum = d->mode == DFX_SPLAT_SUM ? 1 : 0;
    a.keep = d->hole_mode == DFX_SPLAT_HOLE_KEEP ? 1 : 0;
    a.src_pitch = (long long)d->src_pitch, a.src_plane = (long long)d->src_plane_stride;
    a.src_image = (long long)d->src_image_stride;
    a.out_pitch = (long long)d->out_pitch, a.out_plane = (long long)d->out_plane_stride;
    a.out_image = (long long)d->out_image_stride;
    splat_launch(h->stream, a, (long long)(d->work_bytes / per_image));
    return post_finish(h);
}

// ---- backward warp of float, half and label planes along a flow (plane_warp_kernels.hip) ----
namespace {
// rows of W (planar) or C W (interleaved) elements, C planes where planar with several channels, images
bool warp_planes_strides_bad(dfx_handle h, int channels, bool interleaved, size_t pitch, size_t plane, size_t image) {
    const size_t row = (size_t)h->W * (interleaved ? (size_t)channels : 1);
    if (pitch < row || pitch > ((size_t)1 << 40))
        return true;
    if (!interleaved && channels > 1)
        return plane < (size_t)h->H * pitch || plane > ((size_t)1 << 58) || image / (size_t)channels < plane;
    return image < (size_t)h->H * pitch;
}
} // namespace

int dfx_warp_planes_device(dfx_handle h, const dfx_warp_planes_desc *d) {
    int st;
    if (!post_begin(h, d, &st))
        return st;
    if (!d->d_src || !d->d_flow)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device planes or flows");
    if (!d->d_out && !d->d_valid)
        return dfx_fail(h, DFX_ERR_INVALID, "nothing asked for: d_out and d_valid are both NULL");
    if (d->channels < 1)
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be >= 1");
    if (d->layout != DFX_SRC_INTERLEAVED && d->layout != DFX_SRC_PLANAR)
        return dfx_fail(h, DFX_ERR_INVALID, "layout must be DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR");
    if (d->border != DFX_WARP_BORDER_ZERO && d->border != DFX_WARP_BORDER_CLAMP)
        return dfx_fail(h, DFX_ERR_INVALID, "border must be DFX_WARP_BORDER_ZERO or DFX_WARP_BORDER_CLAMP");
    if (d->sample != DFX_SAMPLE_BILINEAR && d->sample != DFX_SAMPLE_NEAREST)
        return dfx_fail(h, DFX_ERR_INVALID, "sample must be DFX_SAMPLE_BILINEAR or DFX_SAMPLE_NEAREST");
    if (d->invalid != DFX_WARP_INVALID_ZERO && d->invalid != DFX_WARP_INVALID_KEEP)
        return dfx_fail(h, DFX_ERR_INVALID, "invalid must be DFX_WARP_INVALID_ZERO or DFX_WARP_INVALID_KEEP");
    if (d->src_dtype < DFX_PLANAR_F32 || d->src_dtype > DFX_WARP_U8 || d->out_dtype < DFX_PLANAR_F32 || d->out_dtype > DFX_WARP_U8)
        return dfx_fail(h, DFX_ERR_INVALID, "src_dtype and out_dtype must be DFX_PLANAR_F32, DFX_PLANAR_F16, DFX_PLANAR_BF16 or DFX_WARP_U8");
    if (d->sample == DFX_SAMPLE_BILINEAR && (d->src_dtype == DFX_WARP_U8 || d->out_dtype == DFX_WARP_U8))
        return dfx_fail(h, DFX_ERR_INVALID, "DFX_SAMPLE_BILINEAR takes and gives float32, float16 or bfloat16 (8-bit images: dfx_warp_device)");
    if (d->sample == DFX_SAMPLE_NEAREST && d->out_dtype != d->src_dtype)
        return dfx_fail(h, DFX_ERR_INVALID, "DFX_SAMPLE_NEAREST copies elements: out_dtype == src_dtype is required");
    if (d->invalid == DFX_WARP_INVALID_KEEP && !d->d_out)
        return dfx_fail(h, DFX_ERR_INVALID, "DFX_WARP_INVALID_KEEP needs d_out");
    if (d->d_out == d->d_src)
        return dfx_fail(h, DFX_ERR_INVALID, "a warp cannot run in place: d_out != d_src is required");
    const bool il = d->layout == DFX_SRC_INTERLEAVED;
    if (warp_planes_strides_bad(h, d->channels, il, d->src_pitch, d->src_plane_stride, d->src_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "source planes: a pitch or stride smaller than what it spans");
    if (planar_strides_bad(h, d->row_pitch_floats, d->plane_stride_floats, d->flow_stride_floats))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarStrides);
    if (d->d_out && warp_planes_strides_bad(h, d->channels, il, d->out_pitch, d->out_plane_stride, d->out_image_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "warped planes: a pitch or stride smaller than what it spans");
    if (int e = plane_check(h, d->d_occ != nullptr, d->occ_pitch, d->occ_stride, "mask", "occ"))
        return e;
    if (int e = plane_check(h, d->d_valid != nullptr, d->valid_pitch, d->valid_stride, "valid", "valid"))
        return e;
    HIPCHK(h, hipSetDevice(h->device));
    PwArgs a{};
    a.src = d->d_src, a.flow = d->d_flow, a.out = d->d_out, a.occ = d->d_occ, a.valid = d->d_valid;
    a.n = d->n, a.w = h->W, a.h = h->H;
    a.channels = d->channels, a.planar = il ? 0 : 1, a.border = d->border, a.sample = d->sample;
    a.keep = d->invalid == DFX_WARP_INVALID_KEEP ? 1 : 0;
    a.src_dtype = d->src_dtype, a.out_dtype = d->out_dtype;
    a.src_pitch = (long long)d->src_pitch, a.src_plane = d->channels > 1 ? (long long)d->src_plane_stride : 0;
    a.src_image = (long long)d->src_image_stride;
    a.row_pitch = (long long)d->row_pitch_floats, a.plane_stride = (long long)d->plane_stride_floats;
    a.flow_stride = (long long)d->flow_stride_floats;
    a.out_pitch = (long long)d->out_pitch, a.out_plane = d->channels > 1 ? (long long)d->out_plane_stride : 0;
    a.out_image = (long long)d->out_image_stride;
    a.occ_pitch = (long long)d->occ_pitch, a.occ_stride = (long long)d->occ_stride;
    a.valid_pitch = (long long)d->valid_pitch, a.valid_stride = (long long)d->valid_stride;
    pw_launch(h->stream, a);
    return post_finish(h);
}

// ---- caller-supplied initial flows (TVL1's useInitialFlow, Farneback's OPTFLOW_USE_INITIAL_FLOW) ----
namespace {
// which handles take a seed: upstream's BroxOpticalFlow has no initial flow, and a DFX_ALGO_FRAMES handle computes no flow
int refuse_seed(dfx_handle h) {
    if (h->algo == DFX_ALGO_TVL1 || h->algo == DFX_ALGO_FARN)
        return DFX_OK;
    return dfx_fail(h, DFX_ERR_UNSUPPORTED, h->algo == DFX_ALGO_BROX ? "brox has no initial flow (BroxOpticalFlow takes none)"
                                                                      : "a DFX_ALGO_FRAMES handle computes no flow");
}
} // namespace

int dfx_calc_batch_init(dfx_handle h, const uint8_t *const *frames, size_t frame_pitch, int n_frames, int step,
                        const float *const *init_uv, size_t init_pitch, float *const *flows_uv, size_t out_pitch) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (const int rc = refuse_seed(h))
        return rc;
    if (!init_uv)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL initial flows");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!frames || !flows_uv))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frames or flows array");
    if ((M > 0 && (pitch_too_small(h, frame_pitch) || out_pitch < (size_t)h->W * 8)) || init_pitch < (size_t)h->W * 8)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    OutSpec out;
    out.flows = flows_uv;
    out.out_pitch = out_pitch;
    InSpec in = InSpec::host(frames, frame_pitch);
    in.init = init_uv, in.init_pitch = init_pitch;
    return dfx_run_flowbuffer(h, in, n_frames, step, out, nullptr);
}

int dfx_calc_batch_init_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                               int step, const float *d_init, size_t init_stride_floats, float *d_flows,
                               size_t flow_stride_floats) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (const int rc = refuse_seed(h))
        return rc;
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    if (!d_init)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL initial flows");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_flows))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or flows");
    if ((M > 0 && (device_frames_too_small(h, pitch, frame_stride) ||
                   flow_stride_floats < (size_t)h->W * h->H * 2)) ||
        init_stride_floats < (size_t)h->W * h->H * 2)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    OutSpec out;
    out.d_flows = d_flows;
    out.d_flow_stride = flow_stride_floats;
    InSpec in = InSpec::device(d_frames, pitch, frame_stride);
    in.d_init = d_init, in.d_init_stride = init_stride_floats;
    return dfx_run_flowbuffer(h, in, n_frames, step, out, nullptr);
}

namespace {
int planar_init_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames, int step,
                       double norm_bound, int dtype, bool typed, const float *d_init, size_t init_row_pitch,
                       size_t init_plane_stride, size_t init_flow_stride, void *d_out, size_t row_pitch, size_t plane_stride,
                       size_t flow_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (!planar_dtype_ok(dtype))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarDtype);
    if (const int rc = refuse_seed(h))
        return rc;
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    if (!planar_bound_ok(norm_bound))
        return dfx_fail(h, DFX_ERR_INVALID, kPlanarBound);
    if (!d_init)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL initial flows");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_out))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or flow planes");
    if (M > 0 && device_frames_too_small(h, pitch, frame_stride))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    if (M > 0 && planar_strides_bad(h, row_pitch, plane_stride, flow_stride))
        return dfx_fail(h, DFX_ERR_INVALID, typed ? kPlanarStridesAs : kPlanarStrides);
    if (M > 0 && planar_strides_bad(h, init_row_pitch, init_plane_stride, init_flow_stride))
        return dfx_fail(h, DFX_ERR_INVALID,
                        "initial flows: init_row_pitch >= W, init_plane_stride >= H * init_row_pitch and init_flow_stride >= "
                        "2 * init_plane_stride (in floats) are required");
    OutSpec out;
    out.planar = true;
    out.norm_bound = (float)norm_bound;
    out.elem = dtype;
    out.d_planar = d_out;
    out.d_row_pitch = row_pitch, out.d_plane_stride = plane_stride, out.d_flow_stride = flow_stride;
    InSpec in = InSpec::device(d_frames, pitch, frame_stride);
    in.d_init = d_init, in.init_planar = true;
    in.d_init_stride = init_flow_stride, in.d_init_row_pitch = init_row_pitch, in.d_init_plane_stride = init_plane_stride;
    return dfx_run_flowbuffer(h, in, n_frames, step, out, nullptr);
}
} // namespace

int dfx_calc_batch_planar_init_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride,
                                      int n_frames, int step, double norm_bound, const float *d_init, float *d_out,
                                      size_t row_pitch_floats, size_t plane_stride_floats, size_t flow_stride_floats) {
    // the seed's planes have the three strides of d_out
    return planar_init_device(h, d_frames, pitch, frame_stride, n_frames, step, norm_bound, DFX_PLANAR_F32, false, d_init,
                              row_pitch_floats, plane_stride_floats, flow_stride_floats, d_out, row_pitch_floats,
                              plane_stride_floats, flow_stride_floats);
}

int dfx_calc_batch_planar_as_init_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride,
                                         int n_frames, int step, double norm_bound, int dtype, const float *d_init,
                                         size_t init_row_pitch, size_t init_plane_stride, size_t init_flow_stride,
                                         void *d_out, size_t row_pitch, size_t plane_stride, size_t flow_stride) {
    return planar_init_device(h, d_frames, pitch, frame_stride, n_frames, step, norm_bound, dtype, true, d_init,
                              init_row_pitch, init_plane_stride, init_flow_stride, d_out, row_pitch, plane_stride,
                              flow_stride);
}

int dfx_calc_batch_png_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                              int step, uint8_t *d_img_x, uint8_t *d_img_y, size_t img_pitch, size_t img_stride,
                              double *d_bounds_xy) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_img_x || !d_img_y || !d_bounds_xy))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames, image planes or bounds");
    if (M > 0 && (device_frames_too_small(h, pitch, frame_stride) || img_pitch < (size_t)h->W ||
                  img_stride < img_pitch * (size_t)h->H))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    OutSpec out;
    out.quantized = out.png = true;
    out.d_img_x = d_img_x, out.d_img_y = d_img_y, out.img_pitch = img_pitch, out.d_img_stride = img_stride;
    out.d_bounds = d_bounds_xy;
    return dfx_run_flowbuffer(h, InSpec::device(d_frames, pitch, frame_stride), n_frames, step, out, nullptr);
}

int dfx_encode_jpeg(dfx_handle h, const uint8_t *const *planes, size_t pitch, int n, int quality, uint8_t *const *jpg,
                    size_t jpg_capacity, uint32_t *sizes) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!planes || !jpg || !sizes)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL plane, JPEG buffer or size array");
    if (pitch < (size_t)h->W)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    if (quality < 1 || quality > 100)
        return dfx_fail(h, DFX_ERR_INVALID, "JPEG quality must be 1..100");
    HIPCHK(h, hipSetDevice(h->device));
    const int B = h->engine->batch();
    if (B < 1)
        return dfx_fail(h, DFX_ERR_HIP, "the engine holds no pair slots (a dfx_set_size failed for lack of memory): set a size again");
    int rc = dfx_ensure_img_staging(h, B);
    if (rc == DFX_OK)
        rc = dfx_ensure_jpeg(h, B, quality);
    if (rc != DFX_OK)
        return rc;
    const size_t plane = (size_t)h->W * h->H;
    // a staging set holds 2 * img_slots planes back to back (after dfx_set_size possibly more than the encoder is sized for)
    // and a launch takes at most DFX_GRID_YZ_MAX planes in grid.y
    const int chunk_max = (int)std::min<long long>(2ll * std::min(h->img_slots, h->jpeg.slots), DFX_GRID_YZ_MAX);
    for (int i0 = 0; i0 < n; i0 += chunk_max) {
        const int nc = std::min(chunk_max, n - i0);
        for (int j = 0; j < nc; ++j)
            HIPCHK(h, hipMemcpy2DAsync(h->d_img[0] + (size_t)j * plane, (size_t)h->W, planes[i0 + j], pitch, (size_t)h->W,
                                       (size_t)h->H, hipMemcpyHostToDevice, h->stream));
        const auto launch = [&] { return dfx_launch_jpeg(h, 0, nc, nc, 0); };
        DfxJpegCoded coded;
        if ((rc = launch()) != DFX_OK ||
            (rc = dfx_jpeg_settle(h, h->jpeg, 0, nc, /*idle=*/false, "JPEG",
                                  "JPEG: the planes do not fit the stream buffer (encode them on the host)", launch,
                                  &coded)) != DFX_OK ||
            (rc = dfx_jpeg_ensure_landing(h, h->jpeg, 0, (size_t)coded.total)) != DFX_OK) // synchronous: no tail in flight
            return rc;
        HIPCHK(h, hipMemcpyAsync(h->jpeg.h_stream[0], h->jpeg.d_stream[0], (size_t)coded.total, hipMemcpyDeviceToHost,
                                 h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        DfxHandover files;
        files.header = h->jpeg.header, files.landing = h->jpeg.h_stream[0], files.coded = coded.planes;
        files.capacity = jpg_capacity;
        for (int j = 0; j < nc; ++j) {
            files.jpg.push_back(jpg[i0 + j]);
            files.size.push_back(sizes + i0 + j);
        }
        std::string err;
        if ((rc = dfx_hand_over(files, &err)) != DFX_OK)
            return dfx_fail(h, rc, err);
    }
    return DFX_OK;
}

size_t dfx_jpeg_capacity(dfx_handle h) {
    if (!h)
        return 0;
    // header (623 bytes) + the entropy-coded segment.  A plane whose segment exceeds its pixel count (8 bits per pixel
    // BEFORE stuffing) is far outside what flow images produce; such a FlowBuffer fails with DFX_ERR_UNSUPPORTED and the
    // caller encodes its 8-bit planes (dfx_calc_batch_u8) itself.
    return (size_t)h->W * h->H + 4096;
}

int dfx_next_segments(dfx_handle h, const int *seg_frames, int n_segments) {
    if (!h)
        return DFX_ERR_INVALID;
    h->clear_segments();
    if (n_segments < 0 || (n_segments > 0 && !seg_frames))
        return dfx_fail(h, DFX_ERR_INVALID, "dfx_next_segments: NULL clip lengths");
    for (int i = 0; i < n_segments; ++i) {
        if (seg_frames[i] < 0) {
            h->clear_segments();
            return dfx_fail(h, DFX_ERR_INVALID, "dfx_next_segments: negative clip length");
        }
        h->next_segments.push_back(seg_frames[i]);
    }
    return DFX_OK;
}

int dfx_next_segments_src(dfx_handle h, const int *seg_frames, const int *seg_src_wh, const size_t *seg_pitch,
                          int n_segments, int channels) {
    if (!h)
        return DFX_ERR_INVALID;
    h->clear_segments();
    if (n_segments == 0)
        return DFX_OK;
    if (n_segments < 0 || !seg_frames || !seg_src_wh || !seg_pitch)
        return dfx_fail(h, DFX_ERR_INVALID, "dfx_next_segments_src: NULL clip lengths, sizes or pitches");
    if (channels != 1 && channels != 3)
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be 1 (gray) or 3 (BGR)");
    for (int i = 0; i < n_segments; ++i) {
        const int w = seg_src_wh[2 * i], hh = seg_src_wh[2 * i + 1];
        const char *bad = seg_frames[i] < 0                                   ? "dfx_next_segments_src: negative clip length"
                          : (w < 1 || hh < 1 || w > 32768 || hh > 32768)      ? "invalid source frame size"
                          : seg_pitch[i] < (size_t)w * (size_t)channels       ? "pitch smaller than a row"
                                                                              : nullptr;
        if (bad) {
            h->clear_segments();
            return dfx_fail(h, DFX_ERR_INVALID, bad);
        }
        h->next_segments.push_back(seg_frames[i]);
        h->next_seg_fmt.push_back({w, hh, seg_pitch[i]});
    }
    h->next_seg_ch = channels;
    return DFX_OK;
}

int dfx_wait(dfx_handle h, uint64_t ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    return dfx_finish_tails(h, ticket, -1, /*report=*/true);
}

int dfx_calc_batch_u8_device(dfx_handle h, const uint8_t *d_frames, size_t pitch, size_t frame_stride, int n_frames,
                             int step, double lower_bound, double upper_bound, uint8_t *d_img_x, uint8_t *d_img_y,
                             size_t img_pitch, size_t img_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    SegmentsScope seg_scope(h);
    if (src_segments_pending(h))
        return dfx_fail(h, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    const int M = std::max(n_frames - abs_step(step), 0);
    if (M > 0 && (!d_frames || !d_img_x || !d_img_y))
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames or image planes");
    if (M > 0 && (device_frames_too_small(h, pitch, frame_stride) || img_pitch < (size_t)h->W ||
                  img_stride < img_pitch * (size_t)h->H))
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    OutSpec out;
    out.quantized = true;
    out.lo = lower_bound;
    out.hi = upper_bound;
    out.d_img_x = d_img_x;
    out.d_img_y = d_img_y;
    out.img_pitch = img_pitch;
    out.d_img_stride = img_stride;
    return dfx_run_flowbuffer(h, InSpec::device(d_frames, pitch, frame_stride), n_frames, step, out, nullptr);
}

int dfx_flow_to_u8_device(dfx_handle h, const float *d_flows, size_t flow_stride_floats, int n, double lower_bound,
                          double upper_bound, uint8_t *d_img_x, uint8_t *d_img_y, size_t img_pitch,
                          size_t img_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!d_flows || !d_img_x || !d_img_y)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows or image planes");
    if (flow_stride_floats < (size_t)h->W * h->H * 2 || img_pitch < (size_t)h->W ||
        img_stride < img_pitch * (size_t)h->H)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    HIPCHK(h, hipSetDevice(h->device));
    quant_launch_flow_to_u8(h->stream, d_flows, (long long)flow_stride_floats, n, h->W, h->H, lower_bound,
                            upper_bound, d_img_x, d_img_y, (long long)img_pitch, (long long)img_stride);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DFX_OK;
}

int dfx_flow_to_png_device(dfx_handle h, const float *d_flows, size_t flow_stride_floats, int n, uint8_t *d_img_x,
                           uint8_t *d_img_y, size_t img_pitch, size_t img_stride, double *d_bounds_xy) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!d_flows || !d_img_x || !d_img_y || !d_bounds_xy)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device flows, image planes or bounds");
    if (flow_stride_floats < (size_t)h->W * h->H * 2 || img_pitch < (size_t)h->W ||
        img_stride < img_pitch * (size_t)h->H)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = dfx_ensure_png(h, n);
    if (rc != DFX_OK)
        return rc;
    quant_launch_flow_to_png_planes(h->stream, d_flows, (long long)flow_stride_floats, n, h->W, h->H, h->d_png_scratch,
                                    d_bounds_xy, d_img_x, d_img_y, (long long)img_pitch, (long long)img_stride);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DFX_OK;
}

namespace {
// order / layout of a colour source (DFX_SRC_*); a gray source has neither
const char *source_layout_error(int channels, int order, int layout, size_t plane_stride) {
    if ((order != DFX_SRC_BGR && order != DFX_SRC_RGB) || (layout != DFX_SRC_INTERLEAVED && layout != DFX_SRC_PLANAR))
        return "order must be DFX_SRC_BGR or DFX_SRC_RGB, layout DFX_SRC_INTERLEAVED or DFX_SRC_PLANAR";
    if (channels == 1 && (order != 0 || layout != 0 || plane_stride != 0))
        return "a gray source (channels = 1) has no channel order, layout or plane_stride";
    if (layout != DFX_SRC_PLANAR && plane_stride != 0)
        return "plane_stride applies to DFX_SRC_PLANAR only";
    return nullptr;
}
} // namespace

int dfx_set_source_format_ex(dfx_handle h, int src_width, int src_height, int channels, int order, int layout,
                             size_t plane_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    if (src_width == 0 && src_height == 0) { // back to the default: W x H gray frames
        h->default_source();
        return DFX_OK;
    }
    if (src_width < 1 || src_height < 1 || src_width > 32768 || src_height > 32768)
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source frame size");
    if (channels != 1 && channels != 3)
        return dfx_fail(h, DFX_ERR_INVALID, "channels must be 1 (gray) or 3 (BGR)");
    if (const char *why = source_layout_error(channels, order, layout, plane_stride))
        return dfx_fail(h, DFX_ERR_INVALID, why);
    if (plane_stride != 0 && plane_stride < (size_t)src_width * src_height)
        return dfx_fail(h, DFX_ERR_INVALID, "plane_stride smaller than a plane");
    if (src_width == h->W && src_height == h->H && channels == 1) {
        h->default_source();
        return DFX_OK;
    }
    h->src_w = src_width;
    h->src_h = src_height;
    h->src_ch = channels;
    h->src_rgb = order == DFX_SRC_RGB, h->src_planar = layout == DFX_SRC_PLANAR;
    h->src_plane_stride = plane_stride;
    return DFX_OK;
}

int dfx_set_source_format(dfx_handle h, int src_width, int src_height, int channels) {
    return dfx_set_source_format_ex(h, src_width, src_height, channels, DFX_SRC_BGR, DFX_SRC_INTERLEAVED, 0);
}

int dfx_prepare_frames_layout_device(dfx_handle h, const uint8_t *d_src, size_t src_pitch, size_t src_frame_stride,
                                     size_t plane_stride, int src_width, int src_height, int channels, int order,
                                     int layout, int n, uint8_t *d_gray, size_t gray_pitch, size_t gray_frame_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!d_src || !d_gray)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames");
    if (src_width < 1 || src_height < 1 || (channels != 1 && channels != 3))
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source format");
    if (const char *why = source_layout_error(channels, order, layout, plane_stride))
        return dfx_fail(h, DFX_ERR_INVALID, why);
    const bool planar = layout == DFX_SRC_PLANAR;
    const size_t one = src_pitch * (size_t)src_height, ps = plane_stride ? plane_stride : one;
    if (src_pitch < (size_t)src_width * (planar ? 1 : channels) || (planar && ps < one) ||
        src_frame_stride < (planar ? 2 * ps + one : one) || gray_pitch < (size_t)h->W ||
        gray_frame_stride < gray_pitch * (size_t)h->H)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    HIPCHK(h, hipSetDevice(h->device));
    prepare_launch(h->stream, d_src, (long long)src_pitch, (long long)src_frame_stride, src_width, src_height, channels,
                   n, d_gray, (long long)gray_pitch, (long long)gray_frame_stride, h->W, h->H, order == DFX_SRC_RGB, planar,
                   (long long)ps);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DFX_OK;
}

int dfx_prepare_frames_device(dfx_handle h, const uint8_t *d_src, size_t src_pitch, size_t src_frame_stride,
                              int src_width, int src_height, int channels, int n, uint8_t *d_gray, size_t gray_pitch,
                              size_t gray_frame_stride) {
    return dfx_prepare_frames_layout_device(h, d_src, src_pitch, src_frame_stride, 0, src_width, src_height, channels,
                                            DFX_SRC_BGR, DFX_SRC_INTERLEAVED, n, d_gray, gray_pitch, gray_frame_stride);
}

int dfx_prepare_frames_layout(dfx_handle h, const uint8_t *const *src, size_t src_pitch, int src_width, int src_height,
                              int channels, int order, int layout, int n, uint8_t *const *gray, size_t gray_pitch) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!src || !gray)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frame arrays");
    if (src_width < 1 || src_height < 1 || (channels != 1 && channels != 3))
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source format");
    if (const char *why = source_layout_error(channels, order, layout, 0))
        return dfx_fail(h, DFX_ERR_INVALID, why);
    // a channels-first frame goes up as 3 * src_height dense rows of src_width bytes
    const bool planar = layout == DFX_SRC_PLANAR;
    const int rows = planar ? 3 * src_height : src_height;
    const size_t rb = (size_t)src_width * (planar ? 1 : channels), fb = rb * rows, plane = (size_t)h->W * h->H;
    if (src_pitch < rb || gray_pitch < (size_t)h->W)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned char *d_in = nullptr, *d_out = nullptr;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / std::max(fb, plane)));
    auto run = [&]() -> int {
        HIPCHK(h, hipMalloc(&d_in, (size_t)chunk * fb));
        HIPCHK(h, hipMalloc(&d_out, (size_t)chunk * plane));
        for (int i0 = 0; i0 < n; i0 += chunk) {
            const int m = std::min(chunk, n - i0);
            for (int j = 0; j < m; ++j)
                HIPCHK(h, hipMemcpy2DAsync(d_in + (size_t)j * fb, rb, src[i0 + j], src_pitch, rb, rows,
                                           hipMemcpyHostToDevice, h->stream));
            prepare_launch(h->stream, d_in, (long long)rb, (long long)fb, src_width, src_height, channels, m, d_out,
                           h->W, (long long)plane, h->W, h->H, order == DFX_SRC_RGB, planar, 0);
            HIPCHK(h, hipGetLastError());
            for (int j = 0; j < m; ++j)
                HIPCHK(h, hipMemcpy2DAsync(gray[i0 + j], gray_pitch, d_out + (size_t)j * plane, h->W, h->W, h->H,
                                           hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
        return DFX_OK;
    };
    const int rc = run();
    dfx_free_dev(d_in);
    dfx_free_dev(d_out);
    return rc;
}

int dfx_prepare_frames(dfx_handle h, const uint8_t *const *src, size_t src_pitch, int src_width, int src_height,
                       int channels, int n, uint8_t *const *gray, size_t gray_pitch) {
    return dfx_prepare_frames_layout(h, src, src_pitch, src_width, src_height, channels, DFX_SRC_BGR, DFX_SRC_INTERLEAVED,
                                     n, gray, gray_pitch);
}

int dfx_get_stats(dfx_handle h, dfx_stats *out) {
    if (!h || !out)
        return DFX_ERR_INVALID;
    *out = h->stats;
    out->batch = h->engine ? h->engine->batch() : 0;
    return DFX_OK;
}

// Test hook, not part of the ABI (include/dfx.h does not declare it).  For every pair of the most recent device batch of
// a TVL1 handle, in pair order (the order of the batch's flows in the FlowBuffer), fills
//     iters[pair][DFX_MAX_LEVELS][DFX_MAX_WARPS]  executed inner iterations per pyramid level and warp,
//     checks[pair][DFX_MAX_LEVELS]                convergence sums evaluated per level,
// zero beyond the pyramid and the warps, and returns the number of pairs.  dfx_stats.tvl1_iters / tvl1_checks hold the
// last of these pairs only.  Valid after a synchronous call has returned, or after dfx_wait(h, 0).  Returns
// -DFX_ERR_UNSUPPORTED for a handle of another algorithm, -DFX_ERR_INVALID before any batch has completed, after a failed
// one, or when max_pairs is smaller than the batch.  However the engine dispatches a batch, the tables stay in pair
// order.
int dfxi_tvl1_batch_tables(dfx_handle h, int max_pairs, int *iters, int *checks) {
    if (!h || !h->engine)
        return -DFX_ERR_INVALID;
    if (h->algo != DFX_ALGO_TVL1)
        return -DFX_ERR_UNSUPPORTED;
    return h->engine->batch_tables(max_pairs, iters, checks);
}

void dfx_reset_stats(dfx_handle h) {
    if (h)
        std::memset(&h->stats, 0, sizeof h->stats);
}

const char *dfx_last_error(dfx_handle h) {
    if (!h)
        return g_create_error.c_str();
    thread_local std::string text; // a copy per calling thread: the collector and the owner may both ask
    text = h->get_err();
    return text.c_str();
}

void dfx_destroy(dfx_handle h) {
    if (!h)
        return;
    (void)hipSetDevice(h->device);
    (void)dfx_finish_tails(h, 0, -1);
    if (h->stream)
        (void)hipStreamSynchronize(h->stream);
    if (h->d2h_stream)
        (void)hipStreamSynchronize(h->d2h_stream);
    delete h->engine;
    h->engine = nullptr;
    if (h->copy_stream)
        (void)hipStreamSynchronize(h->copy_stream);
    for (auto &p : h->d_u8)
        dfx_free_dev(p);
    for (auto &p : h->d_flow_out)
        dfx_free_dev(p);
    for (auto &p : h->d_img)
        dfx_free_dev(p);
    for (auto &p : h->d_seed)
        dfx_free_dev(p);
    for (auto &p : h->d_src)
        dfx_free_dev(p);
    for (auto &p : h->h_in)
        dfx_free_host(p);
    for (auto &p : h->h_out)
        dfx_free_host(p);
    dfx_free_dev(h->d_png_scratch);
    for (auto &p : h->h_png_bounds)
        dfx_free_host(p);
    dfx_jpeg_free(h->jpeg);
    dfx_free_colour(h);
    dfx_destroy_events(h->ev_h2d, 2);
    dfx_destroy_events(h->ev_compute, 2);
    dfx_destroy_events(h->ev_d2h, 2);
    if (h->copy_stream)
        (void)hipStreamDestroy(h->copy_stream);
    if (h->d2h_stream)
        (void)hipStreamDestroy(h->d2h_stream);
    dfx_destroy_events(&h->ev_block, 1);
    dfx_destroy_events(&h->ev_t0, 1);
    dfx_destroy_events(&h->ev_t1, 1);
    if (h->stream)
        (void)hipStreamDestroy(h->stream);
    delete h;
}

int dfx_device_malloc(dfx_handle h, void **dptr, size_t bytes) {
    if (!h || !dptr)
        return DFX_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMalloc(dptr, bytes));
    return DFX_OK;
}

int dfx_device_free(dfx_handle h, void *dptr) {
    if (!h)
        return DFX_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipFree(dptr));
    return DFX_OK;
}

int dfx_memcpy_h2d(dfx_handle h, void *dst, const void *src, size_t bytes) {
    if (!h)
        return DFX_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return DFX_OK;
}

int dfx_memcpy_d2h(dfx_handle h, void *dst, const void *src, size_t bytes) {
    if (!h)
        return DFX_ERR_INVALID;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return DFX_OK;
}

int dfx_host_alloc(void **ptr, size_t bytes) {
    if (!ptr)
        return DFX_ERR_INVALID;
    // portable: the host shell's loader threads allocate frames that any device's handle may copy from
    return hipHostMalloc(ptr, bytes, hipHostMallocPortable) == hipSuccess ? DFX_OK : DFX_ERR_HIP;
}

int dfx_host_free(void *ptr) { return hipHostFree(ptr) == hipSuccess ? DFX_OK : DFX_ERR_HIP; }

} // extern "C"
