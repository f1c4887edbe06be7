// dfx_internal.h — host-side plumbing shared by the C ABI (dfx_api.cpp: argument checks and entry points), the two
// device-to-caller pipelines (dfx_pipeline.cpp: FlowBuffers; dfx_frames.cpp: colour frames), what they share
// (dfx_streams.cpp: deferred tails, JPEG stream state) and the per-algorithm engines (*_engine.cpp).  Nothing here
// crosses the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dfx.h"
#include "dfx_device.h"
#include "dfx_handover.h"
#include "dfx_helper.h"
#include "engine_buffers.h"
#include "engine_plan.h"

// An algorithm engine owns every device buffer of one handle.  The common driver (dfx_pipeline.cpp)
// walks a FlowBuffer in batches of `batch()` pairs, keeps the per-frame derived data (pyramids,
// polynomial expansions) in a ring of frame slots so each frame is prepared once, and calls:
//     build_frames  - prepare `n` new frames (u8 pixels already on the device) into the given slots
//     run_pairs     - compute `nb` flows (pair -> frame-slot descriptors) into d_out
//     account       - fold the finished batch into dfx_stats (after the stream is synchronised)
struct dfx_context;

class AlgoEngine {
  public:
    virtual ~AlgoEngine() {}
    virtual int create() = 0;
    // dfx_set_size: plan the engine for W x H frames (engine_plan.h) and make every buffer hold what the plan needs; a
    // buffer that is large enough stays as it is.  create() runs the same two steps on an empty engine.  The context is
    // idle.  A failure leaves the engine at its previous size, in buffers that still hold it.
    virtual int set_size(int W, int H) = 0;
    virtual size_t device_bytes() const = 0; // device memory the engine holds
    virtual int batch() const = 0;
    virtual int ensure_frame_slots(int need) = 0;
    virtual int frame_slots() const = 0;
    virtual int build_frames(const unsigned char *d_src, long long src_frame_stride, long long src_pitch, int n,
                             const int *h_slots) = 0;
    // planar != nullptr: the flows go to *planar's u and v planes (dfx_device.h) instead, d_out / out_stride unused
    // seed != nullptr: the pairs start from the caller's initial flows (DfxSeedIn, dfx_device.h: pair j of the batch is its
    // pair j) instead of zero — TVL1 and Farneback; Brox has none upstream and returns DFX_ERR_UNSUPPORTED
    virtual int run_pairs(int nb, const PairDesc *h_pairs, float *d_out, long long out_stride,
                          const DfxPlanarOut *planar = nullptr, const DfxSeedIn *seed = nullptr) = 0;
    virtual int account(int nb) = 0; // reads per-batch event timers; stream is idle
    // dfxi_tvl1_batch_tables (dfx_api.cpp): the per-pair TVL1 tables of the last accounted batch, in pair order
    virtual int batch_tables(int max_pairs, int *iters, int *checks) const {
        (void)max_pairs, (void)iters, (void)checks;
        return -DFX_ERR_UNSUPPORTED;
    }
};

// The stream state of a device JPEG encoder, gray (dfx_context::jpeg) or colour (dfx_context::colour): tables and
// per-block temporaries, and per staging parity the shared stream buffer, its page-locked landing buffer and the totals
// the device reports (dfx_streams.cpp).
struct JpegStreams {
    int quality = 0, slots = 0; // what the buffers below are sized for (slots: pairs of a flow batch / colour frames)
    int hdr_w = 0, hdr_h = 0;   // frame size `header` and `slots` were worked out for (the gray encoder: dfx_ensure_jpeg)
    size_t blocks_cap = 0, planes_cap = 0; // gray encoder: 8 x 8 blocks d_dc / d_bits hold, planes the per-plane arrays hold
    struct JpegTables *d_tab = nullptr;
    short *d_dc = nullptr;
    unsigned *d_bits = nullptr;
    unsigned long long *d_plane_bits = nullptr, *d_plane_base = nullptr;
    unsigned long long *d_hdr = nullptr; // device copy of (total, overflow): the emit pass must not poll host memory
    unsigned *d_stream[2] = {nullptr, nullptr};
    unsigned char *h_stream[2] = {nullptr, nullptr};
    size_t h_capacity[2] = {0, 0}; // page-locked landing buffers (gray: sized to what batches need, dfx_jpeg_ensure_landing)
    unsigned long long *h_info[2] = {nullptr, nullptr}, *d_info[2] = {nullptr, nullptr}; // mapped page-locked
    size_t capacity = 0;
    std::vector<unsigned char> header;
};

struct dfx_context {
    int device = 0;
    dfx_algo algo = DFX_ALGO_TVL1;
    int W = 0, H = 0;
    dfx_params prm{};
    // Last error text.  dfx_wait may run on a collector thread beside the owner's dfx_submit_*, and both may fail:
    // every access goes through set_err / get_err.
    std::string err_;
    mutable std::mutex err_mtx;
    void set_err(const std::string &m) {
        std::lock_guard<std::mutex> lock(err_mtx);
        err_ = m;
    }
    std::string get_err() const {
        std::lock_guard<std::mutex> lock(err_mtx);
        return err_;
    }
    // format of the frames handed to the calc entry points (dfx_set_source_format); 0 = the handle's own W x H gray
    int src_w = 0, src_h = 0, src_ch = 1;
    // a colour source's channel order and layout (dfx_set_source_format_ex): R, G, B instead of B, G, R; three byte planes
    // src_plane_stride bytes apart (0: pitch * src_h, the only value the host-pointer forms take) instead of interleaved
    int src_rgb = 0, src_planar = 0;
    size_t src_plane_stride = 0;
    void default_source() {
        src_w = src_h = 0, src_ch = 1;
        src_rgb = src_planar = 0, src_plane_stride = 0;
    }
    bool prepares() const { return src_w > 0; }
    int in_w() const { return prepares() ? src_w : W; }   // width / rows / bytes per row of an input frame as it is uploaded:
    int in_h() const { return prepares() ? src_h * (src_planar ? 3 : 1) : H; } // a channels-first frame is 3 * src_h rows
    size_t in_row_bytes() const { return (size_t)in_w() * (prepares() && !src_planar ? src_ch : 1); }
    // bytes from a device frame's first byte to the end of its last row, rows `pitch` bytes apart; 0: the planes overlap
    size_t in_frame_span(size_t pitch) const {
        if (!prepares() || !src_planar)
            return pitch * (size_t)in_h();
        const size_t one = pitch * (size_t)src_h, ps = src_plane_stride ? src_plane_stride : one;
        return ps < one ? 0 : 2 * ps + one;
    }

    hipStream_t stream = nullptr;      // compute
    hipStream_t copy_stream = nullptr; // host -> device copies of the host-pointer entry points
    hipStream_t d2h_stream = nullptr;  // device -> host copies: uploads of the next batch / FlowBuffer overlap them
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    hipEvent_t ev_block = nullptr; // dfx_params.blocking_sync: the event dfx_stream_wait sleeps on
    hipEvent_t ev_h2d[2] = {nullptr, nullptr};     // frames of batch i are in staging set i&1
    hipEvent_t ev_compute[2] = {nullptr, nullptr}; // flows of batch i are in staging set i&1
    hipEvent_t ev_d2h[2] = {nullptr, nullptr};     // flow staging set i&1 has been copied out

    AlgoEngine *engine = nullptr;

    // staging shared by every engine
    // host-mode staging, two sets each so that copies of batch i+-1 overlap the compute of batch i
    // The buffers are kept by their size in bytes (dfx_set_size re-plans a handle inside them); the slot counts are what
    // those bytes hold at the current W x H / source format.
    unsigned char *d_u8[2] = {nullptr, nullptr}; // u8_slots dense W*H frames per set
    int u8_slots = 0;
    float *d_flow_out[2] = {nullptr, nullptr};   // flow_slots dense H*W*2 flows per set
    int flow_slots = 0;
    // initial flows of the host-pointer seeded form (dfx_calc_batch_init): dense H*W*2 fields per set, uploaded beside the
    // frames.  Allocated at the first seeded call: a handle that never seeds holds none (seed_bytes = 0)
    float *d_seed[2] = {nullptr, nullptr};
    size_t seed_bytes = 0; // per set
    unsigned char *d_src[2] = {nullptr, nullptr}; // source-format frames before preparation (src_slots per set)
    int src_slots = 0;
    size_t src_frame_bytes = 0;
    size_t u8_bytes = 0, flow_bytes = 0, src_bytes = 0, img_bytes = 0; // per set
    // page-locked bounce buffers for FlowBuffers of small frames: one copy per batch instead of one per frame
    unsigned char *h_in[2] = {nullptr, nullptr}, *h_out[2] = {nullptr, nullptr};
    size_t h_in_bytes = 0, h_out_bytes = 0;
    unsigned char *d_img[2] = {nullptr, nullptr}; // bounded output: img_slots x planes, then img_slots y planes
    int img_slots = 0;
    // the -st=png scheme (quantize_kernels.hip): extrema / scale scratch, and per staging parity the adaptive bounds of a
    // batch in mapped page-locked memory (the kernel writes them, the host reads them after the batch's stream wait)
    void *d_png_scratch = nullptr;
    double *h_png_bounds[2] = {nullptr, nullptr}, *d_png_bounds[2] = {nullptr, nullptr};
    int png_slots = 0;
    // device JPEG encoder (jpeg_kernels.hip): tables + per-block temporaries (one set, compute stream only), and per
    // staging parity the shared stream buffer, its page-locked landing buffer and the totals the device reports
    JpegStreams jpeg;
    // colour frame extraction (dfx_frames.cpp: dfx_extract_frames / dfx_encode_jpeg_bgr): the colour encoder's stream state
    // (d_tab is [2]: luminance, chrominance; a slot is a frame); per staging parity the source-size BGR frames; the
    // resized frames (one set: written and read on the compute stream).  Row pitches are multiples of 4
    // (jpeg_colour_kernels.hip reads dwords).
    struct ColourState : JpegStreams {
        unsigned char *d_src[2] = {nullptr, nullptr}; // src_slots source-size frames per parity
        int src_slots = 0;
        size_t src_pitch = 0, src_frame_bytes = 0;
        unsigned char *d_bgr = nullptr; // bgr_slots frames of W x H (only when the source size differs)
        int bgr_slots = 0;
        // what the buffers hold, in bytes (they only grow: dfx_frames.cpp ensure_colour); info_slots: frames h_info holds
        size_t src_cap[2] = {0, 0}, bgr_cap = 0, tab_cap = 0, dc_cap = 0, bits_cap = 0, pbits_cap = 0, pbase_cap = 0,
               hdr_cap = 0, stream_cap[2] = {0, 0};
        int info_slots = 0;
        unsigned long long seq = 0;   // device batches are numbered across calls: parity = seq & 1
        size_t device_bytes = 0;      // device memory held by this state
    } colour;
    DfxHelper helper;              // host-side work beside the calling thread (dfx_helper.h): one thread per handle
    std::vector<int> h_slots;      // slot id of each new frame of the current batch
    std::vector<PairDesc> h_pairs; // descriptors of the current batch

    dfx_stats stats{};

    // Batches are numbered across calls: staging set, bounce buffer and event of batch q are those of parity q & 1.
    unsigned long long batch_seq = 0;
    std::vector<int> next_segments; // dfx_next_segments: clip lengths of the NEXT FlowBuffer (consumed by that call)
    // dfx_next_segments_src: with every clip's own source format (one entry per clip, or none), channels common to them
    struct SegFormat {
        int w, h;
        size_t pitch;
    };
    std::vector<SegFormat> next_seg_fmt;
    int next_seg_ch = 1;
    void clear_segments() {
        next_segments.clear();
        next_seg_fmt.clear();
        next_seg_ch = 1;
    }
    // Deferred tails of dfx_submit_*: the last download of a FlowBuffer (and, for small frames, the hand-over from
    // the bounce buffer to the caller's buffers) completes on a helper thread while the next FlowBuffer is issued.
    // A tail stays registered in `tails` until its worker has FINISHED (done, set under tails_mtx): whoever asks about
    // a ticket or a staging parity — the collector's dfx_wait, the submitting thread's bounce-buffer guard, a
    // re-allocation — sees it and blocks on tails_cv until then.  Only finished tails are removed and joined.
    struct Tail {
        unsigned long long ticket = 0;
        int parity = 0;
        int rc = DFX_OK;
        std::string err;
        bool done = false;
        std::thread worker;
    };
    struct TailError { // a failed tail's status is kept until a dfx_wait that covers its ticket has reported it
        unsigned long long ticket;
        int rc;
        std::string err;
    };
    std::deque<std::unique_ptr<Tail>> tails;
    std::vector<TailError> tail_errors;
    std::mutex tails_mtx; // dfx_wait may be called from another thread than the one that submits
    std::condition_variable tails_cv;
    unsigned long long next_ticket = 1;
};

// Wait until the deferred tails with ticket <= up_to (0 = all) / of staging parity `parity` (-1 = any) have finished.
// report = true (dfx_wait): returns, and forgets, the first error of a tail with ticket <= up_to; report = false
// (housekeeping inside other entry points): errors stay recorded for the dfx_wait of their ticket.
int dfx_finish_tails(dfx_context *c, unsigned long long up_to, int parity, bool report = false);

// The deferred tail of a dfx_submit_* call: a worker waits for `event` (the last download of staging parity `parity`),
// runs `work` (which owns copies of all it touches; it returns a status and fills the error text) and publishes the
// outcome.  Returns the tail's ticket.
unsigned long long dfx_defer_tail(dfx_context *c, int parity, hipEvent_t event, std::function<int(std::string *)> work);
// An error return may leave asynchronous copies in flight that target caller-owned (often pool-recycled) buffers: drain
// every stream and every deferred tail before handing the error back.  The error text survives.
void dfx_drain_after_error(dfx_context *c);

#define HIPCHK(ctx, call)                                                                                       \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess) {                                                                                 \
            char buf_[512];                                                                                     \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,        \
                     __LINE__);                                                                                 \
            (ctx)->set_err(buf_);                                                                                 \
            return DFX_ERR_HIP;                                                                                 \
        }                                                                                                       \
    } while (0)

// Event flags of the hot path's events: with dfx_params.blocking_sync a hipEventSynchronize sleeps instead of spinning.
inline unsigned dfx_event_flags(const dfx_context *c, bool timing) {
    return (timing ? 0u : (unsigned)hipEventDisableTiming) | (c->prm.blocking_sync ? (unsigned)hipEventBlockingSync : 0u);
}
// hipStreamSynchronize spins (the device flags are whatever the process set up before this library saw the device);
// with blocking_sync the wait goes through a blocking event instead.  One waiter per context at a time (the calling
// thread of the calc / submit entry points).
inline hipError_t dfx_stream_wait(dfx_context *c, hipStream_t s) {
    if (!c->prm.blocking_sync || !c->ev_block)
        return hipStreamSynchronize(s);
    const hipError_t e = hipEventRecord(c->ev_block, s);
    return e != hipSuccess ? e : hipEventSynchronize(c->ev_block);
}

inline int dfx_fail(dfx_context *c, int code, const std::string &msg) {
    if (c)
        c->set_err(msg);
    return code;
}

template <class T> inline void dfx_free_dev(T *&p) {
    if (p) {
        (void)hipFree(p);
        p = nullptr;
    }
}
template <class T> inline void dfx_free_host(T *&p) {
    if (p) {
        (void)hipHostFree(p);
        p = nullptr;
    }
}

// The allocator policy of engine_buffers.h on HIP: the engines' buffers and tables grow through it.
struct DfxHipAlloc {
    dfx_context *c;
    static int checked(hipError_t e, void **p) {
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
        }
        return (int)e;
    }
    int dev(void **p, size_t bytes) { return checked(hipMalloc(p, bytes), p); }
    int pinned(void **p, size_t bytes) { return checked(hipHostMalloc(p, bytes, hipHostMallocDefault), p); }
    void free_dev(void *p) { (void)hipFree(p); }
    void free_pinned(void *p) { (void)hipHostFree(p); }
    int free_bytes(size_t *out) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        *out = free_b;
        return 0;
    }
    void failed(size_t bytes, int code) {
        char buf[256];
        snprintf(buf, sizeof buf, "allocating %zu bytes failed: %s", bytes, hipGetErrorString((hipError_t)code));
        c->set_err(buf);
    }
};

inline void dfx_destroy_events(hipEvent_t *ev, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (ev[i]) {
            (void)hipEventDestroy(ev[i]);
            ev[i] = nullptr;
        }
}

// The level table of dfx_stats, the tail of every engine's account(): size_of(l) is level l's (width, height).
template <class F> inline void dfx_stats_levels(dfx_stats &st, size_t n, F size_of) {
    st.levels = (int)std::min<size_t>(n, DFX_MAX_LEVELS);
    for (int l = 0; l < st.levels; ++l) {
        const auto wh = size_of(l);
        st.level_w[l] = wh.first;
        st.level_h[l] = wh.second;
    }
}

// Grow a set of buffers that is sized for `count` slots to `need`: nothing may use the old ones (deferred tails, device
// work), and `alloc` — which frees them and allocates the new ones — may fail half-way.
template <class N, class F> inline int dfx_regrow(dfx_context *c, N &count, N need, F alloc) {
    (void)dfx_finish_tails(c, 0, -1);
    HIPCHK(c, hipDeviceSynchronize());
    count = 0; // a failed allocation below must not leave the old size standing
    const int rc = alloc();
    if (rc == DFX_OK)
        count = need;
    return rc;
}

// dfx_set_size: the shared staging of dfx_pipeline.cpp re-counted for the context's new W x H (nothing is allocated)
void dfx_pipeline_resized(dfx_context *c);
// dfx_set_size: the colour state follows the new W x H at its next use (dfx_frames.cpp)
void dfx_colour_resized(dfx_context *c);

// ---- JPEG stream state (dfx_streams.cpp) ----
void dfx_jpeg_free(JpegStreams &j);
// Both stream buffers and both landing buffers re-sized to hold `need` bytes, all or nothing: a failure leaves the
// encoder as it was.  *delta (optional) receives the change in device bytes.  `noun` names the encoder in the error.
int dfx_jpeg_grow(dfx_context *c, JpegStreams &j, unsigned long long need, const char *noun, size_t *delta = nullptr);
// The landing buffer of parity q holds at least `need` bytes.  Nothing reads or writes h_stream[q] when this is called.
int dfx_jpeg_ensure_landing(dfx_context *c, JpegStreams &j, int q, size_t need);
struct DfxJpegCoded { // what the device reports for one coded batch
    unsigned long long total = 0;     // bytes of the batch's streams in d_stream[parity]
    std::vector<DfxCodedPlane> planes;
};
// After the encode of `n` planes has been launched on the compute stream into parity q: wait for it (idle = true: the
// caller already has), and if the streams did not fit the shared buffer, grow it to what the scan pass measured, `launch`
// the encode once more and wait again.  Still no fit: DFX_ERR_UNSUPPORTED with `no_fit` as the text.
int dfx_jpeg_settle(dfx_context *c, JpegStreams &j, int q, int n, bool idle, const char *noun, const char *no_fit,
                    const std::function<int()> &launch, DfxJpegCoded *out, size_t *delta = nullptr);

AlgoEngine *dfx_make_tvl1_engine(dfx_context *c);
AlgoEngine *dfx_make_farneback_engine(dfx_context *c);
AlgoEngine *dfx_make_brox_engine(dfx_context *c);
AlgoEngine *dfx_make_frames_engine(dfx_context *c); // DFX_ALGO_FRAMES: no flow state at all (dfx_frames.cpp)
void dfx_free_colour(dfx_context *c);               // dfx_destroy: the buffers of dfx_context::colour
