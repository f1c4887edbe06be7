// dfx_pipeline.cpp — the FlowBuffer driver that is common to every algorithm: staging, the upload / compute / download
// schedule over device batches, the bounded / PNG / JPEG output stages and the hand-over to the caller's buffers.
//
// Reference behaviour mirrored: DenseFlow::calc_optflows_imp, /root/reference/src/denseflow_gpu.cpp
// :282-370 — pair selection :315-316, per-pair upload/calc/download :317-339, M = max(N-|step|,0)
// flows per FlowBuffer :307-308.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "dfx_pipeline.h"
#include "dfx_plan.h"
#include "fb_check_kernels.h"
#include "jpeg_kernels.h"
#include "prepare_kernels.h"
#include "quantize_kernels.h"

namespace {

// both buffers of a staging pair, freed and allocated anew (device memory, or page-locked host memory)
template <class T> int realloc_pair(dfx_context *c, T *(&pair)[2], size_t bytes, bool host = false) {
    for (auto &p : pair) {
        if (host) {
            dfx_free_host(p);
            HIPCHK(c, hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
        } else {
            dfx_free_dev(p);
            HIPCHK(c, hipMalloc((void **)&p, bytes));
        }
    }
    return DFX_OK;
}

// The staging sets are kept by their size in bytes and only grow: a set that holds `need` slots at the current frame size
// (after dfx_set_size or another source format: more or fewer than it was allocated for) is used as it is.
int ensure_src_staging(dfx_context *c, int need, size_t fb) { // fb: bytes of a staging slot (the largest source frame)
    if (fb != c->src_frame_bytes) { // another source format: re-count what the buffers hold
        c->src_frame_bytes = fb;
        c->src_slots = dfx_slots_in(c->src_bytes, fb);
    }
    if (need <= c->src_slots)
        return DFX_OK;
    return dfx_regrow(c, c->src_slots, need, [&]() -> int {
        c->src_bytes = 0;
        const int rc = realloc_pair(c, c->d_src, (size_t)need * fb);
        if (rc == DFX_OK)
            c->src_bytes = (size_t)need * fb;
        return rc;
    });
}

int ensure_bounce(dfx_context *c, size_t in_bytes, size_t out_bytes) {
    int rc = DFX_OK;
    if (in_bytes > c->h_in_bytes)
        rc = dfx_regrow(c, c->h_in_bytes, in_bytes, [&] { return realloc_pair(c, c->h_in, in_bytes, true); });
    if (rc == DFX_OK && out_bytes > c->h_out_bytes)
        rc = dfx_regrow(c, c->h_out_bytes, out_bytes, [&] { return realloc_pair(c, c->h_out, out_bytes, true); });
    return rc;
}

int ensure_staging(dfx_context *c, int u8_need, int flow_need) {
    const size_t plane = (size_t)c->W * c->H;
    int rc = DFX_OK;
    if (u8_need > c->u8_slots)
        rc = dfx_regrow(c, c->u8_slots, u8_need, [&]() -> int {
            c->u8_bytes = 0;
            const int arc = realloc_pair(c, c->d_u8, (size_t)u8_need * plane);
            if (arc == DFX_OK)
                c->u8_bytes = (size_t)u8_need * plane;
            return arc;
        });
    if (rc == DFX_OK && flow_need > c->flow_slots)
        rc = dfx_regrow(c, c->flow_slots, flow_need, [&]() -> int {
            c->flow_bytes = 0;
            const int arc = realloc_pair(c, c->d_flow_out, (size_t)flow_need * plane * 2 * sizeof(float));
            if (arc == DFX_OK)
                c->flow_bytes = (size_t)flow_need * plane * 2 * sizeof(float);
            return arc;
        });
    return rc;
}

// The staging pair of the host-pointer seeded form: `need` dense initial flows per set, kept by its size in bytes like
// the others.  First allocated by the first seeded call of a handle.
int ensure_seed_staging(dfx_context *c, int need) {
    const size_t bytes = (size_t)need * c->W * c->H * 2 * sizeof(float);
    if (bytes <= c->seed_bytes)
        return DFX_OK;
    size_t held = c->seed_bytes;
    return dfx_regrow(c, held, bytes, [&]() -> int {
        c->seed_bytes = 0;
        const int rc = realloc_pair(c, c->d_seed, bytes);
        if (rc == DFX_OK)
            c->seed_bytes = bytes;
        return rc;
    });
}

// One frame / plane between host and device.  Dense rows (pitch == row bytes on both sides) go as ONE linear copy:
// a 2-D copy of a small frame costs several times the linear one, and a FlowBuffer of 224x224 frames is hundreds
// of them.
inline hipError_t copy_rows_async(void *dst, size_t dpitch, const void *src, size_t spitch, size_t row_bytes,
                                  size_t rows, hipMemcpyKind kind, hipStream_t s) {
    if (dpitch == row_bytes && spitch == row_bytes)
        return hipMemcpyAsync(dst, src, row_bytes * rows, kind, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, row_bytes, rows, kind, s);
}

// One FlowBuffer on its way through the device, for host- and device-resident frames.
//   host mode  : in.frames[i] host pointers, results to host pointers.  Copies run on their own streams through two
//                staging sets: the frames of batch i+1 go up and the flows of batch i-1 come down while batch i computes
//                (the reference uploads, computes and downloads one pair at a time with a blocking download, :317-339).
//   device mode: in.d_frames / out.d_* contiguous device arrays, no copies at all.
// The handle's helper thread runs host-side work of the neighbouring batches and reads this object: the destructor
// finishes its job on every path out.
struct FlowRun {
    dfx_context *c;
    const InSpec &in;
    const OutSpec &out;
    const int step;
    AlgoEngine *E = nullptr;
    DfxPairs pairs;
    std::vector<DfxBatchPlan> plan;
    unsigned long long seq0 = 0; // batches are numbered across calls (q = seq0 + k): see par()
    int F = 0;                   // frame slots of the engine: frame id f lives in slot f % F
    bool host_mode = false, prep = false, bounce_in = false, bounce = false;
    size_t plane = 0;
    std::vector<DfxJpegCoded> coded; // JPEG mode: what the device reported for each batch
    // Source format of the host frames.  Normally the handle's (dfx_set_source_format) for every frame; under
    // dfx_next_segments_src every clip has its own size and pitch (clip_fmt, clip_of[frame id]), and the staging slots
    // are sized for the largest of them.  Rows are dense in the staging set.
    std::vector<dfx_context::SegFormat> clip_fmt;
    std::vector<int> clip_of;
    int seg_ch = 1, src_ch = 1;
    size_t src_stride = 0; // bytes between the frames of a staging set / bounce buffer
    dfx_context::SegFormat fmt(long long f) const {
        if (clip_fmt.empty())
            return {c->in_w(), c->in_h(), in.frame_pitch};
        return clip_fmt[clip_of[(size_t)f]];
    }

    FlowRun(dfx_context *ctx, const InSpec &i, const OutSpec &o, int s) : c(ctx), in(i), out(o), step(s) {}
    ~FlowRun() { (void)c->helper.finish(); }
    // batch k uses staging set / bounce buffer / events of this parity
    int par(size_t k) const { return (int)((seq0 + k) & 1ull); }
    // bytes of one value of a float flow on its way out: 4, or 2 for the half planes of dfx_calc_batch_planar_as*
    size_t out_elem_bytes() const { return out.planar ? (size_t)dfx_elem_bytes(out.elem) : 4; }
    int prepare(const std::vector<int> &seg);
    int run(uint64_t *ticket);
    int upload(size_t k);
    int download(size_t k);
    DfxHandover describe(size_t k) const;
    int hand_over(size_t k);
    int overlap_copies(size_t k);
    int compute(size_t k);
    int backward(const DfxBatchPlan &p, const DfxPlanarOut &fwd);
    int launch_jpeg(size_t k);
    int finish(uint64_t *ticket);
};

// Pairs, engine frame slots, staging, the bounce decision and the batch plan.  Leaves plan empty for M = 0.
int FlowRun::prepare(const std::vector<int> &seg) {
    pairs = dfx_build_pairs(seg, step); // dfx_plan.h: pure host logic, CPU-tested
    const int M = pairs.size();
    if (M == 0)
        return DFX_OK;
    HIPCHK(c, hipSetDevice(c->device));
    E = c->engine;
    int B = E->batch();
    if (B < 1) // a dfx_set_size that failed could not even get the engine's old buffers back
        return dfx_fail(c, DFX_ERR_HIP, "the engine holds no pair slots (a dfx_set_size failed for lack of memory): set a size again");
    const int F_need = std::max(dfx_frames_needed(pairs, B), std::min(B, M) + std::abs(step));
    int rc = E->ensure_frame_slots(F_need);
    host_mode = in.frames != nullptr;
    // float flows land in the caller's device array, or in a staging set when they are copied to the host
    // or only feed the bounding kernel
    // inputs are source-format frames: convert / resize them on the device first
    prep = c->prepares() || !clip_fmt.empty();
    // (bytes per pixel of an uploaded row: a channels-first frame goes up as 3 * src_h rows of one byte per pixel)
    src_ch = !clip_fmt.empty() ? seg_ch : c->prepares() && !c->src_planar ? c->src_ch : 1;
    src_stride = c->in_row_bytes() * c->in_h();
    if (!clip_fmt.empty()) {
        src_stride = 0;
        for (size_t s = 0; s < clip_fmt.size(); ++s) {
            src_stride = std::max(src_stride, (size_t)clip_fmt[s].w * src_ch * clip_fmt[s].h);
            clip_of.insert(clip_of.end(), (size_t)seg[s], (int)s);
        }
    }
    if (rc == DFX_OK)
        rc = ensure_staging(c, (host_mode || prep) ? F_need : 0, (host_mode || out.quantized) ? B : 0);
    if (rc == DFX_OK && prep && host_mode)
        rc = ensure_src_staging(c, F_need, src_stride);
    if (rc == DFX_OK && in.init) // host-pointer seeds go up beside the frames
        rc = ensure_seed_staging(c, B);
    if (rc == DFX_OK && out.quantized && host_mode)
        rc = dfx_ensure_img_staging(c, B);
    if (rc == DFX_OK && out.jpeg)
        rc = dfx_ensure_jpeg(c, B, out.quality);
    if (rc == DFX_OK && out.png)
        rc = dfx_ensure_png(c, B);
    if (rc != DFX_OK)
        return rc;
    plane = (size_t)c->W * c->H;
    // Small frames: an asynchronous copy costs ~10 us of driver time whatever its size, and a 300-frame clip of
    // 224x224 frames is ~900 of them (a third of the batch's compute time).  Such FlowBuffers go through page-locked
    // bounce buffers instead: the host gathers / scatters the frames with memcpy and the copy stream moves one block
    // per batch and direction.
    const size_t in_fb = src_stride;
    const size_t out_pb = out.quantized ? 2 * plane : plane * 2 * out_elem_bytes(); // bytes per pair leaving the device
    // Decided per direction: a 224x224 frame is 50 KB (gathered), but its float flow is 401 KB — one direct copy per
    // flow (~10 us of driver time) is cheaper than a second pass of host memcpy over 120 MB per clip.
    bounce_in = host_mode && in_fb <= (256u << 10) && (size_t)F_need * in_fb <= (256u << 20);
    bounce = !out.jpeg && bounce_in && out_pb <= (256u << 10) && (size_t)B * out_pb <= (256u << 20); // results
    if (bounce_in) {
        rc = ensure_bounce(c, (size_t)F_need * in_fb, bounce ? (size_t)B * out_pb : 0);
        if (rc != DFX_OK)
            return rc;
    } else if (host_mode && M <= B && M >= 32) {
        // Large frames, and the whole FlowBuffer would be one batch: nothing could overlap its copies.  Two balanced
        // batches put the second upload and the first download under the compute (the engine's batch is sized for
        // the device-resident path, where a bigger batch is simply better: 336 / 362 pairs/s at 32 / 128 for TVL1).
        B = (M + 1) / 2;
    }
    F = E->frame_slots();
    c->h_slots.resize(F);
    c->h_pairs.resize(B);
    // Frames [lo of its first pair, hi of its last pair] must be resident for a batch; earlier batches already prepared
    // the ids below their own end.  Frame id f lives in slot f % F; F >= that range, so a batch never evicts what it needs.
    plan = dfx_plan_batches(pairs, B);
    seq0 = c->batch_seq;
    c->batch_seq += plan.size();
    coded.resize(out.jpeg ? plan.size() : 0);
    return DFX_OK;
}

int FlowRun::upload(size_t k) { // host frames of batch k -> staging set par(k) (upload stream)
    const DfxBatchPlan &p = plan[k];
    const int q = par(k);
    const size_t fb = src_stride;
    unsigned char *dst = prep ? c->d_src[q] : c->d_u8[q];
    // the staging set was last read by the frame preparation of batch q-2 (compute stream)
    if (seq0 + k >= 2)
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_compute[q], 0));
    if (bounce_in) {
        if (seq0 + k >= 2) // the copy that last read this bounce buffer (batch q-2) has long finished; make it formal
            HIPCHK(c, hipEventSynchronize(c->ev_h2d[q]));
        unsigned char *hb = c->h_in[q];
        for (int j = 0; j < p.n_new; ++j) {
            const auto f = fmt(p.first_new + j);
            const size_t rb = (size_t)f.w * src_ch;
            dfx_copy_rows(hb + (size_t)j * fb, rb, in.frames[p.first_new + j], f.pitch, rb, f.h);
        }
        if (p.n_new > 0)
            HIPCHK(c, hipMemcpyAsync(dst, hb, (size_t)p.n_new * fb, hipMemcpyHostToDevice, c->copy_stream));
    } else {
        for (int j = 0; j < p.n_new; ++j) {
            const auto f = fmt(p.first_new + j);
            const size_t rb = (size_t)f.w * src_ch;
            HIPCHK(c, copy_rows_async(dst + (size_t)j * fb, rb, in.frames[p.first_new + j], f.pitch, rb, f.h,
                                      hipMemcpyHostToDevice, c->copy_stream));
        }
    }
    if (in.init) // the initial flows of the batch's pairs, dense in staging set q (last read by the compute of batch q-2)
        for (int j = 0; j < p.nb; ++j)
            HIPCHK(c, copy_rows_async(c->d_seed[q] + (size_t)j * plane * 2, (size_t)c->W * 8, in.init[p.i0 + j], in.init_pitch,
                                      (size_t)c->W * 8, c->H, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->ev_h2d[q], c->copy_stream));
    return DFX_OK;
}

int FlowRun::download(size_t k) { // results of batch k: staging set par(k) -> host (download stream)
    const DfxBatchPlan &p = plan[k];
    const int q = par(k);
    HIPCHK(c, hipStreamWaitEvent(c->d2h_stream, c->ev_compute[q], 0));
    if (out.jpeg || bounce) {
        // one block (JPEG: the entropy-coded segments; bounce: one per plane kind) that hand_over(k) turns into the caller's
        // files / rows later.  A deferred tail of an earlier FlowBuffer may still be reading this landing / bounce buffer.
        const int trc = dfx_finish_tails(c, 0, q);
        if (trc != DFX_OK)
            return trc;
    }
    if (out.jpeg) {
        if (coded[k].total > 0) {
            const int grc = dfx_jpeg_ensure_landing(c, c->jpeg, q, (size_t)coded[k].total);
            if (grc != DFX_OK)
                return grc;
            HIPCHK(c, hipMemcpyAsync(c->jpeg.h_stream[q], c->jpeg.d_stream[q], (size_t)coded[k].total,
                                     hipMemcpyDeviceToHost, c->d2h_stream));
        }
    } else if (bounce) {
        unsigned char *hb = c->h_out[q];
        if (out.quantized) {
            HIPCHK(c, hipMemcpyAsync(hb, c->d_img[q], (size_t)p.nb * plane, hipMemcpyDeviceToHost, c->d2h_stream));
            HIPCHK(c, hipMemcpyAsync(hb + (size_t)p.nb * plane, c->d_img[q] + (size_t)c->img_slots * plane,
                                     (size_t)p.nb * plane, hipMemcpyDeviceToHost, c->d2h_stream));
        } else {
            HIPCHK(c, hipMemcpyAsync(hb, c->d_flow_out[q], (size_t)p.nb * plane * 2 * out_elem_bytes(), hipMemcpyDeviceToHost,
                                     c->d2h_stream));
        }
    } else {
        for (int j = 0; j < p.nb; ++j) {
            if (out.quantized) {
                const unsigned char *sx = c->d_img[q] + (size_t)j * plane;
                const unsigned char *sy = c->d_img[q] + ((size_t)c->img_slots + j) * plane;
                HIPCHK(c, copy_rows_async(out.img_x[p.i0 + j], out.img_pitch, sx, c->W, c->W, c->H,
                                          hipMemcpyDeviceToHost, c->d2h_stream));
                HIPCHK(c, copy_rows_async(out.img_y[p.i0 + j], out.img_pitch, sy, c->W, c->W, c->H,
                                          hipMemcpyDeviceToHost, c->d2h_stream));
            } else if (out.planar) { // staged dense: the u plane of flow j, then its v plane (W * elem bytes per row)
                const size_t e = out_elem_bytes(), rb = (size_t)c->W * e;
                const unsigned char *su = reinterpret_cast<const unsigned char *>(c->d_flow_out[q]) + (size_t)j * plane * 2 * e;
                HIPCHK(c, copy_rows_async(out.flows_u[p.i0 + j], out.out_pitch, su, rb, rb, c->H, hipMemcpyDeviceToHost,
                                          c->d2h_stream));
                HIPCHK(c, copy_rows_async(out.flows_v[p.i0 + j], out.out_pitch, su + plane * e, rb, rb, c->H,
                                          hipMemcpyDeviceToHost, c->d2h_stream));
            } else {
                HIPCHK(c, copy_rows_async(out.flows[p.i0 + j], out.out_pitch, c->d_flow_out[q] + (size_t)j * plane * 2,
                                          (size_t)c->W * 8, (size_t)c->W * 8, c->H, hipMemcpyDeviceToHost,
                                          c->d2h_stream));
            }
        }
    }
    HIPCHK(c, hipEventRecord(c->ev_d2h[q], c->d2h_stream));
    return DFX_OK;
}

// What is left to do on the host for batch k once its download has arrived (nothing for direct copies).  Valid from
// download(k) on: that call settles which landing buffer the batch uses.
DfxHandover FlowRun::describe(size_t k) const {
    const DfxBatchPlan &p = plan[k];
    DfxHandover h;
    if (out.jpeg) { // header + byte-stuffed segment + EOI for every plane of the batch: its x planes, then its y planes
        h.header = c->jpeg.header;
        h.landing = c->jpeg.h_stream[par(k)];
        h.coded = coded[k].planes;
        h.capacity = out.jpg_capacity;
        h.too_small = "JPEG: jpg_capacity is too small for an encoded plane (encode this FlowBuffer's 8-bit planes on the host)";
        for (int j = 0; j < 2 * p.nb; ++j) {
            const bool is_y = j >= p.nb;
            const int i = p.i0 + (is_y ? j - p.nb : j);
            h.jpg.push_back(is_y ? out.jpg_y[i] : out.jpg_x[i]);
            h.size.push_back((is_y ? out.size_y : out.size_x) + i);
        }
    } else if (bounce) {
        h.block = c->h_out[par(k)];
        h.two_planes = out.quantized;
        h.float_planes = out.planar;
        h.elem_bytes = out_elem_bytes();
        h.W = c->W, h.H = c->H;
        h.pitch = out.quantized ? out.img_pitch : out.out_pitch;
        for (int j = 0; j < p.nb; ++j) {
            if (out.quantized) {
                h.dst_a.push_back(out.img_x[p.i0 + j]);
                h.dst_b.push_back(out.img_y[p.i0 + j]);
            } else if (out.planar) {
                h.dst_a.push_back(out.flows_u[p.i0 + j]);
                h.dst_b.push_back(out.flows_v[p.i0 + j]);
            } else {
                h.dst_a.push_back(out.flows[p.i0 + j]);
            }
        }
    }
    return h;
}

int FlowRun::hand_over(size_t k) { // results of batch k -> the caller's buffers, on the calling or the helper thread
    HIPCHK(c, hipEventSynchronize(c->ev_d2h[par(k)]));
    std::string err;
    const int rc = dfx_hand_over(describe(k), &err);
    return rc == DFX_OK ? rc : dfx_fail(c, rc, err);
}

// Host mode, before batch k computes: flows of batch k-1 down (download stream, after its compute), frames of batch k+1
// up (upload stream, after the frame preparation of batch k-1, which last read that staging set).
int FlowRun::overlap_copies(size_t k) {
    int rc = k >= 1 ? download(k - 1) : DFX_OK;
    if (rc != DFX_OK)
        return rc;
    // Host work that can run beside this thread driving batch k (the TVL1 engine polls the device inside
    // run_pairs), on a helper thread: hand the results of batch k-1 over (rows to the caller's buffers / JPEG
    // files assembled; its download was enqueued just above and is a fraction of a batch's compute time), and — for
    // small frames — gather the frames of batch k+1 into the page-locked bounce buffer and send them up: 2048
    // frames of 224 x 224 are 100 MB of host memcpy, 6 % of their batch's compute time when the GPU waits for it.
    const bool hand = (bounce || out.jpeg) && k >= 1;
    const bool up_next = k + 1 < plan.size();
    if (up_next && !bounce_in) { // large frames: a few asynchronous copies to enqueue, nothing to gather
        rc = upload(k + 1);
        if (rc != DFX_OK)
            return rc;
    }
    if (hand || (up_next && bounce_in)) {
        c->helper.start([this, k, hand, up_next] {
            (void)hipSetDevice(c->device);
            int r = hand ? hand_over(k - 1) : DFX_OK;
            if (r == DFX_OK && up_next && bounce_in)
                r = upload(k + 1);
            return r;
        });
    }
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_h2d[par(k)], 0));
    if (seq0 + k >= 2) // flow staging set par(k) must have been drained by the download of batch q-2
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_d2h[par(k)], 0));
    return DFX_OK;
}

int FlowRun::launch_jpeg(size_t k) { // imencode(".jpg") of both planes of every flow, on the device (src/common.cpp:56-57)
    const int rc = dfx_launch_jpeg(c, par(k), 2 * plan[k].nb, plan[k].nb, c->img_slots);
    if (rc == DFX_OK)
        c->stats.kernel_launches += 5;
    return rc;
}

// dfx_calc_batch_bidir_device: the batch's pairs once more with the two frames exchanged — the frames are resident, nothing
// is built again — into the caller's backward planes, then the forward-backward check of both directions in one launch.
// Two run_pairs calls of nb pairs each, each with the account() it is owed on an idle stream: the engine sees the two
// batches it would see from a planar call with `step` and one with -step, so the bits (and TVL1's early-exit grouping)
// are those calls'.  fwd: where the forward planes of this batch just went.
int FlowRun::backward(const DfxBatchPlan &p, const DfxPlanarOut &fwd) {
    HIPCHK(c, dfx_stream_wait(c, c->stream)); // the forward batch's statistics read-backs are complete
    int rc = E->account(p.nb);
    if (rc != DFX_OK)
        return rc;
    for (int j = 0; j < p.nb; ++j) {
        const int i = p.i0 + j;
        c->h_pairs[j].frame_a = dfx_pair_a(pairs, i, -step) % F;
        c->h_pairs[j].frame_b = dfx_pair_b(pairs, i, -step) % F;
    }
    DfxPlanarOut bwd = fwd;
    bwd.base = out.d_planar_bwd + (size_t)p.i0 * out.d_flow_stride;
    bwd.vec = dfx_planar_vec(bwd.base, bwd.flow_stride, bwd.plane_stride, bwd.row_pitch, 4);
    rc = E->run_pairs(p.nb, c->h_pairs.data(), nullptr, 0, &bwd, nullptr);
    if (rc != DFX_OK || !out.d_occ_fwd)
        return rc;
    FbCheckArgs a{};
    a.dir[0].f = a.dir[1].b = static_cast<const float *>(fwd.base);
    a.dir[0].b = a.dir[1].f = static_cast<const float *>(bwd.base);
    a.dir[0].occ = out.d_occ_fwd + (size_t)p.i0 * out.d_occ_stride;
    a.dir[1].occ = out.d_occ_bwd + (size_t)p.i0 * out.d_occ_stride;
    a.dirs = 2, a.n = p.nb, a.w = c->W, a.h = c->H;
    a.row_pitch = fwd.row_pitch, a.plane_stride = fwd.plane_stride, a.flow_stride = fwd.flow_stride;
    a.occ_pitch = (long long)out.occ_pitch, a.occ_stride = (long long)out.d_occ_stride;
    a.alpha1 = out.alpha1, a.alpha2 = out.alpha2;
    fb_check_launch(c->stream, a);
    HIPCHK(c, hipGetLastError());
    c->stats.kernel_launches += 1;
    return DFX_OK;
}

int FlowRun::compute(size_t k) { // batch k on the compute stream, up to its statistics and (JPEG) its coded sizes
    const DfxBatchPlan &p = plan[k];
    const int q = par(k);
    int rc;
    HIPCHK(c, hipEventRecord(c->ev_t0, c->stream));
    for (int j = 0; j < p.n_new; ++j)
        c->h_slots[j] = (int)((p.first_new + j) % F);
    if (p.n_new > 0) {
        // the new frames: in staging set q (host mode: uploaded there) or in the caller's device array
        const unsigned char *src = host_mode ? (prep ? c->d_src[q] : c->d_u8[q])
                                             : in.d_frames + (size_t)p.first_new * in.d_frame_stride;
        long long pitch = host_mode ? (long long)c->in_row_bytes() : (long long)in.d_pitch;
        long long stride = !host_mode ? (long long)in.d_frame_stride : prep ? (long long)src_stride : (long long)plane;
        if (prep && clip_fmt.empty()) { // cvtColor + cv::resize of load_frames_batch (src/denseflow_gpu.cpp:163, :169), on the device
            prepare_launch(c->stream, src, pitch, stride, c->src_w, c->src_h, c->src_ch, p.n_new, c->d_u8[q], c->W,
                           (long long)plane, c->W, c->H, c->src_rgb, c->src_planar,
                           host_mode ? 0 : (long long)c->src_plane_stride); // (staged planes are dense)
            HIPCHK(c, hipGetLastError());
            c->stats.kernel_launches += 1;
            src = c->d_u8[q], pitch = c->W, stride = (long long)plane;
        } else if (prep) { // the same, one launch per run of frames of one source size (at most one per clip)
            std::vector<int> fw, fh;
            for (const auto &f : clip_fmt)
                fw.push_back(f.w), fh.push_back(f.h);
            for (const DfxFormatRun &r : dfx_format_runs(fw, fh, clip_of, p.first_new, p.n_new)) { // dfx_plan.h, CPU-tested
                const auto &f = clip_fmt[(size_t)r.clip];
                prepare_launch(c->stream, src + (size_t)r.j0 * src_stride, (long long)f.w * src_ch, stride, f.w, f.h, src_ch,
                               r.n, c->d_u8[q] + (size_t)r.j0 * plane, c->W, (long long)plane, c->W, c->H);
                HIPCHK(c, hipGetLastError());
                c->stats.kernel_launches += 1;
            }
            src = c->d_u8[q], pitch = c->W, stride = (long long)plane;
        }
        rc = E->build_frames(src, stride, pitch, p.n_new, c->h_slots.data());
        if (rc != DFX_OK)
            return rc;
    }
    // pair i of a clip: a = (step>0 ? i : i-step), b = (step>0 ? i+step : i)   (src/denseflow_gpu.cpp:315-316)
    for (int j = 0; j < p.nb; ++j) {
        const int i = p.i0 + j;
        c->h_pairs[j].frame_a = dfx_pair_a(pairs, i, step) % F;
        c->h_pairs[j].frame_b = dfx_pair_b(pairs, i, step) % F;
    }
    DfxSeedIn seed{}; // the batch's initial flows: pair j of the batch is pair j of the descriptor
    if (in.init) {
        seed.u = c->d_seed[q], seed.step = 2, seed.row_pitch = (long long)c->W * 2, seed.pair_stride = (long long)plane * 2;
    } else if (in.d_init && in.init_planar) {
        seed.u = in.d_init + (size_t)p.i0 * in.d_init_stride, seed.step = 1;
        seed.row_pitch = (long long)in.d_init_row_pitch, seed.pair_stride = (long long)in.d_init_stride;
    } else if (in.d_init) {
        seed.u = in.d_init + (size_t)p.i0 * in.d_init_stride, seed.step = 2;
        seed.row_pitch = (long long)c->W * 2, seed.pair_stride = (long long)in.d_init_stride;
    }
    seed.v = seed.u ? seed.u + (seed.step == 2 ? 1 : (long long)in.d_init_plane_stride) : nullptr;
    const DfxSeedIn *seedp = in.seeded() ? &seed : nullptr;
    const bool staged = host_mode || out.quantized;
    float *dst = staged ? c->d_flow_out[q] : out.planar ? nullptr : out.d_flows + (size_t)p.i0 * out.d_flow_stride;
    const long long dst_stride = staged ? (long long)plane * 2 : (long long)out.d_flow_stride;
    if (out.planar) { // the engine's last kernel writes the planes: the caller's (device mode) or dense ones in staging set q
        DfxPlanarOut po;
        po.elem = out.elem;
        po.base = staged ? (void *)dst
                         : (void *)(static_cast<unsigned char *>(out.d_planar) + (size_t)p.i0 * out.d_flow_stride * out_elem_bytes());
        po.flow_stride = dst_stride;
        po.plane_stride = staged ? (long long)plane : (long long)out.d_plane_stride;
        po.row_pitch = staged ? (long long)c->W : (long long)out.d_row_pitch;
        po.bound = out.norm_bound;
        po.vec = dfx_planar_vec(po.base, po.flow_stride, po.plane_stride, po.row_pitch, (int)out_elem_bytes());
        rc = E->run_pairs(p.nb, c->h_pairs.data(), nullptr, 0, &po, seedp);
        if (rc == DFX_OK && out.bidir)
            rc = backward(p, po);
    } else {
        rc = E->run_pairs(p.nb, c->h_pairs.data(), dst, dst_stride, nullptr, seedp);
    }
    if (rc != DFX_OK)
        return rc;
    if (out.quantized) {
        // the bounded planes of this batch: staging set q (host mode), or the caller's device arrays from pair i0 on
        unsigned char *x = host_mode ? c->d_img[q] : out.d_img_x + (size_t)p.i0 * out.d_img_stride;
        unsigned char *y = host_mode ? c->d_img[q] + (size_t)c->img_slots * plane : out.d_img_y + (size_t)p.i0 * out.d_img_stride;
        const long long pitch = host_mode ? c->W : (long long)out.img_pitch;
        const long long stride = host_mode ? (long long)plane : (long long)out.d_img_stride;
        if (out.png) { // convertFlowToPngImage's bounds and planes on the device (src/common.cpp:18-46)
            double *bounds = host_mode ? c->d_png_bounds[q] : out.d_bounds + 2 * (size_t)p.i0;
            quant_launch_flow_to_png_planes(c->stream, dst, dst_stride, p.nb, c->W, c->H, c->d_png_scratch, bounds, x, y,
                                            pitch, stride);
        } else { // convertFlowToImage on the device (src/common.cpp:4-16)
            quant_launch_flow_to_u8(c->stream, dst, dst_stride, p.nb, c->W, c->H, out.lo, out.hi, x, y, pitch, stride);
        }
        HIPCHK(c, hipGetLastError());
        c->stats.kernel_launches += out.png ? 4 : 1;
    }
    if (out.jpeg) {
        rc = launch_jpeg(k);
        if (rc != DFX_OK)
            return rc;
    }
    HIPCHK(c, hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_compute[q], c->stream));
    HIPCHK(c, dfx_stream_wait(c, c->stream)); // the engines' statistics read-backs are complete
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    c->stats.device_ms += ms;
    rc = E->account(p.nb);
    if (rc != DFX_OK)
        return rc;
    rc = c->helper.finish(); // batch k-1 is in the caller's buffers
    if (rc != DFX_OK)
        return rc;
    if (out.png && host_mode) // the stream is idle: this batch's bounds are in the mapped block
        std::memcpy(out.bounds + 2 * (size_t)p.i0, c->h_png_bounds[q], (size_t)p.nb * 2 * sizeof(double));
    if (out.jpeg) // a batch that is coded again is coded from its bounded planes in staging set q: no flow is recomputed
        rc = dfx_jpeg_settle(c, c->jpeg, q, 2 * p.nb, /*idle=*/true, "JPEG",
                             "JPEG: the batch's streams do not fit the stream buffer (use the 8-bit plane output and encode on "
                             "the host)",
                             [&]() -> int {
                                 const int lrc = launch_jpeg(k);
                                 if (lrc == DFX_OK)
                                     HIPCHK(c, hipEventRecord(c->ev_compute[q], c->stream));
                                 return lrc;
                             },
                             &coded[k]);
    return rc;
}

// The last batch's download, and its hand-over: now, or (ticket) on a deferred tail, so that the caller can issue the
// next FlowBuffer while it runs (its uploads run on the other copy stream).
int FlowRun::finish(uint64_t *ticket) {
    const size_t last = plan.size() - 1;
    const int rc = download(last);
    if (rc != DFX_OK)
        return rc;
    if (ticket) {
        DfxHandover h = describe(last);
        if (!dfx_may_not_fit(h)) {
            *ticket = dfx_defer_tail(c, par(last), c->ev_d2h[par(last)],
                                     [h = std::move(h)](std::string *err) { return dfx_hand_over(h, err); });
            return DFX_OK;
        }
    }
    HIPCHK(c, dfx_stream_wait(c, c->d2h_stream));
    return (bounce || out.jpeg) ? hand_over(last) : DFX_OK;
}

int FlowRun::run(uint64_t *ticket) {
    int rc = host_mode ? upload(0) : DFX_OK;
    for (size_t k = 0; rc == DFX_OK && k < plan.size(); ++k) {
        if (host_mode)
            rc = overlap_copies(k);
        if (rc == DFX_OK)
            rc = compute(k);
    }
    if (rc == DFX_OK && host_mode)
        rc = finish(ticket);
    return rc;
}

int flowbuffer_body(dfx_context *c, const InSpec &in, int n_frames, int step, const OutSpec &out, uint64_t *ticket) {
    // dfx_next_segments applies to this call only, whatever becomes of it
    std::vector<int> seg;
    seg.swap(c->next_segments);
    std::vector<dfx_context::SegFormat> seg_fmt;
    seg_fmt.swap(c->next_seg_fmt);
    const int seg_ch = c->next_seg_ch;
    c->next_seg_ch = 1;
    if (ticket)
        *ticket = 0;
    else
        (void)dfx_finish_tails(c, 0, -1); // synchronous entry points never run beside a deferred tail
    if (n_frames < 0 || step == 0 || step < -(1 << 30) || step > (1 << 30)) // (|INT_MIN| is not an int)
        return dfx_fail(c, DFX_ERR_INVALID, "n_frames must be >= 0 and step non-zero");
    // The FlowBuffer's pairs as (frame a, frame b), frame ids counted over the whole buffer.  One clip: pair i is
    // (i, i + step) for step > 0, (i - step, i) otherwise, M = max(N - |step|, 0) of them (src/denseflow_gpu.cpp:307-316).
    // Several clips joined (dfx_next_segments): the same rule inside every clip, no pair across a clip boundary.
    if (seg.empty())
        seg.push_back(n_frames);
    long long total = 0;
    for (int n : seg) {
        if (n < 0)
            return dfx_fail(c, DFX_ERR_INVALID, "dfx_next_segments: negative clip length");
        total += n;
    }
    if (total != n_frames)
        return dfx_fail(c, DFX_ERR_INVALID, "dfx_next_segments: the clip lengths do not add up to n_frames");
    if (!seg_fmt.empty() && !in.frames)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "dfx_next_segments_src applies to host-pointer calls only");
    if (in.frames && seg_fmt.empty() && c->prepares() && c->src_planar && c->src_plane_stride != 0)
        return dfx_fail(c, DFX_ERR_INVALID,
                        "a non-zero plane_stride applies to the device-resident forms only: host frames hold dense planes");
    FlowRun run(c, in, out, step);
    run.clip_fmt.swap(seg_fmt); // one per clip (dfx_next_segments_src), or none
    run.seg_ch = seg_ch;
    const int rc = run.prepare(seg);
    return rc == DFX_OK && !run.plan.empty() ? run.run(ticket) : rc;
}

} // namespace

int dfx_run_flowbuffer(dfx_context *c, const InSpec &in, int n_frames, int step, const OutSpec &out, uint64_t *ticket) {
    if (c->algo == DFX_ALGO_FRAMES) // every flow entry point funnels through here
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "a DFX_ALGO_FRAMES handle computes no flow");
    const int rc = flowbuffer_body(c, in, n_frames, step, out, ticket);
    if (rc != DFX_OK)
        dfx_drain_after_error(c);
    return rc;
}

int dfx_ensure_img_staging(dfx_context *c, int need) {
    if (need <= c->img_slots)
        return DFX_OK;
    return dfx_regrow(c, c->img_slots, need, [&]() -> int {
        c->img_bytes = 0;
        const int rc = realloc_pair(c, c->d_img, (size_t)need * 2 * c->W * c->H);
        if (rc == DFX_OK)
            c->img_bytes = (size_t)need * 2 * c->W * c->H;
        return rc;
    });
}

// dfx_set_size: what the staging sets hold at the new W x H.  The source format is back at its default, and the gray
// JPEG encoder works its header and its slot count out again at its next use (dfx_ensure_jpeg).
void dfx_pipeline_resized(dfx_context *c) {
    const size_t plane = (size_t)c->W * c->H;
    c->u8_slots = dfx_slots_in(c->u8_bytes, plane);
    c->flow_slots = dfx_slots_in(c->flow_bytes, plane * 2 * sizeof(float));
    c->img_slots = dfx_slots_in(c->img_bytes, 2 * plane);
    c->src_frame_bytes = 0;
    c->src_slots = 0;
    c->jpeg.slots = 0;
    c->jpeg.hdr_w = c->jpeg.hdr_h = 0;
}

int dfx_ensure_png(dfx_context *c, int need) {
    if (need <= c->png_slots)
        return DFX_OK;
    return dfx_regrow(c, c->png_slots, need, [&]() -> int {
        dfx_free_dev(c->d_png_scratch);
        HIPCHK(c, hipMalloc(&c->d_png_scratch, quant_png_scratch_bytes(need)));
        for (int p = 0; p < 2; ++p) {
            dfx_free_host(c->h_png_bounds[p]);
            HIPCHK(c, hipHostMalloc((void **)&c->h_png_bounds[p], (size_t)need * 2 * sizeof(double), hipHostMallocMapped));
            HIPCHK(c, hipHostGetDevicePointer((void **)&c->d_png_bounds[p], c->h_png_bounds[p], 0));
        }
        return DFX_OK;
    });
}

// The shared stream buffer holds 4 bits per pixel on average over the batch (flow planes need ~0.5; a batch that does
// not fit is measured, and coded again after dfx_jpeg_grow).
int dfx_ensure_jpeg(dfx_context *c, int pairs, int quality) {
    auto &j = c->jpeg;
    if (j.quality == quality && j.hdr_w == c->W && j.hdr_h == c->H && pairs <= j.slots)
        return DFX_OK;
    // Every buffer is kept by what it holds and only grows: another frame size (dfx_set_size) or quality re-uses what is
    // large enough.  A handle that sees one size and one quality allocates what it always did.
    return dfx_regrow(c, j.slots, pairs, [&]() -> int {
        const size_t planes = 2 * (size_t)pairs, nblk = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
        JpegTables t;
        unsigned char q[64];
        jpeg_build_tables(quality, t, q);
        j.header = jpeg_file_header(c->W, c->H, q);
        j.hdr_w = j.hdr_h = 0;
        j.quality = 0;
        if (!j.d_tab)
            HIPCHK(c, hipMalloc(&j.d_tab, sizeof(JpegTables)));
        HIPCHK(c, hipMemcpy(j.d_tab, &t, sizeof t, hipMemcpyHostToDevice));
        if (planes * nblk > j.blocks_cap) {
            j.blocks_cap = 0;
            dfx_free_dev(j.d_dc);
            dfx_free_dev(j.d_bits);
            HIPCHK(c, hipMalloc(&j.d_dc, planes * nblk * sizeof(short)));
            HIPCHK(c, hipMalloc(&j.d_bits, planes * nblk * sizeof(unsigned)));
            j.blocks_cap = planes * nblk;
        }
        if (!j.d_hdr)
            HIPCHK(c, hipMalloc(&j.d_hdr, 16));
        if (planes > j.planes_cap) {
            j.planes_cap = 0;
            dfx_free_dev(j.d_plane_bits);
            dfx_free_dev(j.d_plane_base);
            HIPCHK(c, hipMalloc(&j.d_plane_bits, planes * 8));
            HIPCHK(c, hipMalloc(&j.d_plane_base, planes * 8));
            for (int p = 0; p < 2; ++p) {
                dfx_free_host(j.h_info[p]);
                j.d_info[p] = nullptr;
                HIPCHK(c, hipHostMalloc(&j.h_info[p], (2 + 2 * planes) * 8, hipHostMallocMapped));
                HIPCHK(c, hipHostGetDevicePointer((void **)&j.d_info[p], j.h_info[p], 0));
            }
            j.planes_cap = planes;
        }
        for (int p = 0; p < 2; ++p)
            std::memset(j.h_info[p], 0, (2 + 2 * j.planes_cap) * 8);
        const size_t cap = ((planes * (size_t)c->W * c->H / 2 + (64u << 10)) + 255) & ~(size_t)255;
        if (cap > j.capacity) {
            j.capacity = 0;
            for (int p = 0; p < 2; ++p) {
                dfx_free_dev(j.d_stream[p]);
                HIPCHK(c, hipMalloc(&j.d_stream[p], cap));
            }
            j.capacity = cap;
        }
        for (int p = 0; p < 2; ++p) {
            // The page-locked landing buffer starts at 1 bit per pixel (flow planes code to ~0.3-0.5) and grows to what a batch
            // really needs (dfx_jpeg_ensure_landing): pinning 4 bits per pixel twice was ~0.1 s of a 1080p handle's first call
            // (profiles/round5/e2e/) for bytes that never arrive.
            const size_t hcap = (cap / 4 + 255) & ~(size_t)255;
            if (hcap > j.h_capacity[p]) {
                j.h_capacity[p] = 0;
                dfx_free_host(j.h_stream[p]);
                HIPCHK(c, hipHostMalloc(&j.h_stream[p], hcap, hipHostMallocDefault));
                j.h_capacity[p] = hcap;
            }
        }
        j.quality = quality;
        j.hdr_w = c->W, j.hdr_h = c->H;
        return DFX_OK;
    });
}

int dfx_launch_jpeg(dfx_context *c, int q, int n_planes, int n_x, int y_first) {
    const auto &j = c->jpeg;
    if (n_planes > DFX_GRID_YZ_MAX) // they lie in grid.y
        return dfx_fail(c, DFX_ERR_INVALID, "JPEG: more than 65535 planes in one batch");
    JpegCtx jc;
    jc.planes = c->d_img[q];
    jc.plane_stride = (long long)c->W * c->H;
    jc.pitch = c->W, jc.w = c->W, jc.h = c->H, jc.bw = (c->W + 7) / 8, jc.bh = (c->H + 7) / 8;
    jc.n_planes = n_planes, jc.n_x = n_x, jc.y_first = y_first;
    jc.tab = j.d_tab, jc.dc = j.d_dc, jc.bits = j.d_bits;
    jc.plane_bits = j.d_plane_bits, jc.plane_base = j.d_plane_base;
    jc.stream = j.d_stream[q], jc.capacity_bytes = j.capacity;
    jc.info = j.d_info[q], jc.hdr = j.d_hdr;
    jpeg_launch_encode(c->stream, jc);
    HIPCHK(c, hipGetLastError());
    return DFX_OK;
}
