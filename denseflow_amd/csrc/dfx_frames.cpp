// dfx_frames.cpp — colour frame extraction behind the C ABI (include/dfx.h): DFX_ALGO_FRAMES handles, the 3-channel
// resize, the colour JPEG encoder and dfx_extract_frames, which chains them for one buffer of frames.
//
// Reference behaviour replaced: DenseFlow::extract_frames_only, /root/reference/src/denseflow_gpu.cpp:82-105 —
// load_frames_batch(..., to_gray = false) :88, cv::resize of the BGR frame :94-98, imencode(".jpg", frame) :99-101.
#include <algorithm>
#include <cstring>

#include "dfx_internal.h"
#include "jpeg_kernels.h"
#include "prepare_kernels.h"

namespace {

// A DFX_ALGO_FRAMES handle has no flow engine behind it: this one allocates nothing and refuses every flow request
// (the ABI's flow entry points stop earlier, in dfx_run_flowbuffer).
class FramesEngine : public AlgoEngine {
  public:
    explicit FramesEngine(dfx_context *c) : c_(c) {}
    int create() override { return DFX_OK; }
    int set_size(int, int) override { return DFX_OK; } // the colour state follows at its next use (ensure_colour)
    size_t device_bytes() const override { return 0; }  // that state is counted on its own (dfx_frames_device_bytes)
    int batch() const override;
    int ensure_frame_slots(int) override { return refuse(); }
    int frame_slots() const override { return 0; }
    int build_frames(const unsigned char *, long long, long long, int, const int *) override { return refuse(); }
    int run_pairs(int, const PairDesc *, float *, long long, const DfxPlanarOut *, const DfxSeedIn *) override { return refuse(); }
    int account(int) override { return refuse(); }

  private:
    int refuse() const { return dfx_fail(c_, DFX_ERR_UNSUPPORTED, "a DFX_ALGO_FRAMES handle computes no flow"); }
    dfx_context *c_;
};

int frames_batch(const dfx_context *c) { return frames_plan_batch(c->W, c->H, c->prm.max_batch); } // engine_plan.h

int FramesEngine::batch() const { return frames_batch(c_); }

size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

// p holds `need` bytes of device memory (cap: what it holds now); the colour state's byte count follows
template <class T> int dev_grow(dfx_context *c, T *&p, size_t &cap, size_t need) {
    if (need <= cap)
        return DFX_OK;
    dfx_free_dev(p);
    c->colour.device_bytes -= cap;
    cap = 0;
    HIPCHK(c, hipMalloc((void **)&p, need));
    cap = need;
    c->colour.device_bytes += need;
    return DFX_OK;
}

void free_staging(dfx_context *c) {
    auto &j = c->colour;
    for (auto &p : j.d_src)
        dfx_free_dev(p);
    dfx_free_dev(j.d_bgr);
    j.src_slots = j.bgr_slots = 0;
    j.src_pitch = j.src_frame_bytes = 0;
    j.src_cap[0] = j.src_cap[1] = j.bgr_cap = 0;
    j.tab_cap = j.dc_cap = j.bits_cap = j.pbits_cap = j.pbase_cap = j.hdr_cap = j.stream_cap[0] = j.stream_cap[1] = 0;
    j.info_slots = 0;
}

// Everything of the colour state, for batches of `frames` frames at `quality` from sw x sh sources into the handle's
// W x H.  Every buffer is kept by what it holds and only grows: another source size, output size (dfx_set_size) or
// quality re-uses what is large enough, and a handle that sees one of each allocates what it always did.
int ensure_colour(dfx_context *c, int frames, int quality, int sw, int sh) {
    auto &j = c->colour;
    const bool resize = sw != c->W || sh != c->H;
    const size_t sp = round4((size_t)sw * 3), fb = sp * (size_t)sh;
    if (j.quality == quality && j.hdr_w == c->W && j.hdr_h == c->H && frames <= j.slots && frames <= j.src_slots &&
        j.src_frame_bytes == fb && j.src_pitch == sp && (!resize || frames <= j.bgr_slots))
        return DFX_OK;
    return dfx_regrow(c, j.slots, frames, [&]() -> int {
        j.hdr_w = j.hdr_h = 0;
        j.quality = 0;
        j.src_slots = j.bgr_slots = 0;
        const size_t mcus = (size_t)((c->W + 15) / 16) * ((c->H + 15) / 16), nblk = mcus * 6;
        JpegTables t[2];
        jpeg_build_colour_tables(quality, t);
        j.header = jpeg_colour_file_header(c->W, c->H, quality);
        int rc = dev_grow(c, j.d_tab, j.tab_cap, sizeof t);
        if (rc != DFX_OK)
            return rc;
        HIPCHK(c, hipMemcpy(j.d_tab, t, sizeof t, hipMemcpyHostToDevice));
        if ((rc = dev_grow(c, j.d_dc, j.dc_cap, (size_t)frames * nblk * sizeof(short))) != DFX_OK ||
            (rc = dev_grow(c, j.d_bits, j.bits_cap, (size_t)frames * nblk * sizeof(unsigned))) != DFX_OK ||
            (rc = dev_grow(c, j.d_plane_bits, j.pbits_cap, (size_t)frames * 8)) != DFX_OK ||
            (rc = dev_grow(c, j.d_plane_base, j.pbase_cap, (size_t)frames * 8)) != DFX_OK ||
            (rc = dev_grow(c, j.d_hdr, j.hdr_cap, 16)) != DFX_OK)
            return rc;
        // shared stream buffer: 4 bits per pixel on average over the batch (a photographic frame at quality 95 needs 1.5 - 3;
        // a batch that does not fit is measured and coded again after dfx_jpeg_grow)
        const size_t cap = (((size_t)frames * c->W * c->H / 2 + (64u << 10)) + 255) & ~(size_t)255;
        for (int p = 0; p < 2; ++p) {
            j.stream_cap[p] = std::max(j.stream_cap[p], j.d_stream[p] ? j.capacity : (size_t)0); // dfx_jpeg_grow may have grown it
            if ((rc = dev_grow(c, j.d_stream[p], j.stream_cap[p], cap)) != DFX_OK)
                return rc;
            if (cap > j.h_capacity[p]) {
                j.h_capacity[p] = 0;
                dfx_free_host(j.h_stream[p]);
                HIPCHK(c, hipHostMalloc((void **)&j.h_stream[p], cap, hipHostMallocDefault));
                j.h_capacity[p] = cap;
            }
        }
        j.capacity = std::min(j.stream_cap[0], j.stream_cap[1]);
        if (frames > j.info_slots) {
            j.info_slots = 0;
            for (int p = 0; p < 2; ++p) {
                dfx_free_host(j.h_info[p]);
                j.d_info[p] = nullptr;
                HIPCHK(c, hipHostMalloc((void **)&j.h_info[p], (2 + 2 * (size_t)frames) * 8, hipHostMallocMapped));
                HIPCHK(c, hipHostGetDevicePointer((void **)&j.d_info[p], j.h_info[p], 0));
            }
            j.info_slots = frames;
        }
        for (int p = 0; p < 2; ++p) {
            std::memset(j.h_info[p], 0, (2 + 2 * (size_t)j.info_slots) * 8);
            if ((rc = dev_grow(c, j.d_src[p], j.src_cap[p], (size_t)frames * fb)) != DFX_OK)
                return rc;
        }
        const size_t out_frame = round4((size_t)c->W * 3) * c->H;
        if (resize && (rc = dev_grow(c, j.d_bgr, j.bgr_cap, (size_t)frames * out_frame)) != DFX_OK)
            return rc;
        j.quality = quality;
        j.hdr_w = c->W, j.hdr_h = c->H;
        j.src_slots = frames;
        j.bgr_slots = resize ? frames : 0;
        j.src_pitch = sp;
        j.src_frame_bytes = fb;
        return DFX_OK;
    });
}

// n source-size BGR frames -> n files, in device batches.  Per batch q (parity p = seq & 1):
//   copy stream : frames -> d_src[p]                                        (batch q + 1 goes up while q computes)
//   compute     : [resize d_src[p] -> d_bgr] -> encode -> d_stream[p]; the totals land in h_info[p]
//   d2h stream  : d_stream[p] -> h_stream[p]
//   host        : header + stuffing of batch q - 1 while batch q computes
// ticket != nullptr: the last batch's download and assembly finish on a helper thread (dfx_context::Tail).
int extract_body(dfx_context *c, const uint8_t *const *frames, size_t pitch, int sw, int sh, int n, int quality,
                 uint8_t *const *jpg, size_t cap, uint32_t *sizes, uint64_t *ticket) {
    auto &j = c->colour;
    const int B = std::min({frames_batch(c), std::max(n, 1), DFX_GRID_YZ_MAX}); // a batch's frames lie in grid.z
    int rc = ensure_colour(c, std::max(B, j.slots), quality, sw, sh);
    if (rc != DFX_OK)
        return rc;
    const bool resize = sw != c->W || sh != c->H;
    const size_t row = (size_t)sw * 3, out_pitch = round4((size_t)c->W * 3), out_frame = out_pitch * c->H;
    const int nb = (n + B - 1) / B;
    auto upload = [&](int q, int p) -> int {
        // d_src[p] was last read by the compute of batch q - 2, which this thread has waited for; a tail only reads
        // the landing buffer
        const int i0 = q * B, m = std::min(B, n - i0);
        for (int i = 0; i < m; ++i)
            HIPCHK(c, hipMemcpy2DAsync(j.d_src[p] + (size_t)i * j.src_frame_bytes, j.src_pitch, frames[i0 + i], pitch, row,
                                       (size_t)sh, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->ev_h2d[p], c->copy_stream));
        return DFX_OK;
    };
    auto encode = [&](int m, int p) -> int {
        JpegColourCtx jc;
        jc.bgr = resize ? j.d_bgr : j.d_src[p];
        jc.frame_stride = (long long)(resize ? out_frame : j.src_frame_bytes);
        jc.pitch = (int)(resize ? out_pitch : j.src_pitch);
        jc.w = c->W, jc.h = c->H, jc.mcus_x = (c->W + 15) / 16, jc.mcus_y = (c->H + 15) / 16;
        jc.n_planes = m;
        jc.tab = j.d_tab, jc.dc = j.d_dc, jc.bits = j.d_bits;
        jc.plane_bits = j.d_plane_bits, jc.plane_base = j.d_plane_base;
        jc.stream = j.d_stream[p], jc.capacity_bytes = j.capacity;
        jc.info = j.d_info[p], jc.hdr = j.d_hdr;
        jpeg_colour_launch_encode(c->stream, jc);
        HIPCHK(c, hipGetLastError());
        return DFX_OK;
    };
    // the files of batch [i0, i0 + coded.planes.size()) out of the landing buffer of parity p
    auto files_of = [&](int i0, int p, const DfxJpegCoded &coded) {
        DfxHandover h;
        h.header = j.header, h.landing = j.h_stream[p], h.coded = coded.planes;
        h.capacity = cap;
        h.too_small = "JPEG: jpg_capacity is too small for an encoded frame";
        for (size_t i = 0; i < coded.planes.size(); ++i) {
            h.jpg.push_back(jpg[i0 + i]);
            h.size.push_back(sizes + i0 + i);
        }
        return h;
    };
    DfxHandover prev; // the batch whose download is in flight
    bool have_prev = false;
    int prev_parity = 0;
    std::string err;
    const unsigned long long seq0 = j.seq;
    rc = upload(0, (int)(seq0 & 1));
    if (rc != DFX_OK)
        return rc;
    for (int q = 0; q < nb; ++q) {
        const int p = (int)((seq0 + q) & 1), i0 = q * B, m = std::min(B, n - i0);
        j.seq = seq0 + q + 1;
        // the landing buffer and the totals of this parity may still be in use by a deferred tail of an earlier call
        (void)dfx_finish_tails(c, 0, p);
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_h2d[p], 0));
        if (resize) {
            prepare_bgr_launch(c->stream, j.d_src[p], (long long)j.src_pitch, (long long)j.src_frame_bytes, sw, sh, m, j.d_bgr,
                               (long long)out_pitch, (long long)out_frame, c->W, c->H);
            HIPCHK(c, hipGetLastError());
        }
        if ((rc = encode(m, p)) != DFX_OK)
            return rc;
        if (q + 1 < nb && (rc = upload(q + 1, p ^ 1)) != DFX_OK)
            return rc;
        if (have_prev) { // host work of batch q - 1 beside the kernels of batch q
            HIPCHK(c, dfx_stream_wait(c, c->d2h_stream));
            if ((rc = dfx_hand_over(prev, &err)) != DFX_OK)
                return dfx_fail(c, rc, err);
            have_prev = false;
        }
        DfxJpegCoded coded;
        size_t grown = 0;
        rc = dfx_jpeg_settle(c, j, p, m, /*idle=*/false, "colour JPEG",
                             "JPEG: the frames do not fit the stream buffer (encode them on the host)",
                             [&] { return encode(m, p); }, &coded, &grown);
        j.device_bytes += grown;
        if (rc != DFX_OK)
            return rc;
        HIPCHK(c, hipMemcpyAsync(j.h_stream[p], j.d_stream[p], (size_t)coded.total, hipMemcpyDeviceToHost, c->d2h_stream));
        HIPCHK(c, hipEventRecord(c->ev_d2h[p], c->d2h_stream));
        prev = files_of(i0, p, coded);
        prev_parity = p;
        have_prev = true;
    }
    c->stats.kernel_launches += (uint64_t)nb * (resize ? 6 : 5);
    if (!have_prev)
        return DFX_OK;
    if (ticket && !dfx_may_not_fit(prev)) {
        *ticket = dfx_defer_tail(c, prev_parity, c->ev_d2h[prev_parity],
                                 [h = std::move(prev)](std::string *e) { return dfx_hand_over(h, e); });
        return DFX_OK;
    }
    HIPCHK(c, dfx_stream_wait(c, c->d2h_stream));
    rc = dfx_hand_over(prev, &err);
    return rc == DFX_OK ? rc : dfx_fail(c, rc, err);
}

int extract_entry(dfx_handle h, const uint8_t *const *frames, size_t pitch, int sw, int sh, int n, int quality,
                  uint8_t *const *jpg, size_t cap, uint32_t *sizes, uint64_t *ticket) {
    if (!h)
        return DFX_ERR_INVALID;
    if (ticket)
        *ticket = 0;
    else
        (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!frames || !jpg || !sizes)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frame, JPEG buffer or size array");
    if (sw < 1 || sh < 1 || sw > 32768 || sh > 32768)
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source frame size");
    if (pitch < (size_t)sw * 3)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    if (quality < 1 || quality > 100)
        return dfx_fail(h, DFX_ERR_INVALID, "JPEG quality must be 1..100");
    HIPCHK(h, hipSetDevice(h->device));
    const int rc = extract_body(h, frames, pitch, sw, sh, n, quality, jpg, cap, sizes, ticket);
    if (rc != DFX_OK) { // copies into caller-owned buffers may be in flight
        dfx_drain_after_error(h);
        if (ticket)
            *ticket = 0;
    }
    return rc;
}

} // namespace

AlgoEngine *dfx_make_frames_engine(dfx_context *c) { return new FramesEngine(c); }

void dfx_colour_resized(dfx_context *c) { c->colour.slots = 0; } // ensure_colour works everything out again, in place

void dfx_free_colour(dfx_context *c) {
    dfx_jpeg_free(c->colour);
    free_staging(c);
    c->colour.device_bytes = 0;
}

extern "C" {

int dfx_encode_jpeg_bgr(dfx_handle h, const uint8_t *const *frames, size_t pitch, int n, int quality, uint8_t *const *jpg,
                        size_t jpg_capacity, uint32_t *sizes) {
    if (!h)
        return DFX_ERR_INVALID;
    return extract_entry(h, frames, pitch, h->W, h->H, n, quality, jpg, jpg_capacity, sizes, nullptr);
}

int dfx_extract_frames(dfx_handle h, const uint8_t *const *frames, size_t pitch, int src_width, int src_height, int n,
                       int quality, uint8_t *const *jpg, size_t jpg_capacity, uint32_t *sizes) {
    return extract_entry(h, frames, pitch, src_width, src_height, n, quality, jpg, jpg_capacity, sizes, nullptr);
}

int dfx_submit_extract_frames(dfx_handle h, const uint8_t *const *frames, size_t pitch, int src_width, int src_height,
                              int n, int quality, uint8_t *const *jpg, size_t jpg_capacity, uint32_t *sizes,
                              uint64_t *ticket) {
    if (!ticket)
        return h ? dfx_fail(h, DFX_ERR_INVALID, "ticket is NULL") : DFX_ERR_INVALID;
    return extract_entry(h, frames, pitch, src_width, src_height, n, quality, jpg, jpg_capacity, sizes, ticket);
}

size_t dfx_jpeg_capacity_bgr(dfx_handle h) {
    if (!h)
        return 0;
    return (size_t)h->W * h->H * 3 + 4096;
}

size_t dfx_frames_device_bytes(dfx_handle h) { return h ? h->colour.device_bytes : 0; }

int dfx_prepare_frames_bgr_device(dfx_handle h, const uint8_t *d_src, size_t src_pitch, size_t src_frame_stride,
                                  int src_width, int src_height, int n, uint8_t *d_dst, size_t dst_pitch,
                                  size_t dst_frame_stride) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!d_src || !d_dst)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL device frames");
    if (src_width < 1 || src_height < 1 || src_width > 32768 || src_height > 32768)
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source frame size");
    if (src_pitch < (size_t)src_width * 3 || src_frame_stride < src_pitch * (size_t)src_height ||
        dst_pitch < (size_t)h->W * 3 || dst_frame_stride < dst_pitch * (size_t)h->H)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch/stride smaller than a frame");
    HIPCHK(h, hipSetDevice(h->device));
    prepare_bgr_launch(h->stream, d_src, (long long)src_pitch, (long long)src_frame_stride, src_width, src_height, n, d_dst,
                       (long long)dst_pitch, (long long)dst_frame_stride, h->W, h->H);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return DFX_OK;
}

int dfx_prepare_frames_bgr(dfx_handle h, const uint8_t *const *src, size_t src_pitch, int src_width, int src_height, int n,
                           uint8_t *const *dst, size_t dst_pitch) {
    if (!h)
        return DFX_ERR_INVALID;
    (void)dfx_finish_tails(h, 0, -1);
    if (n < 0)
        return dfx_fail(h, DFX_ERR_INVALID, "n must be >= 0");
    if (n == 0)
        return DFX_OK;
    if (!src || !dst)
        return dfx_fail(h, DFX_ERR_INVALID, "NULL frame arrays");
    if (src_width < 1 || src_height < 1 || src_width > 32768 || src_height > 32768)
        return dfx_fail(h, DFX_ERR_INVALID, "invalid source frame size");
    const size_t rb = (size_t)src_width * 3, sp = round4(rb), fb = sp * src_height;
    const size_t ob = (size_t)h->W * 3, op = round4(ob), of = op * h->H;
    if (src_pitch < rb || dst_pitch < ob)
        return dfx_fail(h, DFX_ERR_INVALID, "pitch smaller than a row");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned char *d_in = nullptr, *d_out = nullptr;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, ((size_t)256 << 20) / std::max(fb, of)));
    auto run = [&]() -> int {
        HIPCHK(h, hipMalloc((void **)&d_in, (size_t)chunk * fb));
        HIPCHK(h, hipMalloc((void **)&d_out, (size_t)chunk * of));
        for (int i0 = 0; i0 < n; i0 += chunk) {
            const int m = std::min(chunk, n - i0);
            for (int i = 0; i < m; ++i)
                HIPCHK(h, hipMemcpy2DAsync(d_in + (size_t)i * fb, sp, src[i0 + i], src_pitch, rb, (size_t)src_height,
                                           hipMemcpyHostToDevice, h->stream));
            prepare_bgr_launch(h->stream, d_in, (long long)sp, (long long)fb, src_width, src_height, m, d_out, (long long)op,
                               (long long)of, h->W, h->H);
            HIPCHK(h, hipGetLastError());
            for (int i = 0; i < m; ++i)
                HIPCHK(h, hipMemcpy2DAsync(dst[i0 + i], dst_pitch, d_out + (size_t)i * of, op, ob, (size_t)h->H,
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

} // extern "C"
