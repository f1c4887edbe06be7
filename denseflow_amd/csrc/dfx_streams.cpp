// dfx_streams.cpp — what the device-to-caller pipelines (dfx_pipeline.cpp: FlowBuffers; dfx_frames.cpp: colour frames)
// share: the deferred tails of the submit calls, the drain after an error, and the stream state of a device JPEG encoder.
#include <algorithm>

#include "dfx_internal.h"

int dfx_finish_tails(dfx_context *c, unsigned long long up_to, int parity, bool report) {
    auto matches = [&](const dfx_context::Tail &t) {
        return (up_to == 0 || t.ticket <= up_to) && (parity < 0 || t.parity == parity);
    };
    std::vector<std::unique_ptr<dfx_context::Tail>> finished;
    int rc = DFX_OK;
    {
        std::unique_lock<std::mutex> lock(c->tails_mtx);
        // a tail is visible to every caller until its worker is done: nobody can mistake "being joined" for "finished"
        c->tails_cv.wait(lock, [&] {
            for (const auto &t : c->tails)
                if (matches(*t) && !t->done)
                    return false;
            return true;
        });
        for (auto it = c->tails.begin(); it != c->tails.end();) {
            if (matches(**it)) {
                if ((*it)->rc != DFX_OK)
                    c->tail_errors.push_back({(*it)->ticket, (*it)->rc, (*it)->err});
                finished.push_back(std::move(*it));
                it = c->tails.erase(it);
            } else {
                ++it;
            }
        }
        if (report) {
            for (auto it = c->tail_errors.begin(); it != c->tail_errors.end();) {
                if (up_to == 0 || it->ticket <= up_to) {
                    if (rc == DFX_OK) {
                        rc = it->rc;
                        c->set_err(it->err);
                    }
                    it = c->tail_errors.erase(it);
                } else {
                    ++it;
                }
            }
        }
    }
    for (auto &t : finished) // done was the worker's last action: these joins return at once
        if (t->worker.joinable())
            t->worker.join();
    return rc;
}

unsigned long long dfx_defer_tail(dfx_context *c, int parity, hipEvent_t event, std::function<int(std::string *)> work) {
    std::unique_ptr<dfx_context::Tail> t(new dfx_context::Tail());
    const unsigned long long ticket = t->ticket = c->next_ticket++;
    t->parity = parity;
    dfx_context::Tail *tp = t.get();
    const int dev = c->device;
    t->worker = std::thread([c, tp, dev, event, work]() {
        (void)hipSetDevice(dev);
        const hipError_t e = hipEventSynchronize(event);
        std::string err;
        int rc = DFX_ERR_HIP;
        if (e != hipSuccess)
            err = std::string("deferred download failed: ") + hipGetErrorString(e);
        else
            rc = work(&err);
        {   // last action: publish the result; the context outlives every tail (dfx_destroy drains them)
            std::lock_guard<std::mutex> lock(c->tails_mtx);
            tp->rc = rc;
            tp->err = err;
            tp->done = true;
        }
        c->tails_cv.notify_all();
    });
    std::lock_guard<std::mutex> lock(c->tails_mtx);
    c->tails.push_back(std::move(t));
    return ticket;
}

void dfx_drain_after_error(dfx_context *c) {
    const std::string keep = c->get_err();
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->d2h_stream);
    (void)dfx_finish_tails(c, 0, -1);
    c->set_err(keep);
}

void dfx_jpeg_free(JpegStreams &j) {
    dfx_free_dev(j.d_tab);
    dfx_free_dev(j.d_dc);
    dfx_free_dev(j.d_bits);
    dfx_free_dev(j.d_plane_bits);
    dfx_free_dev(j.d_plane_base);
    dfx_free_dev(j.d_hdr);
    for (int q = 0; q < 2; ++q) {
        dfx_free_dev(j.d_stream[q]);
        dfx_free_host(j.h_stream[q]);
        j.h_capacity[q] = 0;
        dfx_free_host(j.h_info[q]);
        j.d_info[q] = nullptr;
    }
    j.quality = j.slots = 0;
    j.hdr_w = j.hdr_h = 0;
    j.blocks_cap = j.planes_cap = 0;
    j.capacity = 0;
}

// Called when the scan pass of a batch has measured more than the 4 bits per pixel the stream buffers provide for (noise,
// film grain), so that the batch can be coded again from the planes that are still on the device — nothing is recomputed
// and the caller does not have to fall back to the host encoder.
int dfx_jpeg_grow(dfx_context *c, JpegStreams &j, unsigned long long need, const char *noun, size_t *delta) {
    (void)dfx_finish_tails(c, 0, -1); // a deferred tail may still be reading a landing buffer
    HIPCHK(c, hipDeviceSynchronize());
    const size_t cap = (((size_t)need + (size_t)need / 4 + (64u << 10)) + 255) & ~(size_t)255;
    // All four new buffers first, swapped in only when every allocation has succeeded: a failure part-way leaves the
    // encoder exactly as it was (old buffers, old capacity) and the call reports the error.
    unsigned *nd[2] = {nullptr, nullptr};
    unsigned char *nh[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int p = 0; p < 2 && e == hipSuccess; ++p) {
        e = hipMalloc((void **)&nd[p], cap);
        if (e == hipSuccess)
            e = hipHostMalloc((void **)&nh[p], cap, hipHostMallocDefault);
    }
    if (e != hipSuccess) {
        for (int p = 0; p < 2; ++p) {
            if (nd[p])
                (void)hipFree(nd[p]);
            if (nh[p])
                (void)hipHostFree(nh[p]);
        }
        (void)hipGetLastError();
        return dfx_fail(c, DFX_ERR_HIP,
                        std::string("growing the ") + noun + " stream buffers failed; the encoder keeps its old buffers");
    }
    for (int p = 0; p < 2; ++p) {
        dfx_free_dev(j.d_stream[p]);
        dfx_free_host(j.h_stream[p]);
        j.d_stream[p] = nd[p];
        j.h_stream[p] = nh[p];
        j.h_capacity[p] = cap;
    }
    if (delta)
        *delta = 2 * (cap - j.capacity);
    j.capacity = cap;
    return DFX_OK;
}

int dfx_jpeg_ensure_landing(dfx_context *c, JpegStreams &j, int q, size_t need) {
    if (need <= j.h_capacity[q])
        return DFX_OK;
    const size_t cap = std::min(j.capacity, ((need + need / 2) + 255) & ~(size_t)255);
    unsigned char *nh = nullptr;
    if (hipHostMalloc((void **)&nh, cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return dfx_fail(c, DFX_ERR_HIP, "growing the JPEG landing buffer failed");
    }
    dfx_free_host(j.h_stream[q]);
    j.h_stream[q] = nh;
    j.h_capacity[q] = cap;
    return DFX_OK;
}

int dfx_jpeg_settle(dfx_context *c, JpegStreams &j, int q, int n, bool idle, const char *noun, const char *no_fit,
                    const std::function<int()> &launch, DfxJpegCoded *out, size_t *delta) {
    if (!idle)
        HIPCHK(c, dfx_stream_wait(c, c->stream));
    const unsigned long long *hi = j.h_info[q]; // the stream is idle: the totals of this batch are in the mapped block
    if (hi[1] != 0) {
        // The batch's streams do not fit the shared buffer: nothing was written, but the scan pass has measured what they
        // need.  Grow the buffers to that and code the batch again — its input is still on the device.
        int rc = dfx_jpeg_grow(c, j, hi[0], noun, delta);
        if (rc == DFX_OK)
            rc = launch();
        if (rc != DFX_OK)
            return rc;
        HIPCHK(c, dfx_stream_wait(c, c->stream));
        if (hi[1] != 0)
            return dfx_fail(c, DFX_ERR_UNSUPPORTED, no_fit);
    }
    out->total = hi[0];
    out->planes.resize(n);
    for (int i = 0; i < n; ++i)
        out->planes[i] = {hi[2 + 2 * i], hi[2 + 2 * i + 1]};
    return DFX_OK;
}
