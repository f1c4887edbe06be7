// brox_engine.cpp — host control of the -a=brox path (replaces cv::cuda::BroxOpticalFlow::calc as called at
// /root/reference/src/denseflow_gpu.cpp:303, :332-334, including the 1/255 convertTo the reference does itself).
// The algorithm is the one defined in oracle/brox_oracle.h (reference parity unpinned).
// Fixed control flow: a pair is a straight sequence of launches, `batch` pairs share each launch
// (grid.z = pair); a frame's pyramid and its five derivative pyramids are built once and serve two pairs.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "brox_kernels.h"
#include "dfx_internal.h"

namespace {

using BLevel = DfxPlanLevel; // engine_plan.h

class BroxEngine final : public AlgoEngine {
  public:
    explicit BroxEngine(dfx_context *ctx) : c(ctx) {}
    ~BroxEngine() override { destroy(); }
    int create() override;
    int set_size(int W, int H) override;
    size_t device_bytes() const override;
    int batch() const override { return B; }
    int ensure_frame_slots(int need) override;
    int frame_slots() const override { return n_frame_slots; }
    int build_frames(const unsigned char *d_src, long long src_frame_stride, long long src_pitch, int n,
                     const int *h_slots) override;
    int run_pairs(int nb, const PairDesc *h_pairs, float *d_out, long long out_stride, const DfxPlanarOut *planar,
                  const DfxSeedIn *seed) override;
    int account(int nb) override;

  private:
    void destroy();
    int grow_frame_slots(int need, long long elems);
    DfxSlotBufs slot_bufs(long long elems) { // engine_buffers.h: what a frame slot of `elems` floats needs
        DfxSlotBufs s;
        s.add(d_frames, frames_cap, (size_t)elems * sizeof(float));
        return s;
    }
    int slots_held() { return dfx_frame_slots_held(slot_bufs(frame_elems), slots.cap); }
    BroxLevelCtx level_ctx(int l, int nb) const;
    dfx_context *c;
    DfxHipAlloc mem{c};
    // what the buffers hold, in bytes (they only grow: set_size re-plans the engine inside them)
    size_t frames_cap = 0, planes_cap = 0, sink_cap = 0;
    std::vector<BLevel> lv;
    long long pyr_elems = 0, frame_elems = 0;
    int n_frame_slots = 0;
    float *d_frames = nullptr;
    DfxTable<int> slots; // frame-slot ids of build_frames
    int B = 0;
    int n_cu = 0; // compute units of the device: the streaming SOR runs one persistent workgroup on each
    float *d_planes = nullptr;
    long long plane_stride = 0, slot_stride = 0;
    DfxTable<PairDesc> pairs; // descriptors of run_pairs
    float *d_sor_sink = nullptr; // BroxLevelCtx::sor_sink
    hipEvent_t ev[2] = {nullptr, nullptr};
    uint64_t batch_launches = 0;
};

void BroxEngine::destroy() {
    dfx_free_dev(d_frames);
    slots.release(mem);
    dfx_free_dev(d_planes);
    pairs.release(mem);
    dfx_free_dev(d_sor_sink);
    dfx_destroy_events(ev, 2);
}

int BroxEngine::create() {
    const dfx_params &p = c->prm;
    if (p.impl < 0 || p.impl > 1)
        return dfx_fail(c, DFX_ERR_INVALID, "brox: impl must be 0 (tuned) or 1 (simple)");
    if (!(p.brox_scale_factor > 0.f && p.brox_scale_factor < 1.f) || !(p.brox_alpha > 0.f) ||
        p.brox_inner_iterations < 0 || p.brox_outer_iterations < 1 || p.brox_solver_iterations < 0)
        return dfx_fail(c, DFX_ERR_INVALID, "invalid Brox parameters");
    {
        int dev = 0;
        HIPCHK(c, hipGetDevice(&dev));
        HIPCHK(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    }
    // The streaming SOR runs max(n_cu / 8, 1) * 8 persistent workgroups at the most (brox_kernels.hip), whatever the frame
    // size, and each of them owns 16 floats of the sink: sized once, for that many and no fewer than one per CU.
    const int wgs = std::max(std::max(n_cu / 8, 1) * 8, std::max(n_cu, 1));
    HIPCHK(c, hipMalloc(&d_sor_sink, sizeof(float) * 16 * (size_t)wgs));
    sink_cap = sizeof(float) * 16 * (size_t)wgs;
    HIPCHK(c, hipEventCreateWithFlags(&ev[0], dfx_event_flags(c, true)));
    HIPCHK(c, hipEventCreateWithFlags(&ev[1], dfx_event_flags(c, true)));
    return set_size(c->W, c->H);
}

size_t BroxEngine::device_bytes() const {
    return frames_cap + planes_cap + sink_cap + sizeof(int) * (size_t)slots.cap + sizeof(PairDesc) * (size_t)pairs.cap;
}

// Plan (engine_plan.h: host arithmetic) + ensure capacity.  Nothing of the engine changes before the last allocation has
// succeeded; the buffers a failed attempt has already grown stay grown.
int BroxEngine::set_size(int W, int H) {
    BroxPlan pl;
    brox_plan(pl, W, H, c->prm, BROX_FP_COUNT, BROX_PL_COUNT);
    const size_t slot_bytes = (size_t)pl.slot_stride * sizeof(float);
    int nB = 0;
    if (const int rc = dfx_fit_pair_slots(mem, pl.batch, pl.per_pair, slot_bytes, device_bytes(), d_planes, planes_cap, B, nB))
        return rc;
    if (!dfx_grow_tables(mem, nB, pairs))
        return dfx_fail(c, DFX_ERR_HIP, "brox: allocating the pair descriptors failed");
    const int rc = grow_frame_slots(nB + 1, pl.frame_elems);
    if (rc != DFX_OK) { // the engine goes on at its old size, on the frame slots the buffer still holds
        dfx_settle_frame_slots(n_frame_slots, rc, slots_held());
        return rc;
    }
    lv = pl.lv;
    pyr_elems = pl.pyr_elems;
    frame_elems = pl.frame_elems;
    plane_stride = pl.plane_stride;
    slot_stride = pl.slot_stride;
    B = nB;
    dfx_settle_frame_slots(n_frame_slots, DFX_OK, slots_held());
    batch_launches = 0;
    return DFX_OK;
}

int BroxEngine::grow_frame_slots(int need, long long elems) {
    if (const int rc = dfx_grow_slot_bufs(mem, slot_bufs(elems), need))
        return rc;
    if (!dfx_grow_tables(mem, need, slots))
        return dfx_fail(c, DFX_ERR_HIP, "brox: allocating the frame-slot tables failed");
    return DFX_OK;
}

int BroxEngine::ensure_frame_slots(int need) {
    if (need <= n_frame_slots)
        return DFX_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = grow_frame_slots(need, frame_elems);
    // not dfx_settle_frame_slots: after a failure this engine counts whatever the buffers hold, which is more than it
    // counted before if an earlier set_size failed behind a buffer it had already grown
    n_frame_slots = slots_held();
    return rc;
}

int BroxEngine::build_frames(const unsigned char *d_src, long long src_frame_stride, long long src_pitch, int n,
                             const int *h_slots) {
    if (n <= 0)
        return DFX_OK;
    int *const d_frame_slots = slots.dev;
    slots.stage(h_slots, n);
    HIPCHK(c, hipMemcpyAsync(d_frame_slots, slots.host, slots.bytes(n), hipMemcpyHostToDevice, c->stream));
    const float a255 = (float)(1.0 / 255.0); // the reference's convertTo(CV_32F, 1.0/255.0) (:332-333)
    brox_launch_u8_to_f32(c->stream, d_src, src_frame_stride, src_pitch, d_frame_slots, n, d_frames, frame_elems,
                          lv[0].w, lv[0].h, lv[0].pitch, a255);
    for (size_t l = 1; l < lv.size(); ++l)
        brox_launch_downsample(c->stream, d_frames, frame_elems, d_frame_slots, n, lv[l - 1].off, lv[l - 1].w,
                               lv[l - 1].h, lv[l - 1].pitch, lv[l].off, lv[l].w, lv[l].h, lv[l].pitch,
                               c->prm.brox_scale_factor);
    for (size_t l = 0; l < lv.size(); ++l) {
        const BLevel &L = lv[l];
        auto P = [&](int plane) { return (long long)plane * pyr_elems + L.off; };
        brox_launch_deriv(c->stream, d_frames, frame_elems, d_frame_slots, n, P(BROX_FP_I), P(BROX_FP_DX), L.w, L.h, L.pitch, 0);
        brox_launch_deriv(c->stream, d_frames, frame_elems, d_frame_slots, n, P(BROX_FP_I), P(BROX_FP_DY), L.w, L.h, L.pitch, 1);
        brox_launch_deriv(c->stream, d_frames, frame_elems, d_frame_slots, n, P(BROX_FP_DX), P(BROX_FP_DXX), L.w, L.h, L.pitch, 0);
        brox_launch_deriv(c->stream, d_frames, frame_elems, d_frame_slots, n, P(BROX_FP_DY), P(BROX_FP_DYY), L.w, L.h, L.pitch, 1);
        brox_launch_deriv(c->stream, d_frames, frame_elems, d_frame_slots, n, P(BROX_FP_DX), P(BROX_FP_DXY), L.w, L.h, L.pitch, 1);
    }
    c->stats.kernel_launches += 1 + (lv.size() - 1) + 5 * lv.size();
    return DFX_OK;
}

BroxLevelCtx BroxEngine::level_ctx(int l, int nb) const {
    BroxLevelCtx x;
    std::memset(&x, 0, sizeof x);
    x.w = lv[l].w;
    x.h = lv[l].h;
    x.pitch = lv[l].pitch;
    x.lvl_off = lv[l].off;
    x.frames = d_frames;
    x.frame_stride = frame_elems;
    x.pyr_elems = pyr_elems;
    x.planes = d_planes;
    x.plane_stride = plane_stride;
    x.slot_stride = slot_stride;
    x.pairs = pairs.dev;
    x.n_pairs = nb;
    x.alpha = c->prm.brox_alpha;
    x.gamma = c->prm.brox_gamma;
    x.omega = 1.99f;
    x.sor_sink = d_sor_sink;
    x.sor_progress = (c->prm.variant & DFX_VAR_BROX_SOR_PROGRESS) ? 1 : 0;
    x.sor_stream = (c->prm.variant & (DFX_VAR_BROX_SOR_PROGRESS | DFX_VAR_BROX_SOR_PER_TILE)) ? 0 : n_cu;
    return x;
}

int BroxEngine::run_pairs(int nb, const PairDesc *h_pairs, float *d_out, long long out_stride, const DfxPlanarOut *planar,
                          const DfxSeedIn *seed) {
    if (seed) // upstream's BroxOpticalFlow takes no initial flow
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "brox has no initial flow");
    pairs.stage(h_pairs, nb);
    HIPCHK(c, hipMemcpyAsync(pairs.dev, pairs.host, pairs.bytes(nb), hipMemcpyHostToDevice, c->stream));
    const dfx_params &p = c->prm;
    int uv = 0;
    batch_launches = 0;
    HIPCHK(c, hipEventRecord(ev[0], c->stream));
    for (int l = (int)lv.size() - 1; l >= 0; --l) {
        const BroxLevelCtx x = level_ctx(l, nb);
        brox_launch_level_init(c->stream, x, uv, l == (int)lv.size() - 1);
        int ds = 0; // du/dv set holding the current increment
        for (int in = 0; in < p.brox_inner_iterations; ++in) {
            brox_launch_stage1(c->stream, x, uv, ds);
            if (p.impl == 1) { // simple form: stage 2 as its own launch, then one launch per half sweep, in place
                brox_launch_stage2(c->stream, x);
                for (int si = 0; si < p.brox_solver_iterations; ++si) {
                    brox_launch_sor(c->stream, x, uv, ds, 0);
                    brox_launch_sor(c->stream, x, uv, ds, 1);
                }
            } else {
                const int S = brox_fused_sweeps();
                for (int si = 0; si < p.brox_solver_iterations; si += S) {
                    brox_launch_sor_fused(c->stream, x, uv, ds, std::min(S, p.brox_solver_iterations - si));
                    ds ^= 1; // it wrote the other set
                }
            }
        }
        brox_launch_add_increment(c->stream, x, uv, ds);
        batch_launches += 2 + (uint64_t)p.brox_inner_iterations *
                                  (1 + (p.impl == 1 ? 1 + 2 * p.brox_solver_iterations
                                                    : (p.brox_solver_iterations + brox_fused_sweeps() - 1) / brox_fused_sweeps()));
        if (l > 0) {
            brox_launch_prolongate(c->stream, x, uv, lv[l - 1].w, lv[l - 1].h, lv[l - 1].pitch, p.brox_scale_factor,
                                   1.0f / p.brox_scale_factor);
            uv ^= 1;
            batch_launches += 1;
        } else {
            if (planar)
                brox_launch_merge_planar(c->stream, x, uv, *planar);
            else
                brox_launch_merge(c->stream, x, uv, d_out, out_stride);
            batch_launches += 1;
        }
    }
    HIPCHK(c, hipEventRecord(ev[1], c->stream));
    c->stats.kernel_launches += batch_launches;
    return DFX_OK;
}

// Byte model (defined in DESIGN.md §4): per level N px, per inner iteration stage 1+2 move 100 B/px and every
// red+black SOR sweep 52 B/px (13 float planes touched once).
int BroxEngine::account(int nb) {
    dfx_stats &st = c->stats;
    const dfx_params &p = c->prm;
    double bytes = 0, sor_bytes = 0;
    for (const BLevel &L : lv) {
        const double N = (double)L.w * L.h;
        const double s = N * p.brox_inner_iterations * p.brox_solver_iterations * 52.0;
        bytes += N * p.brox_inner_iterations * 100.0 + s + N * 40.0;
        sor_bytes += s;
    }
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    st.step_ms += ms;
    st.step_launches += batch_launches;
    st.algorithmic_bytes += bytes * nb;
    st.step_algorithmic_bytes += bytes * nb;
    (void)sor_bytes;
    st.pairs += (uint64_t)nb;
    dfx_stats_levels(st, lv.size(), [&](int l) { return std::make_pair(lv[l].w, lv[l].h); });
    return DFX_OK;
}

} // namespace

AlgoEngine *dfx_make_brox_engine(dfx_context *c) { return new BroxEngine(c); }
