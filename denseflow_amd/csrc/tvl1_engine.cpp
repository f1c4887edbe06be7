// tvl1_engine.cpp — host control of the -a=tvl1 path (replaces cv::cuda::OpticalFlowDual_TVL1::calc
// as called at /root/reference/src/denseflow_gpu.cpp:327; algorithm: SURVEY.md Appendix A).
//
//   * all device memory is allocated once per handle (the reference re-creates the OpenCV algorithm
//     object, and with it every GpuMat, per FlowBuffer: src/denseflow_gpu.cpp:299, :345-355);
//   * a frame's float pyramid + centred gradient is built once and used as I1 of pair i and as I0
//     of pair i+step (the reference re-uploads and re-converts both frames of every pair, :317-318);
//   * `batch` pairs advance together through every launch (grid.z = pair), each with its own
//     device-side convergence state (tvl1_ctrl.h), so there is no host sync inside a pair — the
//     reference syncs the stream at every convergence check.  The host enqueues
//     groups of identical step launches and only looks at one pinned word per group to learn that
//     every pair has finished the level.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "dfx_internal.h"
#include "tvl1_kernels.h"

namespace {

using Level = DfxPlanLevel; // engine_plan.h

class Tvl1Engine final : public AlgoEngine {
  public:
    explicit Tvl1Engine(dfx_context *ctx) : c(ctx) {}
    ~Tvl1Engine() override { destroy(); }

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
    int batch_tables(int max_pairs, int *iters, int *checks) const override;

  private:
    void destroy();
    int grow_frame_slots(int need, long long elems);
    DfxSlotBufs slot_bufs(long long elems) { // engine_buffers.h: a frame slot is `elems` floats in each pyramid
        DfxSlotBufs s;
        s.add(dI, pyr_cap[0], (size_t)elems * sizeof(float));
        s.add(dIx, pyr_cap[1], (size_t)elems * sizeof(float));
        s.add(dIy, pyr_cap[2], (size_t)elems * sizeof(float));
        return s;
    }
    int slots_held() { return dfx_frame_slots_held(slot_bufs(frame_elems), slots.cap); }
    Tvl1LevelCtx level_ctx(int s, int n_pairs) const;
    int steps_per_group(int s, int nb) const;
    int refuse_if_too_large(const Tvl1Plan &pl);

    dfx_context *c;
    DfxHipAlloc mem{c};
    int nlevels = 0;
    Level lv[DFX_LVL_MAX];
    long long frame_elems = 0;

    int n_frame_slots = 0;
    float *dI = nullptr, *dIx = nullptr, *dIy = nullptr;
    DfxTable<int> slots; // frame-slot ids of build_frames
    // what the buffers hold, in bytes (they only grow: set_size re-plans the engine inside them); pyr_cap: dI / dIx / dIy
    size_t pyr_cap[3] = {0, 0, 0}, planes_cap = 0, partials_cap = 0;

    int B = 0;
    float *d_planes = nullptr;
    long long plane_stride = 0, slot_stride = 0;
    int n_planes = PL_COUNT; // planes of a pair slot (the plan's: PL_COUNT_GAMMA with the illumination channel)
    bool gamma_on = false;   // dfx_params.tvl1_gamma != 0: a pair slot has the planes of u3 / p31 / p32 and their kernels run
    // the per-pair arrays: they grow together (dfx_grow_tables), so pairs.cap is the pairs every one of them holds
    DfxTable<Tvl1State> state{1, false};
    DfxTable<PairDesc> pairs;                               // descriptors of run_pairs
    DfxTable<int> iter_tab{DFX_LVL_MAX * TVL1_MAX_WARPS};   // read back after every batch, as are check_tab and work_tab
    DfxTable<int> check_tab{DFX_LVL_MAX * 2};
    DfxTable<long long> work_tab{DFX_LVL_MAX * 2};
    double *d_partials = nullptr;
    int partials_stride = 0;
    unsigned int *d_level_done = nullptr;
    int *h_done_flag = nullptr, *d_done_flag = nullptr;
    hipEvent_t ev_group[2] = {nullptr, nullptr};
    hipEvent_t ev_lvl[DFX_LVL_MAX][2] = {};
    int done_token = 0;
    int group_override = 0;
    int min_group = 2;
    bool split_warp = false; // backward warp as its own kernel in front of every step (packed step kernels only)
    int geom = 0;            // 1 = tile columns of the step kernel start at x = 0 (Tvl1LevelCtx::geom)
    bool warp_head = false;  // the warp kernel also runs the head of the loop it starts (k_tvl1_warp_head)
    int launched_steps[DFX_LVL_MAX] = {0};
    int last_nb = 0; // pairs of the batch whose read-backs iter_tab / check_tab hold (set by account)
    double seed_bytes_pair = 0; // bytes per pair the seed chain of the batch in flight moved (0: no seed; folded in by account)

    Tvl1LoopCfg loop{};
    Tvl1Consts kc{};
};

void Tvl1Engine::destroy() {
    dfx_free_dev(dI);
    dfx_free_dev(dIx);
    dfx_free_dev(dIy);
    slots.release(mem);
    dfx_free_dev(d_planes);
    state.release(mem), pairs.release(mem), iter_tab.release(mem), check_tab.release(mem), work_tab.release(mem);
    dfx_free_dev(d_partials);
    dfx_free_dev(d_level_done);
    dfx_free_host(h_done_flag);
    dfx_destroy_events(ev_group, 2);
    dfx_destroy_events(&ev_lvl[0][0], DFX_LVL_MAX * 2);
}

int Tvl1Engine::create() {
    const dfx_params &p = c->prm;
    if (p.tvl1_nscales < 1 || p.tvl1_nscales > DFX_LVL_MAX || p.tvl1_warps < 0 || p.tvl1_warps > TVL1_MAX_WARPS ||
        p.tvl1_iterations < 0 || !(p.tvl1_scale_step > 0.0 && p.tvl1_scale_step < 1.0) || !(p.tvl1_theta > 0.0))
        return dfx_fail(c, DFX_ERR_INVALID, "invalid TVL1 parameters");
    if (p.impl < 0 || p.impl > 2)
        return dfx_fail(c, DFX_ERR_INVALID, "tvl1: impl must be 0 (tuned), 1 (simple) or 2 (scalar tile function)");
    if (p.tvl1_math < 0 || p.tvl1_math > 3 || (p.tvl1_math == 1 && p.impl != 0))
        return dfx_fail(c, DFX_ERR_INVALID,
                        "tvl1_math must be 0 (exact), 1 (fast; tuned kernel only), 2 (exact, sqrtf hypot) or 3 (exact, "
                        "libm hypot)");
    if (!std::isfinite(p.tvl1_gamma))
        return dfx_fail(c, DFX_ERR_INVALID, "tvl1_gamma must be finite");
    gamma_on = p.tvl1_gamma != 0.0;
    if (gamma_on && p.tvl1_math != 0)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "tvl1_gamma != 0 runs the exact arithmetic with the default hypot reading only (tvl1_math 0)");
    if (gamma_on && p.impl == 2)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "tvl1_gamma != 0 has no scalar tile function (impl 0 or 1)");
    // The gamma tile kernel has no warp phase: the dedicated warp kernel always runs in front of it.  That kernel has only
    // ever run with tvl1_iterations > 0 (split_warp below), where a warp always leads into phase ITER; the gamma route
    // keeps that condition and opens no configuration of it that the default path does not run.  (With zero iterations no
    // update of A.6 / A.7 would run and the flow would be the gamma = 0 flow: ask for that.)
    if (gamma_on && p.tvl1_iterations == 0)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "tvl1_gamma != 0 needs tvl1_iterations > 0");
    {
        // the size rule before anything is allocated (set_size applies it again to every later size)
        Tvl1Plan pl;
        tvl1_plan(pl, c->W, c->H, p);
        if (const int rc = refuse_if_too_large(pl))
            return rc;
    }
    group_override = std::max(0, std::min(p.step_group, 64));
    // the dedicated warp kernel does not write the grad plane: only the packed tile function (impl 0) rebuilds it;
    // zero iterations: warps inside the step kernel.  DFX_VAR_TVL1_WARP_IN_STEP names a form the gamma route lacks: ignored there
    split_warp = p.impl == 0 && p.tvl1_iterations > 0 && (gamma_on || !(p.variant & DFX_VAR_TVL1_WARP_IN_STEP));
    // tile columns from x = 0 (tvl1_ctrl.h) need every warp outside the step kernel (its warp phase tiles classically)
    geom = (p.impl == 0 && split_warp && !(p.variant & DFX_VAR_TVL1_CLASSIC_GEOM)) ? 1 : 0;
    // warp + head of the loop in one launch (round 6): the tuned forms only — every cross-check variant keeps its own kernels
    // (the warp does not read u3: gamma handles take the dedicated warp kernel plus step launches, as NO_HEAD does)
    warp_head = split_warp && geom == 1 && !gamma_on && !(p.variant & (DFX_VAR_TVL1_NO_HEAD | DFX_VAR_TVL1_WARP_GATHER));

    loop.warps = p.tvl1_warps;
    loop.iterations = p.tvl1_iterations;
    if (p.impl == 1)
        loop.fuse_k = 1;
    else
        loop.fuse_k = std::max(1, std::min(p.tvl1_fuse_k > 0 ? p.tvl1_fuse_k : 4, tvl1_fused_max_k()));
    kc.l_t = (float)(p.tvl1_lambda * p.tvl1_theta);
    kc.taut = (float)(p.tvl1_tau / p.tvl1_theta);
    kc.theta = (float)p.tvl1_theta;
    kc.hyp = p.tvl1_math == 1 ? 0 : p.tvl1_math; // tvl1_math.h: TVL1_HYP_* (the fast mode never reaches a scalar form)
    kc.gamma = (float)p.tvl1_gamma;              // passed as float (A.6 with gamma)

    HIPCHK(c, hipMalloc(&d_level_done, sizeof(unsigned int)));
    HIPCHK(c, hipHostMalloc(&h_done_flag, 64, hipHostMallocMapped));
    HIPCHK(c, hipHostGetDevicePointer((void **)&d_done_flag, h_done_flag, 0));
    HIPCHK(c, hipEventCreateWithFlags(&ev_group[0], dfx_event_flags(c, false)));
    HIPCHK(c, hipEventCreateWithFlags(&ev_group[1], dfx_event_flags(c, false)));
    for (auto &e : ev_lvl) {
        HIPCHK(c, hipEventCreateWithFlags(&e[0], dfx_event_flags(c, true)));
        HIPCHK(c, hipEventCreateWithFlags(&e[1], dfx_event_flags(c, true)));
    }
    return set_size(c->W, c->H);
}

size_t Tvl1Engine::device_bytes() const {
    const size_t per_pair = sizeof(Tvl1State) + sizeof(PairDesc) + sizeof(int) * DFX_LVL_MAX * (TVL1_MAX_WARPS + 2) +
                            sizeof(long long) * DFX_LVL_MAX * 2;
    return planes_cap + partials_cap + pyr_cap[0] + pyr_cap[1] + pyr_cap[2] + sizeof(int) * (size_t)slots.cap + per_pair * (size_t)pairs.cap +
           (d_level_done ? sizeof(unsigned int) : 0);
}

// Plan (engine_plan.h: host arithmetic) + ensure capacity.  Nothing of the engine changes before the last allocation has
// succeeded; the buffers a failed attempt has already grown stay grown.
int Tvl1Engine::refuse_if_too_large(const Tvl1Plan &pl) {
    if (!pl.slot_too_large)
        return DFX_OK;
    if (pl.n_planes == PL_COUNT_GAMMA)
        return dfx_fail(c, DFX_ERR_INVALID, "tvl1: frame too large for tvl1_gamma != 0 (a pair's 22 work planes must stay below 4 GiB: round_up(width, 64) x height x 88 B < 2^32)");
    return dfx_fail(c, DFX_ERR_INVALID, "tvl1: frame too large (a pair's 16 work planes must stay below 4 GiB: round_up(width, 64) x height x 64 B < 2^32)");
}

int Tvl1Engine::set_size(int W, int H) {
    Tvl1Plan pl;
    tvl1_plan(pl, W, H, c->prm); // with the handle's own plane count (tvl1_gamma is part of its parameters)
    if (const int rc = refuse_if_too_large(pl))
        return rc;
    // batch: enough pairs that the coarse levels fill 256 CUs, bounded by memory — by what is free now plus what this
    // engine holds and would give back for a larger allocation
    const size_t slot_bytes = (size_t)pl.slot_stride * sizeof(float);
    int nB = 0;
    if (const int rc = dfx_fit_pair_slots(mem, pl.batch, pl.per_pair, slot_bytes, device_bytes(), d_planes, planes_cap, B, nB))
        return rc;
    if (nB > pairs.cap) {
        if (!dfx_grow_tables(mem, nB, state, pairs, iter_tab, check_tab, work_tab))
            return dfx_fail(c, DFX_ERR_HIP, "tvl1: allocating the per-pair tables failed");
        // as create leaves them: should a later allocation of this call fail, the engine goes on at its old size on these
        HIPCHK(c, hipMemset(state.dev, 0, state.bytes(pairs.cap)));
        HIPCHK(c, hipMemset(work_tab.dev, 0, work_tab.bytes(pairs.cap)));
    }
    if (const int rc = dfx_grow(mem, d_partials, partials_cap, sizeof(double) * (size_t)pl.partials_stride * nB))
        return rc;
    const int rc = grow_frame_slots(nB + 1, pl.frame_elems);
    if (rc != DFX_OK) { // the engine goes on at its old size, on the frame slots the pyramids still hold
        dfx_settle_frame_slots(n_frame_slots, rc, slots_held());
        return rc;
    }
    // commit: the geometry every launch derives its Tvl1LevelCtx from, and the control state as it is after create
    nlevels = pl.nlevels;
    for (int s = 0; s < DFX_LVL_MAX; ++s)
        lv[s] = pl.lv[s];
    frame_elems = pl.frame_elems;
    plane_stride = pl.plane_stride;
    slot_stride = pl.slot_stride;
    n_planes = pl.n_planes;
    partials_stride = pl.partials_stride;
    B = nB;
    dfx_settle_frame_slots(n_frame_slots, DFX_OK, slots_held());
    HIPCHK(c, hipMemset(state.dev, 0, state.bytes(pairs.cap)));
    HIPCHK(c, hipMemset(work_tab.dev, 0, work_tab.bytes(pairs.cap)));
    HIPCHK(c, hipMemset(d_level_done, 0, sizeof(unsigned int)));
    *h_done_flag = 0;
    done_token = 0;
    last_nb = 0;
    for (auto &n : launched_steps)
        n = 0;
    return DFX_OK;
}

// `need` frame slots of `elems` floats per pyramid
int Tvl1Engine::grow_frame_slots(int need, long long elems) {
    if (const int rc = dfx_grow_slot_bufs(mem, slot_bufs(elems), need))
        return rc;
    if (!dfx_grow_tables(mem, need, slots))
        return dfx_fail(c, DFX_ERR_HIP, "tvl1: allocating the frame-slot tables failed");
    return DFX_OK;
}

int Tvl1Engine::ensure_frame_slots(int need) {
    if (need <= n_frame_slots)
        return DFX_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = grow_frame_slots(need, frame_elems);
    dfx_settle_frame_slots(n_frame_slots, rc, slots_held());
    return rc;
}

// float pyramids + centred gradients (A.2 steps 1-3, A.3) of `n` new frames
int Tvl1Engine::build_frames(const unsigned char *d_src, long long src_frame_stride, long long src_pitch, int n,
                             const int *h_slots) {
    if (n <= 0)
        return DFX_OK;
    int *const d_frame_slots = slots.dev;
    slots.stage(h_slots, n);
    HIPCHK(c, hipMemcpyAsync(d_frame_slots, slots.host, slots.bytes(n), hipMemcpyHostToDevice, c->stream));
    const Level &L0 = lv[0];
    tvl1_launch_u8_to_f32(c->stream, d_src, src_frame_stride, src_pitch, d_frame_slots, n, dI, frame_elems, L0.w, L0.h,
                          L0.pitch);
    const float ifs = (float)(1.0 / c->prm.tvl1_scale_step); // the given fx is kept (E.1)
    for (int s = 1; s < nlevels; ++s) {
        const Level &A = lv[s - 1], &Bq = lv[s];
        tvl1_launch_pyr_down(c->stream, dI, frame_elems, d_frame_slots, n, A.off, A.w, A.h, A.pitch, Bq.off, Bq.w, Bq.h,
                             Bq.pitch, ifs, ifs);
    }
    for (int s = 0; s < nlevels; ++s) {
        const Level &L = lv[s];
        tvl1_launch_centered_gradient(c->stream, dI, dIx, dIy, frame_elems, d_frame_slots, n, L.off, L.w, L.h, L.pitch);
    }
    c->stats.kernel_launches += 1 + (nlevels - 1) + nlevels;
    return DFX_OK;
}

Tvl1LevelCtx Tvl1Engine::level_ctx(int s, int n_pairs) const {
    Tvl1LevelCtx x;
    std::memset(&x, 0, sizeof x);
    const Level &L = lv[s];
    x.w = L.w;
    x.h = L.h;
    x.pitch = L.pitch;
    x.frame_I = dI;
    x.frame_Ix = dIx;
    x.frame_Iy = dIy;
    x.frame_stride = frame_elems;
    x.lvl_off = L.off;
    x.planes = d_planes;
    x.plane_stride = plane_stride;
    x.slot_stride = slot_stride;
    x.state = state.dev;
    x.pairs = pairs.dev;
    x.partials = d_partials;
    x.partials_stride = partials_stride;
    x.n_pairs = n_pairs;
    x.loop = loop;
    x.k = kc;
    x.thr = c->prm.tvl1_epsilon * c->prm.tvl1_epsilon * (double)(L.w * L.h);
    x.level = s;
    x.iters_out = iter_tab.dev;
    x.checks_out = check_tab.dev;
    x.work_out = work_tab.dev;
    x.level_done_count = d_level_done;
    x.host_done_flag = d_done_flag;
    x.done_token = 0;
    x.split_warp = split_warp ? 1 : 0;
    x.warp_lds = (c->prm.variant & DFX_VAR_TVL1_WARP_GATHER) ? 0 : 1;
    x.geom = geom;
    x.head = warp_head ? 1 : 0;
    x.n_planes = n_planes;
    return x;
}

int Tvl1Engine::steps_per_group(int s, int nb) const {
    if (group_override > 0)
        return group_override;
    // aim at >= ~150 us of device work per group: the host stays ahead of the device and the event
    // record between groups (~6 us of idle queue) stays below a few percent
    const double px = (double)lv[s].w * lv[s].h * nb;
    const double step_us = 2.0 + px * 64.0 * loop.fuse_k / 4.0e6; // bytes / (4 TB/s) in us
    const int g = (int)std::ceil(150.0 / step_us);
    // at least 2: the launches enqueued behind a level's last useful step (up to two groups: the host looks at the group
    // before the one it has just enqueued) find nothing to do and cost 14-57 us each at 1080p x 129 pairs
    return std::max(min_group, std::min(16, g));
}

int Tvl1Engine::run_pairs(int nb, const PairDesc *h_pairs, float *d_out, long long out_stride, const DfxPlanarOut *planar,
                          const DfxSeedIn *seed) {
    last_nb = 0; // the read-backs below overwrite the last batch's tables
    seed_bytes_pair = 0;
    pairs.stage(h_pairs, nb);
    HIPCHK(c, hipMemcpyAsync(pairs.dev, pairs.host, pairs.bytes(nb), hipMemcpyHostToDevice, c->stream));
    const int impl = c->prm.impl, math = c->prm.tvl1_math;
    const bool nbr_lds = (c->prm.variant & DFX_VAR_TVL1_STEP_NBR_LDS) != 0;
    const bool head_regs = (c->prm.variant & DFX_VAR_TVL1_HEAD_NBR_LDS) != 0;
    const float up = (float)(1.0 / c->prm.tvl1_scale_step);
    const int hard_limit = loop.warps * (loop.iterations + 2) + 64;

    if (seed) {
        // The caller's initial flows down to the coarsest level (tvl1_seed_kernels.hip): one launch per pyramid step, the
        // first one reading the caller's rows, the others ping-ponging between the u plane sets so that the last one
        // writes set 0.  One level: the seed as it is.
        Tvl1SeedStep q;
        std::memset(&q, 0, sizeof q);
        if (nlevels == 1) {
            q.src = *seed, q.sw = lv[0].w, q.sh = lv[0].h, q.dst_set = 0, q.copy = 1;
            tvl1_launch_seed_step(c->stream, level_ctx(0, nb), q);
            seed_bytes_pair += 16.0 * lv[0].w * lv[0].h;
        }
        for (int s = 1; s < nlevels; ++s) {
            const Level &S = lv[s - 1], &D = lv[s];
            const Tvl1LevelCtx xd = level_ctx(s, nb);
            q.dst_set = (nlevels - 1 - s) & 1;
            q.src = s == 1 ? *seed : tvl1_seed_from_planes(xd, q.dst_set ^ 1, S.pitch);
            q.sw = S.w, q.sh = S.h;
            q.ifx = (float)(1.0 / ((double)D.w / (double)S.w));
            q.ify = (float)(1.0 / ((double)D.h / (double)S.h));
            q.mul = (float)c->prm.tvl1_scale_step;
            tvl1_launch_seed_step(c->stream, xd, q);
            seed_bytes_pair += 40.0 * D.w * D.h; // per pixel and channel: four taps read, one value written
        }
        c->stats.kernel_launches += (uint64_t)std::max(1, nlevels - 1);
    }
    for (int s = nlevels - 1; s >= 0; --s) {
        Tvl1LevelCtx x = level_ctx(s, nb);
        x.done_token = ++done_token;
        const bool first = s == nlevels - 1;
        if (first && seed)
            tvl1_launch_level_begin_seeded(c->stream, x); // u is the chain's, in set 0
        else
            tvl1_launch_level_begin(c->stream, x, first);
        c->stats.kernel_launches += (warp_head && !(first && !seed)) ? 1 : 2;
        if (gamma_on) {
            tvl1_launch_level_begin_gamma(c->stream, x, s == nlevels - 1);
            c->stats.kernel_launches += 1;
        }
        launched_steps[s] = 0;
        if (loop.warps > 0) {
            const int G = steps_per_group(s, nb);
            int step_id = 0;
            HIPCHK(c, hipEventRecord(ev_lvl[s][0], c->stream));
            for (int g = 0;; ++g) {
                for (int i = 0; i < G; ++i) {
                    if (warp_head)
                        tvl1_launch_warp_head(c->stream, x, step_id, math, head_regs);
                    else if (split_warp)
                        tvl1_launch_warp(c->stream, x, step_id);
                    if (gamma_on)
                        tvl1_launch_step_gamma(c->stream, x, step_id++, impl);
                    else
                        tvl1_launch_step(c->stream, x, step_id++, impl, math, nbr_lds);
                }
                c->stats.kernel_launches += (uint64_t)G * (split_warp ? 2 : 1);
                HIPCHK(c, hipEventRecord(ev_group[g & 1], c->stream));
                if (g >= 1) { // look at the group before the one just enqueued: the device never idles
                    HIPCHK(c, hipEventSynchronize(ev_group[(g - 1) & 1]));
                    if (*(volatile int *)h_done_flag == x.done_token)
                        break;
                }
                if (step_id > hard_limit + 2 * G) {
                    HIPCHK(c, dfx_stream_wait(c, c->stream));
                    if (*(volatile int *)h_done_flag == x.done_token)
                        break;
                    return dfx_fail(c, DFX_ERR_HIP, "TVL1 level did not terminate within its step bound");
                }
            }
            launched_steps[s] = step_id;
            HIPCHK(c, hipEventRecord(ev_lvl[s][1], c->stream));
        }
        if (s > 0) {
            const Level &D = lv[s - 1], &S = lv[s];
            const float ifx = (float)(1.0 / ((double)D.w / (double)S.w));
            const float ify = (float)(1.0 / ((double)D.h / (double)S.h));
            tvl1_launch_upsample_u(c->stream, x, D.w, D.h, D.pitch, ifx, ify, up);
            if (gamma_on) {
                tvl1_launch_upsample_u3(c->stream, x, D.w, D.h, D.pitch, ifx, ify);
                c->stats.kernel_launches += 1;
            }
        } else if (planar) {
            tvl1_launch_merge_planar(c->stream, x, *planar);
        } else {
            tvl1_launch_merge(c->stream, x, d_out, out_stride);
        }
        c->stats.kernel_launches += 1;
    }
    HIPCHK(c, hipMemcpyAsync(iter_tab.host, iter_tab.dev, iter_tab.bytes(nb), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(check_tab.host, check_tab.dev, check_tab.bytes(nb), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(work_tab.host, work_tab.dev, work_tab.bytes(nb), hipMemcpyDeviceToHost, c->stream));
    return DFX_OK;
}

// Fold the read-back iteration counts of a finished batch into the statistics (SURVEY.md §8d byte model).
int Tvl1Engine::account(int nb) {
    dfx_stats &st = c->stats;
    const int *const h_iters = iter_tab.host, *const h_checks = check_tab.host;
    const long long *const h_work = work_tab.host;
    for (int s = 0; s < nlevels && loop.warps > 0; ++s) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev_lvl[s][0], ev_lvl[s][1]));
        st.step_ms += ms;
        st.step_launches += (uint64_t)launched_steps[s];
        st.level_ms[s] += ms;
        st.level_launches[s] += (uint64_t)launched_steps[s];
        int useful = 0;
        for (int b = 0; b < nb; ++b)
            useful = std::max(useful, h_checks[(b * DFX_LVL_MAX + s) * 2 + 1]);
        st.noop_steps += (uint64_t)std::max(0, launched_steps[s] - useful);
    }
    int step_tiles[DFX_LVL_MAX] = {0}, head_tiles[DFX_LVL_MAX] = {0}; // workgroups per pair of the two launches of a step
    for (int s = 0; s < nlevels && c->prm.impl == 0; ++s) {
        const Tvl1LevelCtx x = level_ctx(s, 1);
        step_tiles[s] = tvl1_step_blocks(x, 0);
        head_tiles[s] = tvl1_head_blocks(x);
    }
    for (int b = 0; b < nb; ++b) {
        for (int s = 0; s < nlevels; ++s) {
            const double px = (double)lv[s].w * lv[s].h;
            long long it = 0;
            for (int w = 0; w < loop.warps; ++w)
                it += h_iters[(b * DFX_LVL_MAX + s) * TVL1_MAX_WARPS + w];
            st.tvl1_total_iters += (uint64_t)it;
            st.tvl1_px_iters += px * (double)it;
            // lane-iterations the tuned kernels executed: half rows x 32 lanes x tiles (tvl1_ctrl.h: tvl1_step_work)
            st.tvl1_lane_iters += 32.0 * ((double)h_work[(b * DFX_LVL_MAX + s) * 2 + 0] * step_tiles[s] +
                                          (double)h_work[(b * DFX_LVL_MAX + s) * 2 + 1] * head_tiles[s]);
            // per pixel: an inner iteration reads 10 planes and writes 6 (64 B; with u3, p31, p32: 13 and 9, 88 B), a warp
            // moves 44 B (it does not read u3), a level 28 B (+ 14 B with gamma: two more planes zeroed, u3 upsampled)
            const double it_b = gamma_on ? 88.0 : 64.0, lvl_b = gamma_on ? 42.0 : 28.0;
            st.algorithmic_bytes += px * (it_b * (double)it + 44.0 * loop.warps + lvl_b);
            st.step_algorithmic_bytes += px * (it_b * (double)it + 44.0 * loop.warps);
        }
        st.algorithmic_bytes += seed_bytes_pair;
        st.pairs += 1;
    }
    last_nb = nb;
    const int b = nb - 1;
    dfx_stats_levels(st, nlevels, [&](int s) { return std::make_pair(lv[s].w, lv[s].h); });
    st.tvl1_checks = 0;
    for (int s = 0; s < nlevels; ++s) {
        for (int w = 0; w < DFX_MAX_WARPS; ++w)
            st.tvl1_iters[s][w] = (w < TVL1_MAX_WARPS) ? h_iters[(b * DFX_LVL_MAX + s) * TVL1_MAX_WARPS + w] : 0;
        st.tvl1_checks += h_checks[(b * DFX_LVL_MAX + s) * 2];
    }
    return DFX_OK;
}

// The read-backs of the last accounted batch, pair by pair: iters[pair][DFX_MAX_LEVELS][DFX_MAX_WARPS] and
// checks[pair][DFX_MAX_LEVELS], zero beyond the pyramid and the warps.
int Tvl1Engine::batch_tables(int max_pairs, int *iters, int *checks) const {
    if (last_nb <= 0)
        return -DFX_ERR_INVALID;
    if (max_pairs < last_nb || !iters || !checks)
        return -DFX_ERR_INVALID;
    static_assert(DFX_LVL_MAX <= DFX_MAX_LEVELS && TVL1_MAX_WARPS <= DFX_MAX_WARPS, "tables do not fit dfx.h's");
    const int *const h_iters = iter_tab.host, *const h_checks = check_tab.host;
    std::memset(iters, 0, sizeof(int) * (size_t)last_nb * DFX_MAX_LEVELS * DFX_MAX_WARPS);
    std::memset(checks, 0, sizeof(int) * (size_t)last_nb * DFX_MAX_LEVELS);
    for (int b = 0; b < last_nb; ++b)
        for (int s = 0; s < nlevels; ++s) {
            for (int w = 0; w < loop.warps; ++w)
                iters[((size_t)b * DFX_MAX_LEVELS + s) * DFX_MAX_WARPS + w] =
                    h_iters[(b * DFX_LVL_MAX + s) * TVL1_MAX_WARPS + w];
            checks[(size_t)b * DFX_MAX_LEVELS + s] = h_checks[(b * DFX_LVL_MAX + s) * 2];
        }
    return last_nb;
}

} // namespace

AlgoEngine *dfx_make_tvl1_engine(dfx_context *c) { return new Tvl1Engine(c); }
