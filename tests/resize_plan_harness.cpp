// tests/resize_plan_harness.cpp — TEST INFRASTRUCTURE: C wrappers around denseflow_amd/csrc/engine_plan.h (the host
// arithmetic every engine's create() and set_size() run) and the clip-boundary rule of dfx_plan.h, so that
// tests/test_resize_plan_cpu.py can drive them on the CPU.
#include "../denseflow_amd/csrc/dfx_plan.h"
#include "../denseflow_amd/csrc/engine_plan.h"

namespace {
struct Out {
    long long *p;
    int cap, n = 0;
    void put(long long v) {
        if (n < cap)
            p[n] = v;
        ++n;
    }
    void putf(double v) { // exact: the bits
        long long b = 0;
        static_assert(sizeof b == sizeof v, "");
        __builtin_memcpy(&b, &v, sizeof v);
        put(b);
    }
};
dfx_params params(int max_batch) {
    dfx_params p{};
    p.tvl1_tau = 0.25, p.tvl1_lambda = 0.15, p.tvl1_theta = 0.3, p.tvl1_nscales = 5, p.tvl1_warps = 5;
    p.tvl1_epsilon = 0.01, p.tvl1_iterations = 300, p.tvl1_scale_step = 0.8;
    p.farn_num_levels = 5, p.farn_pyr_scale = 0.5, p.farn_win_size = 13, p.farn_num_iters = 10, p.farn_poly_n = 5;
    p.farn_poly_sigma = 1.1;
    p.brox_alpha = 0.197f, p.brox_gamma = 50.0f, p.brox_scale_factor = 0.8f;
    p.brox_inner_iterations = 10, p.brox_outer_iterations = 77, p.brox_solver_iterations = 10;
    p.max_batch = max_batch;
    return p;
}
} // namespace

extern "C" {

// Every field of the plan for w x h, written to out (returns the count); w0 > 0: the SAME plan object is planned for
// w0 x h0 first, as dfx_set_size does to an engine.
int rp_tvl1(int w0, int h0, int w, int h, int max_batch, long long *out, int cap) {
    const dfx_params p = params(max_batch);
    Tvl1Plan pl;
    if (w0 > 0)
        tvl1_plan(pl, w0, h0, p);
    tvl1_plan(pl, w, h, p);
    Out o{out, cap};
    o.put(pl.W), o.put(pl.H), o.put(pl.nlevels);
    for (int s = 0; s < DFX_LVL_MAX; ++s)
        o.put(pl.lv[s].w), o.put(pl.lv[s].h), o.put(pl.lv[s].pitch), o.put(pl.lv[s].off);
    o.put(pl.frame_elems), o.put(pl.plane_stride), o.put(pl.slot_stride), o.put(pl.partials_stride), o.put(pl.batch);
    o.put((long long)pl.per_pair), o.put(pl.slot_too_large);
    return o.n;
}

int rp_farn(int w0, int h0, int w, int h, int max_batch, long long *out, int cap) {
    const dfx_params p = params(max_batch);
    FarnPlan pl;
    if (w0 > 0)
        farn_plan(pl, w0, h0, p, 4);
    farn_plan(pl, w, h, p, 4);
    Out o{out, cap};
    o.put(pl.W), o.put(pl.H), o.put(pl.nlev);
    for (int k = 0; k < DFX_LVL_MAX; ++k) {
        const FarnPlanLevel &L = pl.lv[k];
        o.put(L.w), o.put(L.h), o.put(L.pitch), o.put(L.r_off), o.putf(L.sigma), o.put(L.half), o.put(L.ker_off);
        o.putf(L.ifx), o.putf(L.ify);
    }
    o.put((long long)pl.taps.size());
    for (float t : pl.taps)
        o.putf(t);
    o.put(pl.frame_elems), o.put(pl.pitch0), o.put(pl.plane_stride), o.put(pl.slot_stride), o.put(pl.batch);
    o.put((long long)pl.per_pair), o.put(pl.bad_kernel);
    return o.n;
}

int rp_brox(int w0, int h0, int w, int h, int max_batch, long long *out, int cap) {
    const dfx_params p = params(max_batch);
    BroxPlan pl;
    if (w0 > 0)
        brox_plan(pl, w0, h0, p, 6, 15);
    brox_plan(pl, w, h, p, 6, 15);
    Out o{out, cap};
    o.put(pl.W), o.put(pl.H), o.put((long long)pl.lv.size());
    for (const DfxPlanLevel &L : pl.lv)
        o.put(L.w), o.put(L.h), o.put(L.pitch), o.put(L.off);
    o.put(pl.pyr_elems), o.put(pl.frame_elems), o.put(pl.plane_stride), o.put(pl.slot_stride), o.put(pl.batch);
    o.put((long long)pl.per_pair);
    return o.n;
}

int rp_frames_batch(int w, int h, int max_batch) { return frames_plan_batch(w, h, max_batch); }
int rp_fit_batch(int B, long long per_pair, long long free_bytes) {
    return dfx_plan_fit_batch(B, (size_t)per_pair, (size_t)free_bytes);
}

// pairs of a FlowBuffer of several clips: returns M; lo[i], hi[i] frame ids over the whole buffer
int rp_pairs(const int *seg, int n_seg, int step, int *lo, int *hi, int cap) {
    const DfxPairs p = dfx_build_pairs(std::vector<int>(seg, seg + n_seg), step);
    for (int i = 0; i < p.size() && i < cap; ++i)
        lo[i] = p.lo[i], hi[i] = p.hi[i];
    return p.size();
}

// A FlowBuffer of clips with their own source sizes, cut into batches: every batch's new frames as runs of one size.
// Row k of out = {batch, first frame id of the run, frames, clip the run takes its size from}; returns the row count.
int rp_format_runs(const int *seg, const int *wh, int n_seg, int step, int batch, long long *out, int cap) {
    std::vector<int> s(seg, seg + n_seg), w, h, clip_of;
    for (int k = 0; k < n_seg; ++k) {
        w.push_back(wh[2 * k]), h.push_back(wh[2 * k + 1]);
        clip_of.insert(clip_of.end(), (size_t)seg[k], k);
    }
    const DfxPairs p = dfx_build_pairs(s, step);
    const std::vector<DfxBatchPlan> plan = dfx_plan_batches(p, batch);
    int rows = 0;
    for (size_t b = 0; b < plan.size(); ++b)
        for (const DfxFormatRun &r : dfx_format_runs(w, h, clip_of, plan[b].first_new, plan[b].n_new)) {
            if (rows < cap)
                out[4 * rows] = (long long)b, out[4 * rows + 1] = plan[b].first_new + r.j0, out[4 * rows + 2] = r.n,
                        out[4 * rows + 3] = r.clip;
            ++rows;
        }
    return rows;
}
}
