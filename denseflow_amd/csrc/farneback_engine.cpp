// farneback_engine.cpp — host control of the -a=farn path (replaces cv::cuda::FarnebackOpticalFlow::calc
// as called at /root/reference/src/denseflow_gpu.cpp:329; algorithm: SURVEY.md Appendix B).
//
// Control flow is fixed (no data-dependent exit), so a pair is a straight sequence of launches with
// no host synchronisation; `batch` pairs share every launch (grid.z = pair).  Per-frame work (u8 ->
// f32, blur+resize per level, polynomial expansion) is done once per frame and reused by both pairs
// the frame belongs to.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>

#include "dfx_internal.h"
#include "farneback_kernels.h"
#include "farneback_plan.h"

namespace {

struct FLevel {
    FarnLevelGeom g;
    double sigma;
    int half;    // Gaussian pre-blur half width (smoothSize / 2)
    int ker_off; // offset of this level's taps (centre first) in d_gker
    float ifx, ify;
};

// B.3: polynomial-expansion constants (identical to upstream FarnebackPrepareGaussian)
void prepare_poly(int n, double sigma, FarnPolyConsts *out) {
    std::vector<float> buf(n * 6 + 3);
    float *g = buf.data() + n, *xg = g + n * 2 + 1, *xxg = xg + n * 2 + 1;
    if (sigma < FLT_EPSILON)
        sigma = n * 0.3;
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)std::exp(-x * x / (2 * sigma * sigma));
        s += g[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        xg[x] = (float)(x * g[x]);
        xxg[x] = (float)(x * x * g[x]);
    }
    // normal matrix of the basis {1, x, y, x^2, y^2, xy} under the applicability g; only four of its
    // entries are distinct, so the 6x6 inverse reduces to a 3x3 block {1, x^2, y^2} plus diagonals
    double a = 0, bq = 0, cq = 0, d = 0;
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            a += g[y] * g[x];
            bq += g[y] * g[x] * x * x;
            cq += g[y] * g[x] * x * x * x * x;
            d += g[y] * g[x] * x * x * y * y;
        }
    // block [[a, b, b], [b, c, d], [b, d, c]] over (1, x^2, y^2): closed-form inverse entries
    const double det = a * (cq * cq - d * d) - 2.0 * bq * bq * (cq - d);
    const double inv03 = -bq * (cq - d) / det;   // (1, x^2)
    const double inv33 = (a * cq - bq * bq) / det; // (x^2, x^2)
    out->ig11 = (float)(1.0 / bq);
    out->ig03 = (float)inv03;
    out->ig33 = (float)inv33;
    out->ig55 = (float)(1.0 / d);
    for (int i = 0; i <= n; ++i) {
        out->g[i] = g[i];
        out->xg[i] = xg[i];
        out->xxg[i] = xxg[i];
    }
}

class FarnebackEngine final : public AlgoEngine {
  public:
    explicit FarnebackEngine(dfx_context *ctx) : c(ctx) {}
    ~FarnebackEngine() override { destroy(); }
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
    int grow_frame_slots(int need, long long elems, long long plane);
    DfxSlotBufs slot_bufs(long long elems, long long plane);
    int slots_held() { return dfx_frame_slots_held(slot_bufs(frame_elems, plane_stride), slots.cap); }
    dfx_context *c;
    DfxHipAlloc mem{c};
    // what the buffers hold, in bytes (they only grow: set_size re-plans the engine inside them)
    size_t gker_cap = 0, R_cap = 0, f32_cap = 0, tmpv_cap = 0, pyr_cap = 0, planes_cap = 0;
    int nlev = 0; // levels 0..nlev-1 (nlev = numLevelsCropped + 1)
    FLevel lv[DFX_LVL_MAX];
    long long frame_elems = 0;
    int pitch0 = 0;
    FarnPolyConsts pc{};
    float *d_gker = nullptr;

    int n_frame_slots = 0;
    float *d_R = nullptr;
    DfxTable<int> slots; // frame-slot ids of build_frames
    // scratch for frame preparation, sized for n_frame_slots frames
    float *d_f32 = nullptr, *d_tmpv = nullptr, *d_pyr = nullptr;
    int skip_zero_weights = 1, polyexp_rows = 16; // frame-preparation forms, fixed when the engine is created
    bool m_on_chip = true;                        // the default iteration kernel (M recomputed, never in HBM)
    double seed_bytes_pair = 0;                   // bytes per pair the seed's resize of the batch in flight read (0: no seed)
    bool gauss_window = false;                    // dfx_params.farn_window: Gaussian taps in place of the box filter
    bool fast_pyr = false;                        // dfx_params.farn_fast_pyramids: pyrDown frame pyramids, pyrUp flows (B.13)
    FarnWinTaps win_taps{};

    int B = 0;
    float *d_planes = nullptr;
    long long plane_stride = 0, slot_stride = 0;
    DfxTable<PairDesc> pairs; // descriptors of run_pairs
    hipEvent_t ev_it[DFX_LVL_MAX][2] = {};
};

void FarnebackEngine::destroy() {
    dfx_free_dev(d_gker);
    dfx_free_dev(d_R);
    slots.release(mem);
    dfx_free_dev(d_f32);
    dfx_free_dev(d_tmpv);
    dfx_free_dev(d_pyr);
    dfx_free_dev(d_planes);
    pairs.release(mem);
    dfx_destroy_events(&ev_it[0][0], DFX_LVL_MAX * 2);
}

int FarnebackEngine::create() {
    const dfx_params &p = c->prm;
    if (p.impl < 0 || p.impl > 1)
        return dfx_fail(c, DFX_ERR_INVALID, "farn: impl must be 0 (tuned) or 1 (simple)");
    // cross-check forms of the frame preparation (dfx_params.variant; same bits both ways)
    skip_zero_weights = (p.variant & DFX_VAR_FARN_EVAL_ZERO_TAPS) ? 0 : farn_skip_zero_weights_default();
    polyexp_rows = (p.variant & DFX_VAR_FARN_POLY_ONE_ROW) ? 0 : farn_polyexp_rows_default();
    if (p.farn_poly_n != 5 && p.farn_poly_n != 7)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "Farneback: polyN must be 5 or 7 (the two expansions upstream builds)");
    if (p.farn_flags != 0)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED,
                        "Farneback: only flags = 0 (the Gaussian window is requested with farn_window, not with flags = 256)");
    if (p.farn_window != DFX_FARN_WINDOW_BOX && p.farn_window != DFX_FARN_WINDOW_GAUSSIAN)
        return dfx_fail(c, DFX_ERR_INVALID, "Farneback: farn_window must be DFX_FARN_WINDOW_BOX or DFX_FARN_WINDOW_GAUSSIAN");
    if (p.farn_win_size < 1 || !(p.farn_win_size & 1) || p.farn_win_size > 31)
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, "Farneback: winSize must be odd and <= 31");
    if (p.farn_num_levels < 0 || p.farn_num_levels >= DFX_LVL_MAX || p.farn_num_iters < 1 ||
        !(p.farn_pyr_scale > 0.0 && p.farn_pyr_scale < 1.0))
        return dfx_fail(c, DFX_ERR_INVALID, "invalid Farneback parameters");
    if (p.farn_fast_pyramids != 0 && p.farn_fast_pyramids != 1)
        return dfx_fail(c, DFX_ERR_INVALID, "Farneback: farn_fast_pyramids must be 0 or 1");
    fast_pyr = p.farn_fast_pyramids == 1;
    if (fast_pyr && p.farn_pyr_scale != 0.5)
        return dfx_fail(c, DFX_ERR_INVALID, "Farneback: farn_fast_pyramids needs farn_pyr_scale = 0.5 (pyrDown halves a level)");

    prepare_poly(p.farn_poly_n, p.farn_poly_sigma, &pc);
    // the Gaussian update window's taps follow from the parameters alone: set_size leaves them alone
    gauss_window = p.farn_window == DFX_FARN_WINDOW_GAUSSIAN;
    if (gauss_window && !farn_window_taps(p.farn_win_size, win_taps))
        return dfx_fail(c, DFX_ERR_INVALID, "Farneback: bad Gaussian window");
    // The default iteration kernel keeps M on chip: a pair slot is its two flow sets (4 planes, 33 MB at 1080p).  The
    // M-in-HBM kernels (a window the row-stream kernel is not built for: farn_stream_has_half; impl = 1;
    // DFX_VAR_FARN_M_IN_HBM) need the two M sets as well (14 planes).
    m_on_chip = p.impl == 0 && farn_stream_has_half(p.farn_win_size / 2) && !(p.variant & DFX_VAR_FARN_M_IN_HBM);
    for (auto &e : ev_it) {
        HIPCHK(c, hipEventCreateWithFlags(&e[0], dfx_event_flags(c, true)));
        HIPCHK(c, hipEventCreateWithFlags(&e[1], dfx_event_flags(c, true)));
    }
    return set_size(c->W, c->H);
}

size_t FarnebackEngine::device_bytes() const {
    return gker_cap + R_cap + f32_cap + tmpv_cap + pyr_cap + planes_cap + sizeof(int) * (size_t)slots.cap +
           sizeof(PairDesc) * (size_t)pairs.cap;
}

// Plan (engine_plan.h: host arithmetic) + ensure capacity.  Nothing of the engine changes before the last allocation has
// succeeded; the buffers a failed attempt has already grown stay grown.
int FarnebackEngine::set_size(int W, int H) {
    FarnPlan pl;
    farn_plan(pl, W, H, c->prm, m_on_chip ? (int)FARN_PL_M0 : (int)FARN_PL_COUNT);
    if (pl.bad_kernel)
        return dfx_fail(c, DFX_ERR_INVALID, "Farneback: bad Gaussian kernel size");
    if (pl.odd_level) { // refused before anything is allocated: the handle stays at the size it had
        char msg[256];
        snprintf(msg, sizeof msg,
                 "Farneback: farn_fast_pyramids needs even level sizes below the coarsest level (pyrUp doubles a size); "
                 "%d x %d accepts farn_num_levels up to %d",
                 W, H, pl.fast_max_levels);
        return dfx_fail(c, DFX_ERR_UNSUPPORTED, msg);
    }
    const size_t slot_bytes = (size_t)pl.slot_stride * sizeof(float);
    int nB = 0;
    if (const int rc = dfx_fit_pair_slots(mem, pl.batch, pl.per_pair, slot_bytes, device_bytes(), d_planes, planes_cap, B, nB))
        return rc;
    if (!dfx_grow_tables(mem, nB, pairs))
        return dfx_fail(c, DFX_ERR_HIP, "farn: allocating the pair descriptors failed");
    int rc = dfx_grow(mem, d_gker, gker_cap, sizeof(float) * pl.taps.size());
    if (rc == DFX_OK)
        rc = grow_frame_slots(nB + 1, pl.frame_elems, pl.plane_stride);
    if (rc != DFX_OK) { // the engine goes on at its old size, on the frame slots the buffers still hold
        dfx_settle_frame_slots(n_frame_slots, rc, slots_held());
        return rc;
    }
    // the context is idle: the taps of the previous size are no longer read
    if (!pl.taps.empty()) // a fast-pyramids handle has none
        HIPCHK(c, hipMemcpy(d_gker, pl.taps.data(), sizeof(float) * pl.taps.size(), hipMemcpyHostToDevice));
    nlev = pl.nlev;
    for (int k = 0; k < DFX_LVL_MAX; ++k) {
        const FarnPlanLevel &P = pl.lv[k];
        lv[k] = FLevel{FarnLevelGeom{P.w, P.h, P.pitch, P.r_off}, P.sigma, P.half, P.ker_off, P.ifx, P.ify};
    }
    frame_elems = pl.frame_elems;
    pitch0 = pl.pitch0;
    plane_stride = pl.plane_stride;
    slot_stride = pl.slot_stride;
    B = nB;
    dfx_settle_frame_slots(n_frame_slots, DFX_OK, slots_held());
    return DFX_OK;
}

// What a frame slot needs (engine_buffers.h), in the order it is allocated: `elems` floats of R and scratch planes of
// `plane` floats.
DfxSlotBufs FarnebackEngine::slot_bufs(long long elems, long long plane) {
    const size_t pb = (size_t)plane * sizeof(float);
    DfxSlotBufs s;
    s.add(d_R, R_cap, (size_t)elems * sizeof(float));
    if (!skip_zero_weights) // only the cross-check chain converts the frames to a float plane first
        s.add(d_f32, f32_cap, pb);
    s.add(d_tmpv, tmpv_cap, 2 * pb);
    s.add(d_pyr, pyr_cap, pb);
    return s;
}

int FarnebackEngine::grow_frame_slots(int need, long long elems, long long plane) {
    if (const int rc = dfx_grow_slot_bufs(mem, slot_bufs(elems, plane), need))
        return rc;
    if (!dfx_grow_tables(mem, need, slots))
        return dfx_fail(c, DFX_ERR_HIP, "farn: allocating the frame-slot tables failed");
    return DFX_OK;
}

int FarnebackEngine::ensure_frame_slots(int need) {
    if (need <= n_frame_slots)
        return DFX_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int rc = grow_frame_slots(need, frame_elems, plane_stride);
    // not dfx_settle_frame_slots: after a failure this engine counts whatever the buffers hold, which is more than it
    // counted before if an earlier set_size failed behind buffers it had already grown
    n_frame_slots = slots_held();
    return rc;
}

int FarnebackEngine::build_frames(const unsigned char *d_src, long long src_frame_stride, long long src_pitch, int n,
                                  const int *h_slots) {
    if (n <= 0)
        return DFX_OK;
    int *const d_frame_slots = slots.dev;
    slots.stage(h_slots, n);
    HIPCHK(c, hipMemcpyAsync(d_frame_slots, slots.host, slots.bytes(n), hipMemcpyHostToDevice, c->stream));
    const int W = c->W, H = c->H;
    if (fast_pyr) {
        // B.13, walking UP the pyramid: level 0 is the frame as float, level k one pyrDown of level k - 1.  The levels
        // alternate between d_pyr and the first plane of a frame's d_tmpv pair; level 1 reads the 8-bit frame itself.
        farn_launch_u8_to_f32(c->stream, d_src, src_frame_stride, src_pitch, n, d_pyr, plane_stride, W, H, pitch0);
        for (int k = 0; k < nlev; ++k) {
            const FLevel &L = lv[k];
            float *cur = (k & 1) ? d_tmpv : d_pyr;
            const long long cur_stride = (k & 1) ? plane_stride * 2 : plane_stride;
            if (k == 1)
                farn_launch_pyrdown_u8(c->stream, d_src, src_frame_stride, src_pitch, n, W, H, cur, cur_stride, L.g.pitch);
            else if (k > 1)
                farn_launch_pyrdown(c->stream, (k & 1) ? d_pyr : d_tmpv, (k & 1) ? plane_stride : plane_stride * 2,
                                    lv[k - 1].g.pitch, n, lv[k - 1].g.w, lv[k - 1].g.h, cur, cur_stride, L.g.pitch);
            farn_launch_polyexp(c->stream, cur, cur_stride, n, d_frame_slots, d_R, frame_elems, L.g, pc, polyexp_rows,
                                c->prm.farn_poly_n);
        }
        c->stats.kernel_launches += 2 * nlev; // u8 -> f32, nlev - 1 pyrDown, nlev expansions
        return DFX_OK;
    }
    // The vertical blur reads the 8-bit frames themselves unless the cross-check form is asked for
    // (DFX_VAR_FARN_EVAL_ZERO_TAPS: the round-1 chain with its separate convertTo pass; same bits either way).
    const bool from_u8 = skip_zero_weights != 0;
    if (!from_u8)
        farn_launch_u8_to_f32(c->stream, d_src, src_frame_stride, src_pitch, n, d_f32, plane_stride, W, H, pitch0);
    for (int k = nlev - 1; k >= 0; --k) {
        const FLevel &L = lv[k];
        if (from_u8)
            farn_launch_blur_v_u8(c->stream, d_src, src_frame_stride, src_pitch, n, W, H, pitch0, L.g.h, L.ify,
                                  d_gker + L.ker_off, L.half, d_tmpv, plane_stride * 2, skip_zero_weights);
        else
            farn_launch_blur_v(c->stream, d_f32, plane_stride, n, W, H, pitch0, L.g.h, L.ify, d_gker + L.ker_off, L.half,
                               d_tmpv, plane_stride * 2, skip_zero_weights);
        farn_launch_blur_h_resize(c->stream, d_tmpv, plane_stride * 2, n, W, H, pitch0, L.g.w, L.g.h, L.g.pitch, L.ifx,
                                  L.ify, d_gker + L.ker_off, L.half, d_pyr, plane_stride, skip_zero_weights);
        farn_launch_polyexp(c->stream, d_pyr, plane_stride, n, d_frame_slots, d_R, frame_elems, L.g, pc, polyexp_rows,
                            c->prm.farn_poly_n);
    }
    c->stats.kernel_launches += (from_u8 ? 0 : 1) + 3 * nlev;
    return DFX_OK;
}

int FarnebackEngine::run_pairs(int nb, const PairDesc *h_pairs, float *d_out, long long out_stride, const DfxPlanarOut *planar,
                               const DfxSeedIn *seed) {
    pairs.stage(h_pairs, nb);
    HIPCHK(c, hipMemcpyAsync(pairs.dev, pairs.host, pairs.bytes(nb), hipMemcpyHostToDevice, c->stream));
    const dfx_params &p = c->prm;
    const int half = p.farn_win_size / 2;
    const float box_inv = 1.f / (float)((1 + 2 * half) * (1 + 2 * half));
    const float up = (float)(1. / p.farn_pyr_scale);
    const FarnWinTaps *gauss = gauss_window ? &win_taps : nullptr; // nullptr: the box kernels, as before
    // A caller-supplied initial flow enters at the coarsest level k = nlev - 1 only: resize_linear(seed, w_k, h_k) times
    // (float)scale_k, scale_k the double that farneback_calc accumulates (pyrScale multiplied k times; 1 for one level).
    double seed_scale = 1.0;
    for (int k = 0; k < nlev - 1; ++k)
        seed_scale *= p.farn_pyr_scale;
    const FarnLevelGeom &T = lv[nlev - 1].g;
    const float seed_ifx = (float)(1.0 / ((double)T.w / (double)c->W)), seed_ify = (float)(1.0 / ((double)T.h / (double)c->H));
    seed_bytes_pair = seed ? 32.0 * T.w * T.h : 0.0; // four taps per pixel and channel
    FarnPairCtx x;
    std::memset(&x, 0, sizeof x);
    x.frame_R = d_R;
    x.frame_stride = frame_elems;
    x.planes = d_planes;
    x.plane_stride = plane_stride;
    x.slot_stride = slot_stride;
    x.pairs = pairs.dev;
    x.n_pairs = nb;
    // M recomputed inside the iteration kernel (round 4) unless the window is not one of the row-stream kernel's or a
    // cross-check form is asked for
    const bool fused = m_on_chip;
    if (fused) {
        // One launch per iteration and nothing else: the first iteration of a level up-samples the coarser level's flow
        // itself (zero at the coarsest), the last one of level 0 writes the caller's interleaved rows.  The flow
        // ping-pongs between its two plane sets; `cur` = the set the latest flow is in.
        int cur = 0;
        for (int k = nlev - 1; k >= 0; --k) {
            x.L = lv[k].g;
            const bool top = k == nlev - 1;
            const FarnLevelGeom P = top ? lv[k].g : lv[k + 1].g;
            const float ifx = top ? 0.f : (float)(1.0 / ((double)x.L.w / (double)P.w));
            const float ify = top ? 0.f : (float)(1.0 / ((double)x.L.h / (double)P.h));
            // fast pyramids: the coarser level's flow climbs by pyrUp into the other plane set, and the level's first
            // iteration is a plain launch (or the planar one) on it
            const bool climbed = fast_pyr && !top;
            if (climbed) {
                farn_launch_pyrup_flow(c->stream, x, cur, cur ^ 1, P.w, P.h, P.pitch, up);
                c->stats.kernel_launches += 1;
                cur ^= 1;
            }
            HIPCHK(c, hipEventRecord(ev_it[k][0], c->stream));
            for (int it = 0; it < p.farn_num_iters; ++it) {
                const bool last = k == 0 && it == p.farn_num_iters - 1;
                float *merged = last && !planar ? d_out : nullptr;
                if (seed && top && it == 0) {
                    // the seed is this launch's input flow; it may be the very buffer the flows go to, so a launch that
                    // is also the last one (one level, one iteration) leaves the caller's rows to the merge kernel
                    farn_launch_iter_stream_seed(c->stream, x, half, cur ^ 1, box_inv, nullptr, 0, *seed, c->W, c->H, seed_ifx, seed_ify,
                                                 (float)seed_scale, gauss);
                    if (last && !planar) {
                        farn_launch_merge(c->stream, x, cur ^ 1, d_out, out_stride);
                        c->stats.kernel_launches += 1;
                    }
                } else if (last && planar && (it > 0 || climbed))
                    farn_launch_iter_stream_planar(c->stream, x, half, cur, cur ^ 1, box_inv, *planar, gauss);
                else if (it == 0 && !climbed)
                    farn_launch_iter_stream_init(c->stream, x, half, cur, cur ^ 1, box_inv, merged, out_stride, P.w, P.h, P.pitch, ifx,
                                                 ify, up, top ? 1 : 0, gauss);
                else
                    farn_launch_iter_stream(c->stream, x, half, cur, cur ^ 1, box_inv, merged, out_stride, gauss);
                cur ^= 1;
            }
            HIPCHK(c, hipEventRecord(ev_it[k][1], c->stream));
            c->stats.kernel_launches += p.farn_num_iters;
        }
        // level 0's only iteration wrote plane set `cur` — unless it ran on a pyrUp'd flow, as the planar launch itself
        if (planar && p.farn_num_iters == 1 && !(fast_pyr && nlev > 1)) {
            farn_launch_merge_planar(c->stream, x, cur, *planar);
            c->stats.kernel_launches += 1;
        }
        return DFX_OK;
    }
    int set = (nlev - 1) & 1; // flow set the level's iterations run in (the previous level ended in the other one)
    for (int k = nlev - 1; k >= 0; --k) {
        x.L = lv[k].g;
        if (k == nlev - 1 && seed) {
            farn_launch_init_flow_seed(c->stream, x, set, *seed, c->W, c->H, seed_ifx, seed_ify, (float)seed_scale);
        } else if (k == nlev - 1) {
            farn_launch_init_flow(c->stream, x, set, 0, 0, 0, 0.f, 0.f, 0.f, 1);
        } else if (fast_pyr) {
            const FarnLevelGeom &P = lv[k + 1].g;
            farn_launch_pyrup_flow(c->stream, x, set ^ 1, set, P.w, P.h, P.pitch, up);
        } else {
            const FarnLevelGeom &P = lv[k + 1].g;
            const float ifx = (float)(1.0 / ((double)x.L.w / (double)P.w));
            const float ify = (float)(1.0 / ((double)x.L.h / (double)P.h));
            farn_launch_init_flow(c->stream, x, set, P.w, P.h, P.pitch, ifx, ify, up, 0); // reads set ^ 1
        }
        farn_launch_update_matrices(c->stream, x, set, 0);
        int m_src = 0;
        HIPCHK(c, hipEventRecord(ev_it[k][0], c->stream));
        for (int it = 0; it < p.farn_num_iters; ++it) {
            const int dm = it < p.farn_num_iters - 1;
            farn_launch_iteration(c->stream, x, set, m_src, half, box_inv, dm, c->prm.impl, gauss);
            if (dm)
                m_src ^= 1;
        }
        HIPCHK(c, hipEventRecord(ev_it[k][1], c->stream));
        c->stats.kernel_launches += 2 + p.farn_num_iters;
        set ^= 1; // the next (finer) level is initialised into the other set, from the one this level ended in
    }
    set ^= 1; // the set level 0 ended in
    if (planar)
        farn_launch_merge_planar(c->stream, x, set, *planar);
    else
        farn_launch_merge(c->stream, x, set, d_out, out_stride);
    c->stats.kernel_launches += 1;
    return DFX_OK;
}

// SURVEY.md §8d Farneback byte model, per pair as the reference executes it
int FarnebackEngine::account(int nb) {
    dfx_stats &st = c->stats;
    const dfx_params &p = c->prm;
    const double N0 = (double)c->W * c->H;
    double bytes = 34.0 * N0, it_bytes = 0;
    for (int k = 0; k < nlev; ++k) {
        const double Nk = (double)lv[k].g.w * lv[k].g.h;
        if (fast_pyr) // per frame: pyrDown reads the level below and writes this one (level 0 is the converted frame), + expansion
            bytes += 2.0 * ((k > 0 ? 4.0 * lv[k - 1].g.w * lv[k - 1].g.h + 4.0 * Nk : 0.0) + 24.0 * Nk);
        else
            bytes += 2.0 * (8.0 * N0 + 4.0 * std::min(N0, 4.0 * Nk) + 4.0 * Nk + 24.0 * Nk);
        bytes += 68.0 * Nk + 16.0 * Nk;
        const double itb = p.farn_num_iters * (40.0 + 28.0) * Nk + (p.farn_num_iters - 1) * 68.0 * Nk;
        bytes += itb;
        it_bytes += itb;
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev_it[k][0], ev_it[k][1]));
        st.step_ms += ms;
        st.level_ms[k] += ms;
        st.step_launches += (uint64_t)p.farn_num_iters;
        st.level_launches[k] += (uint64_t)p.farn_num_iters;
    }
    st.algorithmic_bytes += (bytes + seed_bytes_pair) * nb;
    st.step_algorithmic_bytes += it_bytes * nb;
    st.pairs += (uint64_t)nb;
    dfx_stats_levels(st, nlev, [&](int k) { return std::make_pair(lv[k].g.w, lv[k].g.h); });
    return DFX_OK;
}

} // namespace

AlgoEngine *dfx_make_farneback_engine(dfx_context *c) { return new FarnebackEngine(c); }
