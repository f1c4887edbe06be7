// tests/tvl1_gamma_plan_harness.cpp — TEST INFRASTRUCTURE: the TVL1 plan (tvl1_plan, denseflow_amd/csrc/engine_plan.h: the
// host arithmetic Tvl1Engine::create and set_size run) with a given tvl1_gamma behind a C entry point, for
// tests/test_tvl1_gamma_ref.py: the plane count of a pair slot and the 32-bit offset rule that follows it.
#include "../denseflow_amd/csrc/engine_plan.h"

extern "C" {
// out = {n_planes, plane_stride, slot_stride, slot_too_large, per_pair}
void gp_tvl1(int w, int h, double gamma, long long *out) {
    dfx_params p{};
    p.tvl1_nscales = 5, p.tvl1_scale_step = 0.8;
    p.tvl1_gamma = gamma;
    Tvl1Plan pl;
    tvl1_plan(pl, w, h, p);
    out[0] = pl.n_planes, out[1] = pl.plane_stride, out[2] = pl.slot_stride, out[3] = pl.slot_too_large;
    out[4] = (long long)pl.per_pair;
}
}
