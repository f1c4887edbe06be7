// farn_fastpyr_plan_harness.cpp — TEST INFRASTRUCTURE: the Farneback plan (farn_plan, denseflow_amd/csrc/engine_plan.h: the
// host arithmetic FarnebackEngine::create and set_size run) with dfx_params.farn_fast_pyramids behind a C entry point, for
// tests/test_farneback_fastpyr_ref.py: the level sizes of the (n + 1) / 2 chain and the odd-level refusal.
#include "../denseflow_amd/csrc/engine_plan.h"

// Returns 1 where the plan reports an odd level below the coarsest (the engine refuses the size), 0 otherwise.
// w16 / h16: the sizes of levels 0 .. *nlev - 1; *max_levels: the largest farn_num_levels the size accepts (fast only);
// *n_taps: Gaussian pre-blur taps the plan holds.
extern "C" int ffp_plan(int W, int H, int num_levels, int fast, int *nlev, int *w16, int *h16, int *max_levels, int *n_taps) {
    dfx_params p{};
    p.farn_num_levels = num_levels;
    p.farn_pyr_scale = 0.5;
    p.farn_win_size = 13;
    p.farn_num_iters = 10;
    p.farn_poly_n = 5;
    p.farn_poly_sigma = 1.1;
    p.farn_fast_pyramids = fast;
    FarnPlan pl;
    farn_plan(pl, W, H, p, 4);
    *nlev = pl.nlev;
    for (int k = 0; k < 16; ++k)
        w16[k] = pl.lv[k].w, h16[k] = pl.lv[k].h;
    *max_levels = pl.fast_max_levels;
    *n_taps = (int)pl.taps.size();
    return pl.odd_level ? 1 : 0;
}
