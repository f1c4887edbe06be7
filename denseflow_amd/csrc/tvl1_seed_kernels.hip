// tvl1_seed_kernels.hip — a caller-supplied initial flow on its way to the coarsest level of the -a=tvl1 pyramid
// (upstream: the useInitialFlow_ branch of cv::cuda::OpticalFlowDual_TVL1::calc; SURVEY.md Appendix A "initial flow",
// rated MED).  The seed is u1[0], u2[0]; level s is resize_linear(level s - 1, w_s, h_s, ifx, ify) * (float)scaleStep,
// every level rounded to float before the next one reads it; the coarsest one replaces the zeros the solver starts from.
//
// One launch per pyramid step, 64 x 4 pixels per workgroup as k_tvl1_upsample_u.  The first launch reads the caller's own
// rows — interleaved (u, v) or two planes, DfxSeedIn — so no full-resolution de-interleaved copy exists when the pyramid
// has more than one level; later launches ping-pong between the two u plane sets of the pair slot, which nothing else
// uses before the coarsest level begins.  The engine picks the sets so that the chain ends in set 0, where
// k_tvl1_level_begin(first_level) puts `cur`.  A one-level pyramid copies the seed as it is.
// Compiled with -ffp-contract=off (see tvl1_math.h).
#include <hip/hip_runtime.h>

#include "dfx_device.h"
#include "tvl1_device_common.h"
#include "tvl1_kernels.h"

// `c` describes the DESTINATION level; the source — the caller's seed, or the u planes of the finer level — is `q.src`
// with geometry q.sw x q.sh.  Writes u1 / u2 of plane set q.dst_set.
__global__ __launch_bounds__(256) void k_tvl1_seed_step(Tvl1LevelCtx c, Tvl1SeedStep q) {
    const DfxBlockXY blk = dfx_block_xy(); // XCD-aware (dfx_device.h): neighbouring rows share one L2
    const int x = blk.x * 64 + (threadIdx.x & 63);
    const int y = blk.y * 4 + (threadIdx.x >> 6);
    if (x >= c.w || y >= c.h)
        return;
    const int b = blockIdx.z;
    const long long o = (long long)y * c.pitch + x;
    const long long pb = (long long)b * q.src.pair_stride;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float *src = (k ? q.src.v : q.src.u) + pb;
        float *dst = pair_plane(c, b, PL_U1_0 + 2 * q.dst_set + k);
        if (q.copy)
            dst[o] = src[(long long)y * q.src.row_pitch + (long long)x * q.src.step];
        else
            dst[o] = dfx_seed_resize_px(src, q.sw, q.sh, q.src.row_pitch, q.src.step, x, y, q.ifx, q.ify) * q.mul;
    }
}

void tvl1_launch_seed_step(hipStream_t s, const Tvl1LevelCtx &c_dst, const Tvl1SeedStep &q) {
    const dim3 grid((c_dst.w + 63) / 64, (c_dst.h + 3) / 4, c_dst.n_pairs);
    hipLaunchKernelGGL(k_tvl1_seed_step, grid, dim3(256), 0, s, c_dst, q);
}

// The u planes of set `set` of pair slot 0 as a seed source (level pitch `pitch`): what a later step of the chain reads.
DfxSeedIn tvl1_seed_from_planes(const Tvl1LevelCtx &c, int set, int pitch) {
    DfxSeedIn in;
    in.u = c.planes + (long long)(PL_U1_0 + 2 * set) * c.plane_stride;
    in.v = c.planes + (long long)(PL_U2_0 + 2 * set) * c.plane_stride;
    in.step = 1;
    in.row_pitch = pitch;
    in.pair_stride = c.slot_stride;
    return in;
}
