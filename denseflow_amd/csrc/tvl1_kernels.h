// tvl1_kernels.h — host-callable launchers of the TVL1 kernels (defined in tvl1_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "dfx_device.h"

void tvl1_launch_u8_to_f32(hipStream_t s, const unsigned char *src, long long src_frame_stride, long long src_pitch,
                           const int *frame_slots, int n_frames, float *dst, long long dst_frame_stride, int w, int h,
                           int pitch);
void tvl1_launch_pyr_down(hipStream_t s, float *frame_I, long long frame_stride, const int *frame_slots, int n_frames,
                          long long src_off, int sw, int sh, int spitch, long long dst_off, int dw, int dh, int dpitch,
                          float ifx, float ify);
void tvl1_launch_centered_gradient(hipStream_t s, const float *frame_I, float *frame_Ix, float *frame_Iy,
                                   long long frame_stride, const int *frame_slots, int n_frames, long long off, int w,
                                   int h, int pitch);
void tvl1_launch_level_begin(hipStream_t s, const Tvl1LevelCtx &c, int first_level);
// A caller-supplied initial flow (tvl1_seed_kernels.hip): one step of the chain that carries it to the coarsest level.
// The launch's context describes the destination level; u1 / u2 of plane set dst_set = resize_linear(src, ifx, ify) * mul,
// or (copy: a one-level pyramid) the source as it is.
struct Tvl1SeedStep {
    DfxSeedIn src; // the caller's seed (first step) or the finer level's u planes (tvl1_seed_from_planes)
    int sw, sh;    // geometry of the source
    int dst_set;
    float ifx, ify, mul;
    int copy;
};
void tvl1_launch_seed_step(hipStream_t s, const Tvl1LevelCtx &c_dst, const Tvl1SeedStep &q);
DfxSeedIn tvl1_seed_from_planes(const Tvl1LevelCtx &c, int set, int pitch);
// tvl1_launch_level_begin of the coarsest level when the seed chain has left u in plane set 0: the state machine is armed
// on that set and u is not zeroed (p is, unless the warp-and-head kernel takes it as zero)
void tvl1_launch_level_begin_seeded(hipStream_t s, const Tvl1LevelCtx &c);
void tvl1_launch_warp(hipStream_t s, const Tvl1LevelCtx &c, int step_id); // dedicated backward-warp kernel of a step
// the warp AND the head of the loop it starts (tvl1_head_kernels.hip), in place of tvl1_launch_warp
// (regs: its register form of round 6, DFX_VAR_TVL1_HEAD_NBR_LDS)
void tvl1_launch_warp_head(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int math, bool regs);
int tvl1_head_blocks(const Tvl1LevelCtx &c); // workgroups per pair of that launch
void tvl1_launch_step(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int impl, int math, bool nbr_lds);
int tvl1_step_blocks(const Tvl1LevelCtx &c, int impl); // workgroups per pair of a step launch
int tvl1_fused_max_k();                                // largest supported inner-iteration fusion
void tvl1_launch_upsample_u(hipStream_t s, const Tvl1LevelCtx &c_src, int dw, int dh, int dpitch, float ifx, float ify,
                            float up);
void tvl1_launch_merge(hipStream_t s, const Tvl1LevelCtx &c0, float *out, long long out_stride);
void tvl1_launch_merge_planar(hipStream_t s, const Tvl1LevelCtx &c0, const DfxPlanarOut &o); // u and v planes, bounded
// the illumination channel (dfx_params.tvl1_gamma != 0): p31 = p32 = 0 (and u3 = 0 at the coarsest level) behind
// tvl1_launch_level_begin; the step with the third channel (impl 0: fused tile kernel behind tvl1_launch_warp, 1: simple
// kernel); u3's upsample (factor 1) beside tvl1_launch_upsample_u
void tvl1_launch_level_begin_gamma(hipStream_t s, const Tvl1LevelCtx &c, int first_level);
void tvl1_launch_step_gamma(hipStream_t s, const Tvl1LevelCtx &c, int step_id, int impl);
void tvl1_launch_upsample_u3(hipStream_t s, const Tvl1LevelCtx &c_src, int dw, int dh, int dpitch, float ifx, float ify);
