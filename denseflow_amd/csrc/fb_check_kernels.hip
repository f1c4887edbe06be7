// fb_check_kernels.hip — the forward-backward consistency check of two flows on the device (Sundaram et al. 2010; the
// occlusion mask of UnFlow, Meister et al. 2018).
//
// Per pixel (x, y) of a forward flow F with the backward flow B of the same frame pair, all in float32, every operation
// rounded on its own (the build's -ffp-contract=off: no fused multiply-add anywhere below):
//     p = (x, y) + F(x, y);  outside [0, W-1] x [0, H-1] (NaN and inf included): occ = 1, err = +inf
//     s = B sampled bilinearly at p (x1 / y1 clamped to the last column / row)
//     err = |F + s|^2;  occ = err <= alpha1 * (|F|^2 + |s|^2) + alpha2 ? 0 : 1          (a NaN anywhere: 1)
// tests/fb_check_ref.py is the same text in NumPy; the two agree bit for bit.
//
// A streaming kernel with a gather on the lane quad of flow_quad.h (the F planes, the mask and err each one access per
// lane).  The B taps are plain global loads through fq_tap / fq_sample_f32: the displacement is unbounded, so there is no
// tile to stage.  No LDS, no scratch, at most 64 registers (eight waves per SIMD hide the gather's latency).
// Bytes per pixel and direction: 8 of F, 8 .. 32 of B (perfectly cached .. every tap its own sector), 1 of mask (+ 4 of err).
#include "fb_check_kernels.h"

#include <algorithm>

#include "dfx_device.h"
#include "flow_quad.h"

namespace {

// err of pixel (x, y) with flow (fu, fv); *occ its mask value
__device__ __forceinline__ float fb_check_px(float fu, float fv, int x, int y, const float *bu, const float *bv,
                                             long long pitch, int w, int h, float alpha1, float alpha2, unsigned *occ) {
    float err = INFINITY;
    *occ = 1u;
    const FqTap t = fq_tap((float)x + fu, (float)y + fv, w, h, FQ_BORDER_ZERO);
    if (t.inside) {
        const float su = fq_sample_f32(bu, pitch, t);
        const float sv = fq_sample_f32(bv, pitch, t);
        const float du = fu + su, dv = fv + sv;
        err = du * du + dv * dv;
        const float mag = (fu * fu + fv * fv) + (su * su + sv * sv);
        const float thr = alpha1 * mag + alpha2;
        *occ = err <= thr ? 0u : 1u; // a NaN compares false
    }
    return err;
}

// vec_f / vec_occ / vec_err: 4 where the bases and strides of the F planes / mask planes / err planes of every direction
// keep a lane's 4 pixels aligned to one access (fb_check_launch), 1 otherwise.  Wave-uniform.
__global__ __launch_bounds__(256, 8) void k_fb_check(FbCheckArgs a, int vec_f, int vec_occ, int vec_err) {
    const int x = fq_x(), y = fq_y();
    if (x >= a.w || y >= a.h)
        return;
    const int z = (int)blockIdx.z;
    const bool second = z >= a.n; // direction 1 of a two-direction launch; wave-uniform
    const long long i = second ? z - a.n : z;
    const float *fu = (second ? a.dir[1].f : a.dir[0].f) + i * a.flow_stride;
    const float *bu = (second ? a.dir[1].b : a.dir[0].b) + i * a.flow_stride;
    unsigned char *occ = (second ? a.dir[1].occ : a.dir[0].occ) + i * a.occ_stride + (long long)y * a.occ_pitch + x;
    float *err = second ? a.dir[1].err : a.dir[0].err;
    const float *bv = bu + a.plane_stride;
    const int n = fq_count(a.w, x);
    float u[4], v[4];
    fq_load_flow(fu + (long long)y * a.row_pitch + x, a.plane_stride, vec_f == 4, n, u, v);
    float e[4];
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e[k] = INFINITY, o[k] = 1u;
        if (k < n)
            e[k] = fb_check_px(u[k], v[k], x + k, y, bu, bv, a.row_pitch, a.w, a.h, a.alpha1, a.alpha2, &o[k]);
    }
    fq_store_u8(occ, vec_occ == 4, n, o);
    if (err)
        fq_store_f32(err + i * a.err_stride + (long long)y * a.err_pitch + x, vec_err == 4, n, e);
}

} // namespace

void fb_check_launch(hipStream_t s, const FbCheckArgs &args) {
    if (args.n <= 0 || args.w <= 0 || args.h <= 0)
        return;
    const int dirs = args.dirs == 2 ? 2 : 1;
    // a lane's 4 pixels in one access: every base and every stride of every direction a multiple of that access
    int vec_f = 4, vec_err = 4;
    unsigned long long occ_bits = (unsigned long long)args.occ_pitch | (unsigned long long)args.occ_stride;
    for (int d = 0; d < dirs; ++d) {
        vec_f = std::min(vec_f, dfx_planar_vec(args.dir[d].f, args.flow_stride, args.plane_stride, args.row_pitch));
        if (args.dir[d].err)
            vec_err = std::min(vec_err, dfx_planar_vec(args.dir[d].err, args.err_stride, 0, args.err_pitch));
        occ_bits |= (unsigned long long)(size_t)args.dir[d].occ;
    }
    const int vec_occ = (occ_bits & 3) == 0 ? 4 : 1;
    // grid.z holds at most FQ_ITEMS_MAX = 65535 planes: more flows than that go in several launches
    const int chunk = FQ_ITEMS_MAX / dirs;
    for (int i0 = 0; i0 < args.n; i0 += chunk) {
        FbCheckArgs a = args;
        a.dirs = dirs;
        a.n = std::min(chunk, args.n - i0);
        for (int d = 0; d < dirs; ++d) {
            a.dir[d].f += (long long)i0 * args.flow_stride;
            a.dir[d].b += (long long)i0 * args.flow_stride;
            a.dir[d].occ += (long long)i0 * args.occ_stride;
            if (a.dir[d].err)
                a.dir[d].err += (long long)i0 * args.err_stride;
        }
        hipLaunchKernelGGL(k_fb_check, fq_grid(a.w, a.h, a.n * dirs), dim3(256), 0, s, a, vec_f == 4 ? 4 : 1, vec_occ,
                           vec_err == 4 ? 4 : 1);
    }
}
