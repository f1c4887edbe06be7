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
// A streaming kernel with a gather: 4 neighbouring pixels of a row per lane (one 16-byte load per F plane, one 4-byte mask
// store, one 16-byte err store where bases and strides keep that alignment; scalar accesses otherwise and at the ragged
// right edge), a wave covers 1 KB of a row per plane.  The B taps are plain global loads: the displacement is unbounded, so
// there is no tile to stage.  No LDS, no scratch, at most 64 registers (eight waves per SIMD hide the gather's latency).
// Bytes per pixel and direction: 8 of F, 8 .. 32 of B (perfectly cached .. every tap its own sector), 1 of mask (+ 4 of err).
#include "fb_check_kernels.h"

#include <algorithm>

#include "dfx_device.h"

namespace {

// bilinear sample of a plane at the four taps of an inside position (r0 / r1: element offsets of rows y0 / y1)
__device__ __forceinline__ float fb_sample(const float *p, long long r0, long long r1, int x0, int x1, float ax, float ay) {
    const float p00 = p[r0 + x0], p01 = p[r0 + x1], p10 = p[r1 + x0], p11 = p[r1 + x1];
    const float t = p00 + ax * (p01 - p00);
    const float b = p10 + ax * (p11 - p10);
    return t + ay * (b - t);
}

// err of pixel (x, y) with flow (fu, fv); *occ its mask value
__device__ __forceinline__ float fb_check_px(float fu, float fv, int x, int y, const float *bu, const float *bv,
                                             long long pitch, int w, int h, float alpha1, float alpha2, unsigned *occ) {
    float err = INFINITY;
    *occ = 1u;
    const float px = (float)x + fu, py = (float)y + fv;
    // the range test comes before any conversion to int: false for NaN and for either infinity
    if (px >= 0.0f && py >= 0.0f && px <= (float)(w - 1) && py <= (float)(h - 1)) {
        const float fx = floorf(px), fy = floorf(py);
        const int x0 = (int)fx, y0 = (int)fy;
        const float ax = px - fx, ay = py - fy;
        const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
        const long long r0 = (long long)y0 * pitch, r1 = (long long)y1 * pitch;
        const float su = fb_sample(bu, r0, r1, x0, x1, ax, ay);
        const float sv = fb_sample(bv, r0, r1, x0, x1, ax, ay);
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
    const int x = ((int)blockIdx.x * 64 + ((int)threadIdx.x & 63)) * 4;
    const int y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6);
    if (x >= a.w || y >= a.h)
        return;
    const int z = (int)blockIdx.z;
    const bool second = z >= a.n; // direction 1 of a two-direction launch; wave-uniform
    const long long i = second ? z - a.n : z;
    const float *fu = (second ? a.dir[1].f : a.dir[0].f) + i * a.flow_stride;
    const float *bu = (second ? a.dir[1].b : a.dir[0].b) + i * a.flow_stride;
    unsigned char *occ = (second ? a.dir[1].occ : a.dir[0].occ) + i * a.occ_stride + (long long)y * a.occ_pitch + x;
    float *err = second ? a.dir[1].err : a.dir[0].err;
    const float *fv = fu + a.plane_stride, *bv = bu + a.plane_stride;
    const long long at = (long long)y * a.row_pitch + x;
    const int n = min(4, a.w - x);
    float u[4], v[4];
    if (vec_f == 4 && n == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(fu + at);
        const float4 s = *reinterpret_cast<const float4 *>(fv + at);
        u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
        v[0] = s.x, v[1] = s.y, v[2] = s.z, v[3] = s.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            u[k] = k < n ? fu[at + k] : 0.0f;
            v[k] = k < n ? fv[at + k] : 0.0f;
        }
    }
    float e[4];
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e[k] = INFINITY, o[k] = 1u;
        if (k < n)
            e[k] = fb_check_px(u[k], v[k], x + k, y, bu, bv, a.row_pitch, a.w, a.h, a.alpha1, a.alpha2, &o[k]);
    }
    if (vec_occ == 4 && n == 4) {
        *reinterpret_cast<unsigned *>(occ) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n)
                occ[k] = (unsigned char)o[k];
    }
    if (err) {
        float *d = err + i * a.err_stride + (long long)y * a.err_pitch + x;
        if (vec_err == 4 && n == 4) {
            *reinterpret_cast<float4 *>(d) = make_float4(e[0], e[1], e[2], e[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n)
                    d[k] = e[k];
        }
    }
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
    // grid.z holds at most 65535 planes: more flows than that go in several launches
    const int chunk = 65535 / dirs;
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
        const dim3 grid((unsigned)((a.w + 255) / 256), (unsigned)((a.h + 3) / 4), (unsigned)(a.n * dirs));
        hipLaunchKernelGGL(k_fb_check, grid, dim3(256), 0, s, a, vec_f == 4 ? 4 : 1, vec_occ, vec_err == 4 ? 4 : 1);
    }
}
