// prepare_kernels.hip — frame preparation on the device.
//
// Replaces the two per-frame host steps of DenseFlow::load_frames_batch
// (/root/reference/src/denseflow_gpu.cpp:146-177): cvtColor(frame, gray, COLOR_BGR2GRAY) (:163) and
// cv::resize(gray, resized, size) with the default INTER_LINEAR (:169), so the loader thread only reads
// bytes and source-size frames cross PCIe once.  The arithmetic is OpenCV's 8-bit integer arithmetic
// (imgproc 4.5.2, not in the reference repository — parity unpinned, see oracle/prepare_oracle.h):
//   * BGR2GRAY: (B*3735 + G*19235 + R*9798 + 2^14) >> 15;
//   * resize INTER_LINEAR: source coordinate (float)((d + 0.5)*scale - 0.5), weights rounded to 11-bit
//     fixed point (x2048), horizontal pass in int, vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16),
//     +2 >> 2; an exact 2x2 decimation is what cv::resize turns into INTER_AREA: (a+b+c+d+2) >> 2.
// A colour source may also be R, G, B (COLOR_RGB2GRAY: the same sum with the outer weights exchanged) and channels-first
// (three byte planes): gray_at, a template on the format, reads the three bytes where the format puts them; everything behind
// it is unchanged, and the B, G, R interleaved instantiation is the kernel as it was.
// One thread per destination pixel; the four taps of a pixel are byte gathers served by L2 (a frame is
// read once per destination pixel, 1-3 B/px of source + 1 B/px written: HBM-bound, tiny next to the flow).
#include "prepare_kernels.h"

#include <algorithm>

#include "dfx_device.h"

namespace {

// gray value of pixel x of a row.  The source format is a template parameter, so that the B, G, R interleaved form stays the
// code it was: RGB (COLOR_RGB2GRAY) exchanges the outer weights, PLANAR reads the three bytes from byte planes `ch` bytes
// apart (row: the row of the first plane) instead of from one 3-byte pixel.
template <bool RGB, bool PLANAR> __device__ __forceinline__ int gray_at(const unsigned char *row, int x, int channels, long long ch) {
    if (channels == 1)
        return row[x];
    int c0, c1, c2;
    if (PLANAR) {
        c0 = row[x], c1 = row[x + ch], c2 = row[x + 2 * ch];
    } else {
        const unsigned char *p = row + 3 * x;
        c0 = p[0], c1 = p[1], c2 = p[2];
    }
    return ((RGB ? c2 : c0) * 3735 + c1 * 19235 + (RGB ? c0 : c2) * 9798 + (1 << 14)) >> 15;
}

// cv::resize's coefficient tables (resize.cpp, INTER_LINEAR, 8-bit): the source coordinate is evaluated in
// double and rounded to float, the weights are rounded to 11-bit fixed point (saturate_cast<short> = cvRound).
// The two axes treat the borders differently, as upstream does: along x an out-of-range index is clamped AND
// its fraction zeroed when the table is built; along y the table keeps the fraction and the row loop clamps
// the two row indices.
__device__ __forceinline__ void linear_coeff_x(int d, double scale, int ssize, int &s, int &w0, int &w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) {
        f = 0.f;
        s = 0;
    }
    if (s >= ssize - 1) {
        f = 0.f;
        s = ssize - 1;
    }
    w0 = (int)rintf((1.f - f) * 2048.f); // exact products: 11-bit scale
    w1 = (int)rintf(f * 2048.f);
}
__device__ __forceinline__ void linear_coeff_y(int d, double scale, int ssize, int &s0, int &s1, int &w0, int &w1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    s0 = min(max(s, 0), ssize - 1);
    s1 = min(max(s + 1, 0), ssize - 1);
    w0 = (int)rintf((1.f - f) * 2048.f);
    w1 = (int)rintf(f * 2048.f);
}

template <bool RGB, bool PLANAR>
__global__ __launch_bounds__(256) void k_prepare_frames(const unsigned char *src, long long src_pitch,
                                                         long long src_frame_stride, int sw, int sh, int channels,
                                                         long long ch, unsigned char *dst, long long dst_pitch,
                                                         long long dst_frame_stride, int dw, int dh, double scale_x,
                                                         double scale_y, int mode) {
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh)
        return;
    const unsigned char *S = src + (long long)blockIdx.z * src_frame_stride;
    unsigned char *D = dst + (long long)blockIdx.z * dst_frame_stride;
    auto gray = [&](const unsigned char *row, int x) { return gray_at<RGB, PLANAR>(row, x, channels, ch); };
    int out;
    if (mode == 0) { // same size: colour conversion only
        out = gray(S + (long long)dy * src_pitch, dx);
    } else if (mode == 1) { // exact 2x decimation: INTER_AREA fast path
        const unsigned char *r0 = S + (long long)(2 * dy) * src_pitch, *r1 = r0 + src_pitch;
        out = (gray(r0, 2 * dx) + gray(r0, 2 * dx + 1) + gray(r1, 2 * dx) + gray(r1, 2 * dx + 1) + 2) >> 2;
    } else {
        int sx, a0, a1, sy0, sy1, b0, b1;
        linear_coeff_x(dx, scale_x, sw, sx, a0, a1);
        linear_coeff_y(dy, scale_y, sh, sy0, sy1, b0, b1);
        const int sx1 = min(sx + 1, sw - 1); // weight 0 whenever this clamps
        const unsigned char *r0 = S + (long long)sy0 * src_pitch, *r1 = S + (long long)sy1 * src_pitch;
        const int h0 = gray(r0, sx) * a0 + gray(r0, sx1) * a1; // HResizeLinear, int
        const int h1 = gray(r1, sx) * a0 + gray(r1, sx1) * a1;
        out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2; // VResizeLinear<uchar, int, short>
    }
    D[(long long)dy * dst_pitch + dx] = (unsigned char)out;
}

// ---- the 3-channel form: cv::resize(bgr, resized, size) of the reference's colour frame extraction
// (/root/reference/src/denseflow_gpu.cpp:82-105, -s=0).  cv::resize treats the channels independently, so every channel
// goes through exactly the arithmetic above.  A row of interleaved BGR is 3 bytes per pixel: a pixel is fetched as the
// aligned dword(s) that hold it (one, or two when it straddles a dword boundary), not byte by byte.  The first dword
// always contains a byte of the pixel and the second is only touched when the pixel reaches into it, so no load leaves
// the row's own dwords.  One thread produces four destination pixels = 12 bytes, stored as three dwords where the
// destination row allows it.
__device__ __forceinline__ unsigned load_bgr(const unsigned char *row, int x) {
    const unsigned long long a = (unsigned long long)(row + 3 * (long long)x);
    const unsigned *p = reinterpret_cast<const unsigned *>(a & ~3ull);
    const unsigned sh = (unsigned)(a & 3ull) * 8u;
    unsigned v = p[0] >> sh;
    if (sh > 8u)
        v |= p[1] << (32u - sh);
    return v & 0xFFFFFFu;
}

__global__ __launch_bounds__(256) void k_prepare_bgr(const unsigned char *src, long long src_pitch, long long src_frame_stride,
                                                      int sw, int sh, unsigned char *dst, long long dst_pitch,
                                                      long long dst_frame_stride, int dw, int dh, double scale_x,
                                                      double scale_y, int mode) {
    const int gx = blockIdx.x * 64 + (threadIdx.x & 63); // group of four destination pixels
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (gx * 4 >= dw || dy >= dh)
        return;
    const unsigned char *S = src + (long long)blockIdx.z * src_frame_stride;
    unsigned char *D = dst + (long long)blockIdx.z * dst_frame_stride + (long long)dy * dst_pitch + 12ll * gx;
    unsigned out[4] = {0u, 0u, 0u, 0u}; // packed B | G << 8 | R << 16
    int sy0 = 0, sy1 = 0, b0 = 0, b1 = 0;
    if (mode == 2)
        linear_coeff_y(dy, scale_y, sh, sy0, sy1, b0, b1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int dx = gx * 4 + i;
        if (dx >= dw)
            break;
        if (mode == 0) {
            out[i] = load_bgr(S + (long long)dy * src_pitch, dx);
        } else if (mode == 1) {
            const unsigned char *r0 = S + (long long)(2 * dy) * src_pitch, *r1 = r0 + src_pitch;
            const unsigned p00 = load_bgr(r0, 2 * dx), p01 = load_bgr(r0, 2 * dx + 1), p10 = load_bgr(r1, 2 * dx),
                           p11 = load_bgr(r1, 2 * dx + 1);
#pragma unroll
            for (int c = 0; c < 24; c += 8)
                out[i] |= ((((p00 >> c) & 255u) + ((p01 >> c) & 255u) + ((p10 >> c) & 255u) + ((p11 >> c) & 255u) + 2u) >> 2) << c;
        } else {
            int sx, a0, a1;
            linear_coeff_x(dx, scale_x, sw, sx, a0, a1);
            const int sx1 = min(sx + 1, sw - 1); // weight 0 whenever this clamps
            const unsigned char *r0 = S + (long long)sy0 * src_pitch, *r1 = S + (long long)sy1 * src_pitch;
            const unsigned p00 = load_bgr(r0, sx), p01 = load_bgr(r0, sx1), p10 = load_bgr(r1, sx), p11 = load_bgr(r1, sx1);
#pragma unroll
            for (int c = 0; c < 24; c += 8) {
                const int h0 = (int)((p00 >> c) & 255u) * a0 + (int)((p01 >> c) & 255u) * a1; // HResizeLinear, int
                const int h1 = (int)((p10 >> c) & 255u) * a0 + (int)((p11 >> c) & 255u) * a1;
                out[i] |= (unsigned)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2) << c;
            }
        }
    }
    if (gx * 4 + 4 <= dw && ((unsigned long long)D & 3ull) == 0) {
        unsigned *W = reinterpret_cast<unsigned *>(D);
        W[0] = out[0] | (out[1] << 24);
        W[1] = (out[1] >> 8) | (out[2] << 16);
        W[2] = (out[2] >> 16) | (out[3] << 8);
    } else {
        for (int i = 0; i < 4 && gx * 4 + i < dw; ++i) {
            D[3 * i] = (unsigned char)out[i];
            D[3 * i + 1] = (unsigned char)(out[i] >> 8);
            D[3 * i + 2] = (unsigned char)(out[i] >> 16);
        }
    }
}

} // namespace

int prepare_mode(int sw, int sh, int dw, int dh) {
    if (sw == dw && sh == dh)
        return 0;
    if (sw == 2 * dw && sh == 2 * dh)
        return 1;
    return 2;
}

void prepare_launch(hipStream_t s, const unsigned char *d_src, long long src_pitch, long long src_frame_stride, int sw,
                    int sh, int channels, int n, unsigned char *d_dst, long long dst_pitch, long long dst_frame_stride,
                    int dw, int dh, int rgb, int planar, long long plane_stride) {
    if (n <= 0)
        return;
    // cv::resize: inv_scale = dsize / ssize (double), scale = 1 / inv_scale
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    const int mode = prepare_mode(sw, sh, dw, dh);
    const bool swap = channels == 3 && rgb, pl = channels == 3 && planar;
    const long long ch = pl ? (plane_stride ? plane_stride : src_pitch * sh) : 1;
    auto k = pl ? (swap ? k_prepare_frames<true, true> : k_prepare_frames<false, true>)
                : (swap ? k_prepare_frames<true, false> : k_prepare_frames<false, false>);
    // grid.z holds at most DFX_GRID_YZ_MAX frames: more than that go in several launches
    const int chunk = DFX_GRID_YZ_MAX;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const dim3 grid((dw + 63) / 64, (dh + 3) / 4, std::min(chunk, n - i0));
        hipLaunchKernelGGL(k, grid, dim3(256), 0, s, d_src + i0 * src_frame_stride, src_pitch, src_frame_stride, sw, sh, channels,
                           ch, d_dst + i0 * dst_frame_stride, dst_pitch, dst_frame_stride, dw, dh, scale_x, scale_y, mode);
    }
}

void prepare_bgr_launch(hipStream_t s, const unsigned char *d_src, long long src_pitch, long long src_frame_stride, int sw,
                        int sh, int n, unsigned char *d_dst, long long dst_pitch, long long dst_frame_stride, int dw,
                        int dh) {
    if (n <= 0)
        return;
    const double scale_x = 1.0 / ((double)dw / (double)sw), scale_y = 1.0 / ((double)dh / (double)sh);
    const int chunk = DFX_GRID_YZ_MAX; // as in prepare_launch
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const dim3 grid(((dw + 3) / 4 + 63) / 64, (dh + 3) / 4, std::min(chunk, n - i0));
        hipLaunchKernelGGL(k_prepare_bgr, grid, dim3(256), 0, s, d_src + i0 * src_frame_stride, src_pitch, src_frame_stride, sw, sh,
                           d_dst + i0 * dst_frame_stride, dst_pitch, dst_frame_stride, dw, dh, scale_x, scale_y,
                           prepare_mode(sw, sh, dw, dh));
    }
}
