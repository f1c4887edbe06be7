// tests/colour_harness.cpp — C entry points over the host shell's colour stages (src/image_io.cpp) for the ctypes tests of
// the colour -s=0 path: the BGR JPEG encoder, the 3-channel resize and the .ppm reader.  Built by the `colour_harness`
// fixture of tests/test_jpeg_colour_pin.py against build/libzzdenseflow.a.
#include <cstring>

#include "image_io.h"

extern "C" {

// BGR frame (h rows of w * 3 bytes, dense) -> a JPEG file in out; returns its size, 0 on failure, -needed if cap is short
long long ch_encode_jpeg_bgr(const unsigned char *bgr, int w, int h, int quality, unsigned char *out, long long cap) {
    Mat m(Size(w, h), CV_8UC3);
    std::memcpy(m.data(), bgr, (size_t)w * h * 3);
    vector<uchar> file;
    if (!imencodeJpeg(m, file, quality))
        return 0;
    if ((long long)file.size() > cap)
        return -(long long)file.size();
    std::memcpy(out, file.data(), file.size());
    return (long long)file.size();
}

void ch_jpeg_force_portable(int on) { imencodeJpegForcePortable(on != 0); }

// cv::resize(INTER_LINEAR) of a dense BGR frame sw x sh -> dw x dh
void ch_resize_bgr(const unsigned char *src, int sw, int sh, unsigned char *dst, int dw, int dh) {
    Mat s(Size(sw, sh), CV_8UC3), d;
    std::memcpy(s.data(), src, (size_t)sw * sh * 3);
    resizeLinear(s, d, Size(dw, dh));
    std::memcpy(dst, d.data(), (size_t)dw * dh * 3);
}

// .ppm -> BGR into out (cap bytes); returns 1 and the size through w / h, 0 when the file is not a readable P6
int ch_imread_color(const char *file, unsigned char *out, long long cap, int *w, int *h) {
    Mat m;
    if (!imreadColor(file, m) || (long long)m.cols * m.rows * 3 > cap)
        return 0;
    *w = m.cols, *h = m.rows;
    std::memcpy(out, m.data(), (size_t)m.cols * m.rows * 3);
    return 1;
}
}
