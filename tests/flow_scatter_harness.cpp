// tests/flow_scatter_harness.cpp — the integer scatter of the flow projection and the splat (denseflow_amd/csrc/flow_scatter.h:
// fs_landing, fs_taps, fs_add, fs_window, fs_window_clear, fs_window_flush) compiled as plain C++ with -ffp-contract=off, the very
// text the kernels compile, run serially: tile after tile in the kernels' 32 x 8 order, lane after lane, the add a plain +=.
// Once with every tap going straight to the workspace and once through a window array, with the header's own origin, in-window
// test and flush.  A stand-alone program, so that it also runs under -fsanitize=undefined,address with no preload: the float to
// int casts and the window and workspace indices (both are heap blocks of exactly their size) are what the sanitizers guard.
// Driven by tests/test_flow_scatter_cpu.py.  The payload rules are the kernel files' own: the projection's quantisation of
// the flow is restated here in one line, the splat's payload arrives as the integers tests/splat_ref.py's payload() made of it.
//
// argv[1 ..]: text files, one case each, of
//         w h t(float32 bits, hex) channels has_imp has_occ     channels 0: the projection, WORDS = 3; 1 .. 4: a splat payload
//         2 * w * h float32 bit patterns (8 hex digits each, nothing between them): the u and the v plane
//         has_imp: w * h float32 bit patterns likewise;  has_occ: w * h bytes (decimal)
//         channels > 0: w * h flags (the pixel's payload is taken), then channels * w * h integers (decimal): q, planar
// stdout: per case two lines of w * h * WORDS words (16 hex digits each, nothing between them): the workspace of the global
//         form, then that of the window form; and a line with the count of non-zero words the windows held at their flushes
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../denseflow_amd/csrc/flow_scatter.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// in_window: the non-zero words the windows held when they were flushed, over all tiles
template <int WORDS, bool WINDOW, typename Payload>
static std::vector<fs_u64> scatter(const FsSource &a, Payload payload, long long *in_window) {
    std::vector<fs_u64> work((size_t)a.w * a.h * WORDS, 0ull), win((size_t)fs_window_words(WORDS));
    for (int by = 0; by < (a.h + FS_TH - 1) / FS_TH; ++by) {
        for (int bx = 0; bx < (a.w + FS_TW - 1) / FS_TW; ++bx) {
            FsWindow o = {win.data(), 0, 0};
            if (WINDOW) {
                fs_window_clear<WORDS>(win.data(), 0, 1);
                o = fs_window(win.data(), a, 0, bx, by);
            }
            for (int lane = 0; lane < FS_THREADS; ++lane) {
                const int x = bx * FS_TW + lane % FS_TW, y = by * FS_TH + lane / FS_TW;
                const FsLanding l = fs_landing(a, 0, x, y, a.imp != nullptr, a.occ != nullptr);
                int q[WORDS - 1];
                if (l.live && payload(l, x, y, q))
                    fs_taps(l, a.w, a.h, [&](int tx, int ty, fs_u64 wt) { fs_add<WORDS, WINDOW>(o, work.data(), a.w, tx, ty, wt, q); });
            }
            if (WINDOW) {
                for (fs_u64 v : win)
                    *in_window += v != 0ull;
                fs_window_flush<WORDS>(o, work.data(), a.w, a.h, 0, 1);
            }
        }
    }
    return work;
}

template <int WORDS, typename Payload>
static void both(const FsSource &a, Payload payload) {
    long long in_window = 0;
    const std::vector<fs_u64> forms[2] = {scatter<WORDS, false>(a, payload, &in_window), scatter<WORDS, true>(a, payload, &in_window)};
    for (const std::vector<fs_u64> &work : forms) {
        for (fs_u64 v : work)
            std::printf("%016llx", v);
        std::printf("\n");
    }
    std::printf("%lld\n", in_window);
}

template <int C>
static void splat(const FsSource &a, const std::vector<int> &ok, const std::vector<int> &q_planes) {
    const size_t hw = (size_t)a.w * a.h;
    both<1 + C>(a, [&](const FsLanding &, int x, int y, int (&q)[C]) {
        for (int c = 0; c < C; ++c)
            q[c] = q_planes[c * hw + (size_t)y * a.w + x];
        return ok[(size_t)y * a.w + x] != 0;
    });
}

static int run(const char *path) {
    FILE *in = std::fopen(path, "r");
    int w, h, channels, has_imp, has_occ;
    unsigned tb;
    if (!in || std::fscanf(in, "%d %d %x %d %d %d", &w, &h, &tb, &channels, &has_imp, &has_occ) != 6 || w <= 0 || h <= 0 ||
        channels < 0 || channels > 4)
        return 2;
    const size_t hw = (size_t)w * h;
    std::vector<float> flow(2 * hw), imp(has_imp ? hw : 0);
    std::vector<unsigned char> occ(has_occ ? hw : 0);
    std::vector<int> ok(channels ? hw : 0), q_planes(channels * hw);
    unsigned b;
    for (float &v : flow)
        v = std::fscanf(in, "%8x", &b) == 1 ? from_bits(b) : 0.0f;
    for (float &v : imp)
        v = std::fscanf(in, "%8x", &b) == 1 ? from_bits(b) : 0.0f;
    for (unsigned char &v : occ)
        v = std::fscanf(in, "%u", &b) == 1 ? (unsigned char)b : 0;
    for (int &v : ok)
        if (std::fscanf(in, "%d", &v) != 1)
            return 2;
    for (int &v : q_planes)
        if (std::fscanf(in, "%d", &v) != 1)
            return 2;
    std::fclose(in);
    FsSource a{};
    a.flow = flow.data(), a.imp = has_imp ? imp.data() : nullptr, a.occ = has_occ ? occ.data() : nullptr;
    a.n = 1, a.w = w, a.h = h, a.t = from_bits(tb);
    a.row_pitch = w, a.plane_stride = (long long)hw, a.imp_pitch = w, a.occ_pitch = w;
    if (channels == 0) // flow_project_kernels.hip: q = (int)rintf(fminf(fmaxf(f * 256.f, -8388608.f), 8388608.f))
        both<3>(a, [](const FsLanding &l, int, int, int (&q)[2]) {
            q[0] = (int)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(l.fu * 256.0f, -8388608.0f), 8388608.0f));
            q[1] = (int)__builtin_rintf(__builtin_fminf(__builtin_fmaxf(l.fv * 256.0f, -8388608.0f), 8388608.0f));
            return true;
        });
    else if (channels == 1)
        splat<1>(a, ok, q_planes);
    else if (channels == 2)
        splat<2>(a, ok, q_planes);
    else if (channels == 3)
        splat<3>(a, ok, q_planes);
    else
        splat<4>(a, ok, q_planes);
    return 0;
}

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i)
        if (int e = run(argv[i]))
            return e;
    return 0;
}
