// jpeg_kernels.h — baseline JPEG encoding of bounded flow planes on the device (jpeg_kernels.hip) and the host-side
// assembly of the files (jpeg_host.cpp).  SURVEY.md §8f-1: replaces the two imencode(".jpg") per flow of encodeFlowMap
// (/root/reference/src/common.cpp:56-57).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

struct JpegTables { // one per (handle, quality), in device memory
    unsigned div[64];   // 8 q: the divisor of libjpeg's quantisation (include/dfx_jpeg_tables.h), natural order
    unsigned magic[64]; // dfx_jpeg_divide_magic(div)
    unsigned short dc_code[12];
    unsigned char dc_len[12];
    unsigned short ac_code[256];
    unsigned char ac_len[256];
    unsigned char nat2zig[64]; // zig-zag position of natural-order coefficient i
};

// What the device reports to the host after a batch (page-locked, mapped: written by k_jpeg_layout with system-scope
// stores, read by the host after the stream is synchronised).
struct JpegInfo {
    unsigned long long total_bytes; // bytes of the batch's streams in the shared buffer (each plane 4-byte aligned)
    unsigned long long overflow;    // != 0: the streams did not fit the shared buffer; nothing was written
    // followed by n_planes x { unsigned long long bits, base_byte }
};

struct JpegCtx {
    const unsigned char *planes; // plane p: planes + (p < n_x ? p : y_first + p - n_x) * plane_stride
    long long plane_stride;
    int pitch, w, h, bw, bh;
    int n_planes, n_x, y_first;   // planes 0..n_x-1 are consecutive, the other n_planes - n_x start at index y_first
    const JpegTables *tab;
    short *dc;                    // [n_planes][bw * bh] quantised DC of every block
    unsigned *bits;               // [n_planes][bw * bh] AC bits of every block, then its exclusive bit offset
    unsigned long long *plane_bits; // [n_planes] bits of each plane's entropy-coded segment (before stuffing)
    unsigned long long *plane_base; // [n_planes] first byte of each plane's stream in `stream`
    unsigned *stream;             // shared output buffer, zeroed before the emit pass
    unsigned long long capacity_bytes;
    unsigned long long *info;     // JpegInfo + per-plane entries (device view of the page-locked block); written once
    unsigned long long *hdr;      // device copy of {total_bytes, overflow} for the zero-fill and emit passes
};

// Enqueue the whole encode of a batch on stream s: count pass, scans, layout, zero-fill, emit pass.
void jpeg_launch_encode(hipStream_t s, const JpegCtx &c);

// The colour form (jpeg_colour_kernels.hip): n_planes BGR frames -> one YCbCr 4:2:0 interleaved stream each, what
// cv::imencode(".jpg", bgr) codes (reference src/denseflow_gpu.cpp:82-105, the -s=0 mode).  A frame's blocks are numbered
// in MCU order (Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 MCU, MCUs row-major); the other fields mean what they mean in JpegCtx,
// with "plane" = frame.  The rows are read as dwords: the first frame is 4-byte aligned, pitch and frame_stride are
// multiples of 4.
struct JpegColourCtx {
    const unsigned char *bgr; // frame f: bgr + f * frame_stride, rows of w interleaved B G R pixels, pitch bytes apart
    long long frame_stride;
    int pitch, w, h, mcus_x, mcus_y;
    int n_planes;
    const JpegTables *tab; // [0] luminance, [1] chrominance
    short *dc;             // [n_planes][mcus_x * mcus_y * 6]
    unsigned *bits;
    unsigned long long *plane_bits, *plane_base;
    unsigned *stream;
    unsigned long long capacity_bytes;
    unsigned long long *info, *hdr;
};
void jpeg_colour_launch_encode(hipStream_t s, const JpegColourCtx &c);

// ---- host side (jpeg_host.cpp) ---------------------------------------------------------------------------------------
void jpeg_build_tables(int quality, JpegTables &t, unsigned char q_out[64]);
// The table pair of a colour file: t[0] luminance (the gray encoder's), t[1] chrominance (Annex K.2 / K.3.3 tables 2).
void jpeg_build_colour_tables(int quality, JpegTables t[2]);
// The file header up to and including SOS of a w x h colour image (include/dfx_jpeg_tables.h: dfx_jpeg_colour_header).
std::vector<unsigned char> jpeg_colour_file_header(int w, int h, int quality);
// The file header up to and including SOS for a w x h gray image with quantiser q (what imencodeJpeg writes).
std::vector<unsigned char> jpeg_file_header(int w, int h, const unsigned char q[64]);
// header + byte-stuffed entropy-coded segment (`bits` bits at src, last byte padded with ones) + EOI into dst.
// Returns the file size, or 0 when it would exceed `capacity`.
size_t jpeg_assemble(const std::vector<unsigned char> &header, const unsigned char *src, unsigned long long bits,
                     unsigned char *dst, size_t capacity);
