// nsr_jpeg.h -- a baseline JPEG encoder (ITU-T T.81 sequential DCT, 8 bit, three components, JFIF YCbCr) for a batch of images that
// are already on the device (include/nsr.h, "JPEG encoding").  The library produces each frame's entropy-coded segment, byte-stuffed,
// with its restart markers, in one compact buffer; the caller writes the markers around it (SOI .. SOS, EOI: nice_slam_amd/jpeg.py).
// Included by nsr_api.cpp.
//
// Numerical contract (tests/jpeg_reference.py restates it in numpy, operation for operation; the bytes are the same on the GPU, in the
// emulator and there).  Integers end to end; `>>` is the arithmetic shift; no floating point, no atomics on global memory.
//   Input      u8 [n][H][W][3], RGB.  1 <= H, W <= 65535.
//   MCU        4:4:4: 8 x 8 pixels, blocks Y Cb Cr.  4:2:0: 16 x 16 pixels, blocks Y00 Y01 Y10 Y11 Cb Cr (Y in raster order).  A pixel
//              outside the image is the nearest one inside (its last column / row repeated).  A block that holds NO pixel of the
//              image (4:2:0 only: the right or lower Y blocks of an MCU that the image ends in) is a dummy as libjpeg makes them:
//              its DC value is that of the Y block before it and it has no AC, so it costs a zero difference and an EOB.
//   Colour     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//              Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
//              Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16          (the 16-bit constants of JFIF's matrix)
//   Chroma     4:2:0: a sample is (a + b + c + d + 2) >> 2 of the 2 x 2 pixels' Cb (Cr), each converted as above.
//   Shift      s = sample - 128.
//   DCT        M[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2: the integers of kJpgCos below.
//              Rows first:   t[y][u] = (sum_x M[u][x] s[y][x] + 512) >> 10         (three fractional bits kept)
//              then columns: F[v][u] = sum_y M[v][y] t[y][u]                        (the coefficient times 2^16, |F| < 2^31)
//   Quantise   with the table entry Q: d = Q << 16, c = (|F| + (d >> 1)) / d, the sign of F put back (round half away from zero);
//              AC values are clamped to +-1023.  Tables: Annex K scaled by the IJG rule, s = q < 50 ? 5000 / q : 200 - 2 q,
//              Q = clamp((T s + 50) / 100, 1, 255).
//   Scan       int16 [block][64] in zig-zag order, the blocks in interleaved scan order: frame, MCU row, MCU, block of the MCU.
//   Entropy    the four "typical" Huffman tables of Annex K (K.3 - K.6).  The restart interval is ONE MCU ROW: at its start the DC
//              predictors are 0 and the stream is byte-aligned, its last byte is padded with 1-bits, and behind every interval but
//              a frame's last stands RSTm, m = MCU row mod 8.  A 0xFF byte of the coded data is followed by 0x00.
//
// Four stages, seven launches.  `interval` = one MCU row of one frame; a block = one 8 x 8 block of coefficients.
//   1 jpeg_transform_kernel<S>  a lane per block: load with edge replication, convert, (downsample,) DCT, quantise, zig-zag, store
//   2 jpeg_measure_kernel       a workgroup per interval: a lane per block takes its DC difference and sums its code lengths; a
//                               fixed-order scan over the interval's blocks gives each its bit offset and the interval its length
//   3 jpeg_pack_kernel          a workgroup per interval: a window of the interval's bit stream is assembled in LDS -- every block
//                               adds its codes at its bit offset (disjoint bits: integer adds in LDS, any order gives the same word) --
//                               and then stored, one lane per word
//   4 jpeg_count_kernel         a workgroup per interval: the 0xFF bytes of its stream
//     jpeg_offsets_kernel       grid n, then grid 1: the stuffed lengths scanned over a frame's intervals, then over the frames
//     jpeg_stuff_kernel         a workgroup per interval: its bytes go to their final place, 0xFF followed by 0x00, RSTm behind
// Workspace (nsr_jpeg_size): coefficients 128 B per block, bit offsets 4 B per block, the unstuffed stream at its worst case per
// interval -- a block is at most 63 AC codes of 16 + 10 bits and a DC code of 9 + 11 -- and four numbers per interval and frame.
// The output's worst case is that stream doubled by stuffing plus the restart markers.  Nothing is sized by what an image holds.
#pragma once

namespace nsr {

constexpr int kJpgThreads = 256;
constexpr int kJpgBlockBits = 63 * 26 + 20;       // worst case of one block
constexpr int kJpgWinWords = 4096;                // the pack kernel's LDS window: 16 KiB = 131072 bits of an interval at a time
constexpr int kJpgHuffEntries = 2 * 16 + 2 * 256; // DC lum, DC chroma, AC lum, AC chroma: code | length << 16
constexpr int kJpgStuffBytes = 8;                 // bytes per lane and round of the stuff kernel
constexpr int kJpgScanLds = 2 * 8 * kJpgThreads;                      // jpg_scan's two rows of 64-bit values
constexpr int kJpgMeasureLds = 4 * kJpgHuffEntries + kJpgScanLds;     // the code tables, then the scan
constexpr int kJpgPackLds = 4 * kJpgHuffEntries + 4 * kJpgWinWords;   // the code tables, then the window

// round(4096 cos(k pi / 16)), k = 0..7; row 0 of M is round(8192 sqrt(1 / 8)) = kJpgCos[4]
constexpr int kJpgCos[8] = {4096, 4017, 3784, 3406, 2896, 2276, 1567, 799};

// natural index of zig-zag position k (T.81 figure A.6)
constexpr unsigned char kJpgZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 tables K.1 and K.2, natural order
constexpr unsigned char kJpgQuantBase[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// T.81 tables K.3 - K.6: the number of codes of each length 1..16 and the symbols in code order
constexpr unsigned char kJpgDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kJpgDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kJpgAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char kJpgAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// the code of every symbol (T.81 annex C): entry = code | length << 16, 0 for a symbol without a code; DC lum at 0, DC chroma at 16,
// AC lum at 32, AC chroma at 288
struct JpegHuff { unsigned e[kJpgHuffEntries]; };
constexpr void jpg_huff_fill(JpegHuff &T, int at, const unsigned char *bits, const unsigned char *vals) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) T.e[at + vals[k++]] = code++ | (unsigned)len << 16;
        code <<= 1;
    }
}
constexpr JpegHuff jpg_huff_make() {
    JpegHuff T = {};
    jpg_huff_fill(T, 0, kJpgDcBits[0], kJpgDcVals);
    jpg_huff_fill(T, 16, kJpgDcBits[1], kJpgDcVals);
    jpg_huff_fill(T, 32, kJpgAcBits[0], kJpgAcVals[0]);
    jpg_huff_fill(T, 288, kJpgAcBits[1], kJpgAcVals[1]);
    return T;
}
constexpr JpegHuff kJpgHuff = jpg_huff_make();

struct JpegParams {
    const unsigned char *img;           // [n][H][W][3]
    short *coef;                        // [nblocks][64], zig-zag
    unsigned *bitoff;                   // [nblocks]: a block's first bit in its interval's stream
    unsigned char *raw;                 // [nint][rawstride]: the intervals' unstuffed streams
    unsigned *ibits;                    // [nint]: bits of the interval before padding
    unsigned *nff;                      // [nint]: its 0xFF bytes
    long long *ioff;                    // [nint]: the interval's first byte in its frame's output
    long long *ftot;                    // [n]: a frame's bytes
    unsigned char *out;                 // the compact buffer
    long long *offsets;                 // [n + 1]
    long long nblocks;
    int n, H, W, sub;                   // sub 1: 4:4:4, 2: 4:2:0 (the MCU's side in blocks)
    int mcux, mcuy, bpm, BI, nint;      // MCUs per row / column, blocks per MCU / interval, intervals
    unsigned rawstride;
    unsigned char q[2][64];             // luminance, chrominance; zig-zag order
};

// exclusive scan over the workgroup's kJpgThreads values in a fixed order: returns the sum of the lower threads' values,
// `total` the sum of all.  s: [2 kJpgThreads] in LDS.
NSR_DEV unsigned long long jpg_scan(unsigned long long *s, int t, unsigned long long v, unsigned long long &total) {
    int cur = 0;
    s[t] = v;
    block_sync();
    for (int d = 1; d < kJpgThreads; d <<= 1) {
        unsigned long long x = s[cur * kJpgThreads + t];
        if (t >= d) x += s[cur * kJpgThreads + t - d];
        cur ^= 1;
        s[cur * kJpgThreads + t] = x;
        block_sync();
    }
    const unsigned long long incl = s[cur * kJpgThreads + t];
    total = s[cur * kJpgThreads + kJpgThreads - 1];
    block_sync();
    return incl - v;
}

NSR_DEV void jpg_stage_huff(unsigned *huff, int t) {
    for (int i = t; i < kJpgHuffEntries; i += kJpgThreads) huff[i] = kJpgHuff.e[i];
}

NSR_DEV int jpg_nbits(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }     // a >= 0

// 8 samples -> 8 sums of M[u][.] s[.], by the symmetry M[u][7 - x] = (-1)^u M[u][x] (the same integers as the full products)
NSR_DEV void jpg_dct8(const int *s, int *o) {
    constexpr int c1 = kJpgCos[1], c2 = kJpgCos[2], c3 = kJpgCos[3], c4 = kJpgCos[4], c5 = kJpgCos[5], c6 = kJpgCos[6], c7 = kJpgCos[7];
    const int a0 = s[0] + s[7], a1 = s[1] + s[6], a2 = s[2] + s[5], a3 = s[3] + s[4];
    const int b0 = s[0] - s[7], b1 = s[1] - s[6], b2 = s[2] - s[5], b3 = s[3] - s[4];
    o[0] = c4 * (a0 + a1 + a2 + a3);
    o[4] = c4 * (a0 - a1 - a2 + a3);
    o[2] = c2 * (a0 - a3) + c6 * (a1 - a2);
    o[6] = c6 * (a0 - a3) - c2 * (a1 - a2);
    o[1] = c1 * b0 + c3 * b1 + c5 * b2 + c7 * b3;
    o[3] = c3 * b0 - c7 * b1 - c1 * b2 - c5 * b3;
    o[5] = c5 * b0 - c1 * b1 + c7 * b2 + c3 * b3;
    o[7] = c7 * b0 - c5 * b1 + c3 * b2 - c1 * b3;
}

// component `comp` (0 Y, 1 Cb, 2 Cr) of the pixel at p
NSR_DEV int jpg_component(int comp, const unsigned char *p) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}

template <int S>
NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_transform_kernel(const JpegParams P) {
    constexpr int BPM = S == 1 ? 3 : 6;
    const long long blk = (long long)bid_x() * kJpgThreads + tid();
    if (blk >= P.nblocks) return;
    const long long mcu = blk / BPM, row = mcu / P.mcux;
    const int b = (int)(blk - mcu * BPM), mx = (int)(mcu - row * P.mcux);
    const long long f = row / P.mcuy;
    const int my = (int)(row - f * P.mcuy);
    const int comp = S == 1 ? b : (b < 4 ? 0 : b - 3);
    const unsigned char *src = P.img + f * (3ll * P.H * P.W);
    const int xmax = P.W - 1, ymax = P.H - 1;
    int s[64];
    if (S == 1 || comp == 0) {
        const int x0 = 8 * S * mx + (S == 2 ? 8 * (b & 1) : 0), y0 = 8 * S * my + (S == 2 ? 8 * (b >> 1) : 0);
        if (S == 2 && (x0 > xmax || y0 > ymax)) {                   // a dummy block: zeros; its DC value is resolved by jpg_dc
            unsigned *z = reinterpret_cast<unsigned *>(P.coef + 64 * blk);
#pragma unroll
            for (int i = 0; i < 32; ++i) z[i] = 0u;
            return;
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const long long line = (long long)(y0 + y < ymax ? y0 + y : ymax) * P.W;
#pragma unroll
            for (int x = 0; x < 8; ++x) s[8 * y + x] = jpg_component(comp, src + 3 * (line + (x0 + x < xmax ? x0 + x : xmax))) - 128;
        }
    } else {
        const int x0 = 16 * mx, y0 = 16 * my;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const long long l0 = (long long)(y0 + 2 * y < ymax ? y0 + 2 * y : ymax) * P.W, l1 = (long long)(y0 + 2 * y + 1 < ymax ? y0 + 2 * y + 1 : ymax) * P.W;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const int xa = x0 + 2 * x < xmax ? x0 + 2 * x : xmax, xb = x0 + 2 * x + 1 < xmax ? x0 + 2 * x + 1 : xmax;
                const int sum = jpg_component(comp, src + 3 * (l0 + xa)) + jpg_component(comp, src + 3 * (l0 + xb)) +
                                jpg_component(comp, src + 3 * (l1 + xa)) + jpg_component(comp, src + 3 * (l1 + xb));
                s[8 * y + x] = ((sum + 2) >> 2) - 128;
            }
        }
    }
    int o[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) {                                   // rows: t[y][u]
        jpg_dct8(s + 8 * y, o);
#pragma unroll
        for (int u = 0; u < 8; ++u) s[8 * y + u] = (o[u] + 512) >> 10;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {                                   // columns: F[v][u]
        int c[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) c[y] = s[8 * y + u];
        jpg_dct8(c, o);
#pragma unroll
        for (int v = 0; v < 8; ++v) s[8 * v + u] = o[v];
    }
    const unsigned char *q = P.q[comp ? 1 : 0];
    unsigned w[32];
#pragma unroll
    for (int k = 0; k < 64; ++k) {
        const int F = s[kJpgZigzag[k]];
        const unsigned d = (unsigned)q[k] << 16, a = (unsigned)(F < 0 ? -F : F);
        int c = (int)((a + (d >> 1)) / d);
        if (k > 0 && c > 1023) c = 1023;
        const unsigned h = (unsigned)(F < 0 ? -c : c) & 0xffffu;
        if (k & 1) w[k >> 1] |= h << 16;
        else w[k >> 1] = h;
    }
    unsigned *dst = reinterpret_cast<unsigned *>(P.coef + 64 * blk);       // 128-byte aligned
#pragma unroll
    for (int i = 0; i < 32; ++i) dst[i] = w[i];
}

// block b of interval i (its first block: `first`): the block whose DC value is its predictor, -1 at the interval's start
NSR_DEV long long jpg_pred(const JpegParams &P, long long first, int b) {
    const int mx = b / P.bpm, k = b - mx * P.bpm;
    if (P.sub == 2 && k > 0 && k < 4) return first + b - 1;                // Y01, Y10, Y11: the block before
    if (mx == 0) return -1;
    return first + b - (P.sub == 2 && k == 0 ? 3 : P.bpm);                  // Y00: the MCU before's Y11; else the same block there
}

// block b (Y block k of MCU mx) of MCU row my holds no pixel of the image
NSR_DEV bool jpg_dummy(const JpegParams &P, int my, int b) {
    if (P.sub != 2) return false;
    const int mx = b / 6, k = b - 6 * mx;
    return k < 4 && (16 * mx + 8 * (k & 1) >= P.W || 16 * my + 8 * (k >> 1) >= P.H);
}

// the DC value of block b: a dummy's is that of the Y block before it (Y00 of an MCU is never one)
NSR_DEV int jpg_dc(const JpegParams &P, long long first, int my, int b) {
    while (jpg_dummy(P, my, b)) --b;
    return P.coef[64 * (first + b)];
}

// One block's codes in stream order, handed to sink.put(code, length) (length <= 26): the measure and the pack kernel share it.
// c: the coefficients (c[0] is not read), dc0: the block's DC value, pred: its predictor
template <class Sink>
NSR_DEV void jpg_code_block(const short *c, int dc0, int pred, const unsigned *dc, const unsigned *ac, Sink &sink) {
    const int diff = dc0 - pred;
    int nb = jpg_nbits(diff < 0 ? -diff : diff);
    unsigned e = dc[nb];
    sink.put((e & 0xffffu) << nb | ((unsigned)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = c[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) sink.put(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
        nb = jpg_nbits(v < 0 ? -v : v);
        e = ac[run << 4 | nb];
        sink.put((e & 0xffffu) << nb | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), (int)(e >> 16) + nb);
        run = 0;
    }
    if (run > 0) sink.put(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

struct JpegCount {
    unsigned bits = 0;
    NSR_DEV void put(unsigned, int len) { bits += (unsigned)len; }
};

// adds the stream's 32-bit words (first bit = bit 31) that lie in the window [w0, w0 + nw) to win[]
struct JpegEmit {
    unsigned *win;
    unsigned w0, nw, wi;                // wi: the word being filled
    unsigned long long acc = 0;
    int nacc;                           // bits in acc (the word's bits before the block's first count as zeros)
    NSR_DEV JpegEmit(unsigned *win_, unsigned w0_, unsigned nw_, unsigned bit) : win(win_), w0(w0_), nw(nw_), wi(bit >> 5), nacc((int)(bit & 31u)) {}
    NSR_DEV void word(unsigned v) {
        if (v != 0 && wi >= w0 && wi - w0 < nw) atomic_add_lds_i(reinterpret_cast<int *>(win + (wi - w0)), (int)v);
        ++wi;
    }
    NSR_DEV void put(unsigned code, int len) {
        acc = acc << len | code;
        nacc += len;
        if (nacc >= 32) {
            nacc -= 32;
            word((unsigned)(acc >> nacc));
            acc &= (1ull << nacc) - 1ull;
        }
    }
    NSR_DEV void flush() {
        if (nacc > 0) word((unsigned)(acc << (32 - nacc)));
    }
};

NSR_DEV void jpg_tables(const JpegParams &P, int b, const unsigned *huff, const unsigned *&dc, const unsigned *&ac) {
    const int k = b % P.bpm, chroma = k >= P.bpm - 2 ? 1 : 0;
    dc = huff + 16 * chroma;
    ac = huff + 32 + 256 * chroma;
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_measure_kernel(const JpegParams P) {
    unsigned *huff = reinterpret_cast<unsigned *>(lds_base());
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base() + 4 * kJpgHuffEntries);
    const int t = tid();
    const long long i = bid_x(), first = i * P.BI;
    const int my = (int)(i % P.mcuy);
    jpg_stage_huff(huff, t);
    block_sync();
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < P.BI; b0 += kJpgThreads) {
        const int b = b0 + t;
        JpegCount cnt;
        if (b < P.BI) {
            const long long pb = jpg_pred(P, first, b);
            const unsigned *dc, *ac;
            jpg_tables(P, b, huff, dc, ac);
            jpg_code_block(P.coef + 64 * (first + b), jpg_dc(P, first, my, b), pb < 0 ? 0 : jpg_dc(P, first, my, (int)(pb - first)), dc, ac, cnt);
        }
        unsigned long long total;
        const unsigned long long before = jpg_scan(scan, t, cnt.bits, total);
        if (b < P.BI) P.bitoff[first + b] = (unsigned)(carry + before);
        carry += total;
    }
    if (t == 0) P.ibits[i] = (unsigned)carry;
}

NSR_DEV unsigned jpg_ff_count(unsigned w) {
    return (unsigned)((w & 0xffu) == 0xffu) + (unsigned)((w >> 8 & 0xffu) == 0xffu) + (unsigned)((w >> 16 & 0xffu) == 0xffu) + (unsigned)(w >> 24 == 0xffu);
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_pack_kernel(const JpegParams P) {
    unsigned *huff = reinterpret_cast<unsigned *>(lds_base());
    unsigned *win = huff + kJpgHuffEntries;
    const int t = tid();
    const long long i = bid_x(), first = i * P.BI;
    const int my = (int)(i % P.mcuy);
    jpg_stage_huff(huff, t);
    const unsigned bits = P.ibits[i], pad = (8u - (bits & 7u)) & 7u, nwords = (bits + pad + 31u) >> 5;
    unsigned *raw = reinterpret_cast<unsigned *>(P.raw + i * (long long)P.rawstride);
    const unsigned *off = P.bitoff + first;
    for (unsigned w0 = 0; w0 < nwords; w0 += kJpgWinWords) {
        const unsigned nw = nwords - w0 < (unsigned)kJpgWinWords ? nwords - w0 : (unsigned)kJpgWinWords;
        for (unsigned k = t; k < nw; k += kJpgThreads) win[k] = 0;
        block_sync();
        // the last block that starts at or before the window's first bit: it, and those behind it that start inside, have bits here
        const unsigned lo_bit = w0 << 5, hi_bit = (w0 + nw) << 5;
        int lo = 0, hi = P.BI - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= lo_bit) lo = mid;
            else hi = mid - 1;
        }
        for (int b = lo + t; b < P.BI && off[b] < hi_bit; b += kJpgThreads) {
            const long long pb = jpg_pred(P, first, b);
            const unsigned *dc, *ac;
            jpg_tables(P, b, huff, dc, ac);
            JpegEmit em(win, w0, nw, off[b]);
            jpg_code_block(P.coef + 64 * (first + b), jpg_dc(P, first, my, b), pb < 0 ? 0 : jpg_dc(P, first, my, (int)(pb - first)), dc, ac, em);
            if (b == P.BI - 1 && pad) em.put((1u << pad) - 1u, (int)pad);
            em.flush();
        }
        block_sync();
        for (unsigned k = t; k < nw; k += kJpgThreads) {
            const unsigned w = win[k];
            raw[w0 + k] = w >> 24 | (w >> 8 & 0xff00u) | (w << 8 & 0xff0000u) | w << 24;       // the stream's first byte first
        }
        block_sync();
    }
}

// the 0xFF bytes of an interval's stream (the zero bytes that fill its last word are none)
NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_count_kernel(const JpegParams P) {
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base());
    const int t = tid();
    const long long i = bid_x();
    const unsigned nwords = (((P.ibits[i] + 7u) >> 3) + 3u) >> 2;
    const unsigned *raw = reinterpret_cast<const unsigned *>(P.raw + i * (long long)P.rawstride);
    unsigned ff = 0;
    for (unsigned k = t; k < nwords; k += kJpgThreads) ff += jpg_ff_count(raw[k]);
    unsigned long long total;
    jpg_scan(scan, t, ff, total);
    if (t == 0) P.nff[i] = (unsigned)total;
}

// stage 0, grid n: ioff over the frame's intervals and the frame's length; stage 1, grid 1: offsets over the frames
NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_offsets_kernel(const JpegParams P, int stage) {
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base());
    const int t = tid();
    unsigned long long carry = 0, total;
    if (stage == 0) {
        const long long f = bid_x(), first = f * P.mcuy;
        for (int r0 = 0; r0 < P.mcuy; r0 += kJpgThreads) {
            const int r = r0 + t;
            unsigned long long len = 0;
            if (r < P.mcuy) len = (unsigned long long)((P.ibits[first + r] + 7u) >> 3) + P.nff[first + r] + (r < P.mcuy - 1 ? 2u : 0u);
            const unsigned long long before = jpg_scan(scan, t, len, total);
            if (r < P.mcuy) P.ioff[first + r] = (long long)(carry + before);
            carry += total;
        }
        if (t == 0) P.ftot[f] = (long long)carry;
    } else {
        for (int f0 = 0; f0 < P.n; f0 += kJpgThreads) {
            const int f = f0 + t;
            const unsigned long long before = jpg_scan(scan, t, f < P.n ? (unsigned long long)P.ftot[f] : 0ull, total);
            if (f < P.n) P.offsets[f] = (long long)(carry + before);
            carry += total;
        }
        if (t == 0) P.offsets[P.n] = (long long)carry;
    }
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpeg_stuff_kernel(const JpegParams P) {
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base());
    const int t = tid();
    const long long i = bid_x(), f = i / P.mcuy;
    const int r = (int)(i - f * P.mcuy);
    const unsigned nbytes = (P.ibits[i] + 7u) >> 3;
    const unsigned char *raw = P.raw + i * (long long)P.rawstride;
    unsigned char *dst = P.out + P.offsets[f] + P.ioff[i];
    unsigned long long carry = 0, total;
    for (unsigned c0 = 0; c0 < nbytes; c0 += kJpgStuffBytes * kJpgThreads) {
        const unsigned at = c0 + kJpgStuffBytes * t;
        unsigned char v[kJpgStuffBytes];
        unsigned ff = 0;
#pragma unroll
        for (int k = 0; k < kJpgStuffBytes; ++k) {
            v[k] = at + k < nbytes ? raw[at + k] : 0;
            ff += v[k] == 0xffu;
        }
        unsigned long long o = at + carry + jpg_scan(scan, t, ff, total);
#pragma unroll
        for (int k = 0; k < kJpgStuffBytes; ++k)
            if (at + k < nbytes) {
                dst[o++] = v[k];
                if (v[k] == 0xffu) dst[o++] = 0;
            }
        carry += total;
    }
    if (t == 0 && r < P.mcuy - 1) {
        dst[nbytes + carry] = 0xff;
        dst[nbytes + carry + 1] = (unsigned char)(0xd0 + (r & 7));
    }
}

}  // namespace nsr
