// nsr_figure.h -- the figure of src/utils/Visualizer.py:24-107 (include/nsr.h, "Rendering figures"): a 2 x 3 sheet per frame pair,
// input depth | generated depth | depth residual over input RGB | generated RGB | RGB residual, as bytes ready for an image file,
// and the depth colour map alone.  Included by nsr_api.cpp AFTER nsr_imgmetrics.h (im_clip).
//
// Numerical contract (tests/figure_reference.py restates it in numpy, operation for operation; the bytes are the same on the GPU,
// in the emulator and there):
//   Inputs     rendered colour a, input colour b [B][H][W][3]; rendered depth d, input depth g [B][H][W]; all fp32.  H, W >= 1.
//   Layout     h = ceil(H / stride), w = ceil(W / stride); sheet u8 [B][SH][SW][3], SH = 2 margin + 2 h + gap, SW = 2 margin + 3 w + 2 gap;
//              panel (r, c) starts at row margin + r (h + gap), column margin + c (w + gap); its pixel (y, x) shows the source pixel
//              (y stride, x stride); every byte outside the six panels is 255.  Row 0: g, d, depth residual; row 1: b, a, colour residual.
//   vmax       per frame the maximum of g over ALL its pixels, folded with fmaxf from -inf (a NaN does not win): what nsr_image_metrics
//              reports as the depth maximum, bit for bit.
//   Depth      a NaN value is white.  Else index = 0 if vmax == 0, else with t = v / vmax (ONE correctly rounded fp32 division, no
//              reciprocal): 255 if t >= 1 (also +inf), (int)(t * 256.0f) if 0 < t < 1, else 0 (t <= 0, or not a number: vmax is).  The
//              colour is kPlasmaLut[index]: matplotlib's Normalize(0, vmax) and its 256-entry plasma map, floor(colors * 255).
//   Residuals  nsr_image_metrics' maps: |g - d| and |b_c - a_c|, one fp32 subtraction each, 0 where g == 0.  The depth residual goes
//              through the colour map with the same vmax.
//   RGB        (uint8)(fminf(fmaxf(v, 0), 1) * 255.0f), truncated; a NaN gives 0.
//
// Three launches, no atomics, nothing depends on a frame's place in the batch:
//   1 figure_max_partial_kernel  grid (np, B): block j of a frame folds the elements j 256 + t, + np 256, ... and leaves ONE partial
//   2 figure_max_final_kernel    grid B: folds the np partials in a fixed tree into the frame's vmax
//   3 figure_sheet_kernel        the output of the WHOLE batch as one array of pixels: a lane produces kFigLane neighbouring pixels
//                                = 12 bytes = three whole dwords, which are aligned whatever the frame's size is (the output's base
//                                must be 4-byte aligned); only the batch's last lane can hold fewer pixels and stores bytes.
// The partials need no workspace of their own: they sit in the frame's own part of the OUTPUT, which launch 3 overwrites after launch 2
// has read them.  A frame's vmax goes to the caller's [B] buffer; without one it goes to the first whole dword of the frame's output
// (its "slot"), launch 3 leaves that dword alone, and a fourth launch of one thread per frame reads the slot and writes the dword's
// four bytes (figure_slot_kernel).  (A depth image of fewer than kFigTinyPixels pixels cannot hold a slot: each lane folds them itself.)
//
// The sheet kernel is a stream, 18 bytes out per source pixel and 32 in (measured: DESIGN.md 3.16).  A source value is asked for by up to three panels
// (g by three, the others by two); the panels of one sheet row lie next to one another in the pixel order, so the blocks that ask
// for the same source row run at about the same time and the repeats are served by the caches.  The colour map is staged in LDS
// once per block as 256 packed dwords (1 KiB: one ds_read_b32 per look-up instead of three byte reads of the 768-byte table).
#pragma once

namespace nsr {

constexpr int kFigThreads = 256;
constexpr int kFigLane = 4;                   // neighbouring output pixels per lane: 12 bytes, three dwords
constexpr int kFigMaxChunk = 4096;            // elements per block of the partial maximum (16 per thread)
constexpr int kFigTinyPixels = 6;             // 3 * 6 = 18 bytes: the smallest output that holds a slot and a partial
constexpr int kFigLds = 4 * 256;
constexpr unsigned kFigWhite = 0xffffffu;
static_assert(kFigThreads == 256, "a thread stages one entry of the colour map");

// floor(matplotlib.colormaps["plasma"].colors * 255): tests/golden/make_golden_plasma.py --header prints these rows
constexpr unsigned char kPlasmaLut[256][3] = {
    {12,7,134}, {16,7,135}, {19,6,137}, {21,6,138}, {24,6,139}, {27,6,140}, {29,6,141}, {31,5,142},
    {33,5,143}, {35,5,144}, {37,5,145}, {39,5,146}, {41,5,147}, {43,5,148}, {45,4,148}, {47,4,149},
    {49,4,150}, {51,4,151}, {52,4,152}, {54,4,152}, {56,4,153}, {58,4,154}, {59,3,154}, {61,3,155},
    {63,3,156}, {64,3,156}, {66,3,157}, {68,3,158}, {69,3,158}, {71,2,159}, {73,2,159}, {74,2,160},
    {76,2,161}, {78,2,161}, {79,2,162}, {81,1,162}, {82,1,163}, {84,1,163}, {86,1,163}, {87,1,164},
    {89,1,164}, {90,0,165}, {92,0,165}, {94,0,165}, {95,0,166}, {97,0,166}, {98,0,166}, {100,0,167},
    {101,0,167}, {103,0,167}, {104,0,167}, {106,0,167}, {108,0,168}, {109,0,168}, {111,0,168}, {112,0,168},
    {114,0,168}, {115,0,168}, {117,0,168}, {118,1,168}, {120,1,168}, {121,1,168}, {123,2,168}, {124,2,167},
    {126,3,167}, {127,3,167}, {129,4,167}, {130,4,167}, {132,5,166}, {133,6,166}, {134,7,166}, {136,7,165},
    {137,8,165}, {139,9,164}, {140,10,164}, {142,12,164}, {143,13,163}, {144,14,163}, {146,15,162}, {147,16,161},
    {149,17,161}, {150,18,160}, {151,19,160}, {153,20,159}, {154,21,158}, {155,23,158}, {157,24,157}, {158,25,156},
    {159,26,155}, {160,27,155}, {162,28,154}, {163,29,153}, {164,30,152}, {165,31,151}, {167,33,151}, {168,34,150},
    {169,35,149}, {170,36,148}, {172,37,147}, {173,38,146}, {174,39,145}, {175,40,144}, {176,42,143}, {177,43,143},
    {178,44,142}, {180,45,141}, {181,46,140}, {182,47,139}, {183,48,138}, {184,50,137}, {185,51,136}, {186,52,135},
    {187,53,134}, {188,54,133}, {189,55,132}, {190,56,131}, {191,57,130}, {192,59,129}, {193,60,128}, {194,61,128},
    {195,62,127}, {196,63,126}, {197,64,125}, {198,65,124}, {199,66,123}, {200,68,122}, {201,69,121}, {202,70,120},
    {203,71,119}, {204,72,118}, {205,73,117}, {206,74,117}, {207,75,116}, {208,77,115}, {209,78,114}, {209,79,113},
    {210,80,112}, {211,81,111}, {212,82,110}, {213,83,109}, {214,85,109}, {215,86,108}, {215,87,107}, {216,88,106},
    {217,89,105}, {218,90,104}, {219,91,103}, {220,93,102}, {220,94,102}, {221,95,101}, {222,96,100}, {223,97,99},
    {223,98,98}, {224,100,97}, {225,101,96}, {226,102,96}, {227,103,95}, {227,104,94}, {228,106,93}, {229,107,92},
    {229,108,91}, {230,109,90}, {231,110,90}, {232,112,89}, {232,113,88}, {233,114,87}, {234,115,86}, {234,116,85},
    {235,118,84}, {236,119,84}, {236,120,83}, {237,121,82}, {237,123,81}, {238,124,80}, {239,125,79}, {239,126,78},
    {240,128,77}, {240,129,77}, {241,130,76}, {242,132,75}, {242,133,74}, {243,134,73}, {243,135,72}, {244,137,71},
    {244,138,71}, {245,139,70}, {245,141,69}, {246,142,68}, {246,143,67}, {246,145,66}, {247,146,65}, {247,147,65},
    {248,149,64}, {248,150,63}, {248,152,62}, {249,153,61}, {249,154,60}, {250,156,59}, {250,157,58}, {250,159,58},
    {250,160,57}, {251,162,56}, {251,163,55}, {251,164,54}, {252,166,53}, {252,167,53}, {252,169,52}, {252,170,51},
    {252,172,50}, {252,173,49}, {253,175,49}, {253,176,48}, {253,178,47}, {253,179,46}, {253,181,45}, {253,182,45},
    {253,184,44}, {253,185,43}, {253,187,43}, {253,188,42}, {253,190,41}, {253,192,41}, {253,193,40}, {253,195,40},
    {253,196,39}, {253,198,38}, {252,199,38}, {252,201,38}, {252,203,37}, {252,204,37}, {252,206,37}, {251,208,36},
    {251,209,36}, {251,211,36}, {250,213,36}, {250,214,36}, {250,216,36}, {249,217,36}, {249,219,36}, {248,221,36},
    {248,223,36}, {247,224,36}, {247,226,37}, {246,228,37}, {246,229,37}, {245,231,38}, {245,233,38}, {244,234,38},
    {243,236,38}, {243,238,38}, {242,240,38}, {242,241,38}, {241,243,38}, {240,245,37}, {240,246,35}, {239,248,33},
};

struct FigureParams {
    const float *color, *gt_color;      // a, b [B][H][W][3] (null for the colour map alone)
    const float *depth, *gt_depth;      // d, g [B][H][W]    (the colour map alone: depth is the image, gt_depth null)
    const float *vmax;                  // [B], or null: the frame's slot in `out`
    float *vmax_out;                    // [B] or null: where launch 2 leaves the maxima (null: the slots)
    unsigned char *out;                 // [B][SH][SW][3], 4-byte aligned
    long long npix;                     // B SH SW
    int B, H, W, stride, margin, gap, h, w, SH, SW;
    int sheet;                          // 1: the six panels; 0: the colour map of `depth` alone (SH = H, SW = W)
    int np;                             // partial maxima per frame
    int skip_slot;                      // launch 3 leaves the frames' slot dwords to figure_slot_kernel
    int tiny;                           // colour map alone, own maximum, fewer than kFigTinyPixels pixels: no slot, every lane folds
};

// the first whole dword of frame k's output: its index in `out` taken as dwords
NSR_DEV long long fig_slot(const FigureParams &P, long long k) { return (k * (3ll * P.SH * P.SW) + 3) >> 2; }

NSR_DEV unsigned fig_cmap(const unsigned *lut, float v, float vmax) {
    if (v != v) return kFigWhite;
    int idx = 0;
    if (vmax != 0.f) {
        const float t = v / vmax;
        idx = t >= 1.f ? 255 : (t > 0.f ? (int)(t * 256.f) : 0);
    }
    return lut[idx];
}

NSR_DEV unsigned fig_byte(float v) { return (unsigned)(unsigned char)(im_clip(v) * 255.f); }

NSR_DEV float fig_vmax(const FigureParams &P, long long k) {
    if (P.tiny) {
        float m = -INFINITY;
        for (int i = 0; i < P.H * P.W; ++i) m = fmaxf(m, P.depth[k * P.H * P.W + i]);
        return m;
    }
    return P.vmax ? P.vmax[k] : reinterpret_cast<const float *>(P.out)[fig_slot(P, k)];
}

// pixel (sy, sx) of frame k's output as r | g << 8 | b << 16
NSR_DEV unsigned fig_pixel(const FigureParams &P, const unsigned *lut, long long k, int sy, int sx, float vmax) {
    int r = 0, c = 1, yy = sy, xx = sx;
    if (P.sheet) {
        const int ry = sy - P.margin, cx = sx - P.margin, ph = P.h + P.gap, pw = P.w + P.gap;
        if (ry < 0 || cx < 0) return kFigWhite;
        r = ry >= ph ? 1 : 0;
        c = cx >= 2 * pw ? 2 : (cx >= pw ? 1 : 0);
        yy = ry - r * ph;
        xx = cx - c * pw;
        if (yy >= P.h || xx >= P.w) return kFigWhite;              // a gap, or the margin below / right of the panels
    }
    const long long pix = (k * P.H + (long long)yy * P.stride) * P.W + (long long)xx * P.stride;
    if (r == 0) {
        if (c == 1) return fig_cmap(lut, P.depth[pix], vmax);
        const float g = P.gt_depth[pix];
        if (c == 0) return fig_cmap(lut, g, vmax);
        return fig_cmap(lut, g != 0.f ? fabsf(g - P.depth[pix]) : 0.f, vmax);
    }
    if (c == 0) return fig_byte(P.gt_color[3 * pix]) | fig_byte(P.gt_color[3 * pix + 1]) << 8 | fig_byte(P.gt_color[3 * pix + 2]) << 16;
    if (c == 1) return fig_byte(P.color[3 * pix]) | fig_byte(P.color[3 * pix + 1]) << 8 | fig_byte(P.color[3 * pix + 2]) << 16;
    const bool valid = P.gt_depth[pix] != 0.f;
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out |= fig_byte(valid ? fabsf(P.gt_color[3 * pix + ch] - P.color[3 * pix + ch]) : 0.f) << (8 * ch);
    return out;
}

// [kFigThreads] floats in LDS -> red[0], the same pairing whatever the values
NSR_DEV void fig_block_max(float *red, int t) {
    block_sync();
    for (int w = kFigThreads / 2; w >= 1; w >>= 1) {
        if (t < w) red[t] = fmaxf(red[t], red[t + w]);
        block_sync();
    }
}

NSR_KERNEL NSR_BOUNDS(kFigThreads) void figure_max_partial_kernel(const FigureParams P) {
    float *red = reinterpret_cast<float *>(lds_base());
    const int t = tid(), j = bid_x();
    const long long k = bid_y(), n = (long long)P.H * P.W;
    const float *src = (P.sheet ? P.gt_depth : P.depth) + k * n;
    float m = -INFINITY;
    for (long long i = (long long)j * kFigThreads + t; i < n; i += (long long)P.np * kFigThreads) m = fmaxf(m, src[i]);
    red[t] = m;
    fig_block_max(red, t);
    if (t == 0) reinterpret_cast<float *>(P.out)[fig_slot(P, k) + 1 + j] = red[0];
}

NSR_KERNEL NSR_BOUNDS(kFigThreads) void figure_max_final_kernel(const FigureParams P) {
    float *red = reinterpret_cast<float *>(lds_base());
    const int t = tid();
    const long long k = bid_x();
    float *slot = reinterpret_cast<float *>(P.out) + fig_slot(P, k);
    float m = -INFINITY;
    for (int j = t; j < P.np; j += kFigThreads) m = fmaxf(m, slot[1 + j]);
    red[t] = m;
    fig_block_max(red, t);
    if (t == 0) {
        if (P.vmax_out) P.vmax_out[k] = red[0];
        else slot[0] = red[0];
    }
}

NSR_KERNEL NSR_BOUNDS(kFigThreads) void figure_sheet_kernel(const FigureParams P) {
    unsigned *lut = reinterpret_cast<unsigned *>(lds_base());
    const int t = tid();
    lut[t] = (unsigned)kPlasmaLut[t][0] | (unsigned)kPlasmaLut[t][1] << 8 | (unsigned)kPlasmaLut[t][2] << 16;       // kFigThreads == 256
    block_sync();
    const long long group = (long long)bid_x() * kFigThreads + t, p0 = group * kFigLane;
    if (p0 >= P.npix) return;
    const int fp = P.SH * P.SW;                                    // pixels of a frame's output (< 2^31 / 3)
    long long k = p0 / fp;
    const int rem = (int)(p0 - k * fp);
    int sy = rem / P.SW, sx = rem - sy * P.SW;
    float vmax = fig_vmax(P, k);
    unsigned px[kFigLane];
    const int n = P.npix - p0 < kFigLane ? (int)(P.npix - p0) : kFigLane;
#pragma unroll
    for (int i = 0; i < kFigLane; ++i) {
        px[i] = 0;
        if (i < n) {
            px[i] = fig_pixel(P, lut, k, sy, sx, vmax);
            if (++sx == P.SW) {
                sx = 0;
                if (++sy == P.SH) {
                    sy = 0;
                    ++k;
                    if (i + 1 < n) vmax = fig_vmax(P, k);
                }
            }
        }
    }
    if (n == kFigLane) {
        const unsigned dw[3] = {px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8};
        unsigned *o = reinterpret_cast<unsigned *>(P.out) + 3 * group;
        if (P.skip_slot) {                                         // the lane's pixels lie in the frame of p0 and at most the next one
            const long long f0 = p0 / fp, s0 = fig_slot(P, f0), s1 = fig_slot(P, f0 + 1);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (3 * group + q != s0 && 3 * group + q != s1) o[q] = dw[q];
        } else {
            o[0] = dw[0];
            o[1] = dw[1];
            o[2] = dw[2];
        }
    } else {                                                       // the batch's last pixels: fewer than a lane's share
        unsigned char *o = P.out + 3 * p0;
        const long long s0 = 4 * fig_slot(P, p0 / fp);
        for (int i = 0; i < n; ++i)
            for (int ch = 0; ch < 3; ++ch) {
                const long long at = 3 * p0 + 3 * i + ch;
                if (P.skip_slot && at >= s0 && at < s0 + 4) continue;
                o[3 * i + ch] = (unsigned char)(px[i] >> (8 * ch));
            }
    }
}

// without a vmax buffer: thread k reads frame k's slot and writes the four bytes of the output that share its dword
NSR_KERNEL NSR_BOUNDS(kFigThreads) void figure_slot_kernel(const FigureParams P) {
    unsigned *lut = reinterpret_cast<unsigned *>(lds_base());
    const int t = tid();
    lut[t] = (unsigned)kPlasmaLut[t][0] | (unsigned)kPlasmaLut[t][1] << 8 | (unsigned)kPlasmaLut[t][2] << 16;
    block_sync();
    const long long k = (long long)bid_x() * kFigThreads + t;
    if (k >= P.B) return;
    const long long slot = fig_slot(P, k), fp = (long long)P.SH * P.SW;
    const float vmax = reinterpret_cast<const float *>(P.out)[slot];
    unsigned dw = 0;
    for (int q = 0; q < 4; ++q) {
        const long long at = 4 * slot + q, p = at / 3 - k * fp;   // the byte's pixel in frame k (the slot lies inside the frame)
        const int sy = (int)(p / P.SW), sx = (int)(p - (long long)sy * P.SW);
        dw |= ((fig_pixel(P, lut, k, sy, sx, vmax) >> (8 * (int)(at % 3))) & 255u) << (8 * q);
    }
    reinterpret_cast<unsigned *>(P.out)[slot] = dw;
}

}  // namespace nsr
