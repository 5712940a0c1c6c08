// nsr_imgmetrics.h -- rendering evaluation of frame pairs (include/nsr.h, "Rendering evaluation"): colour squared error (PSNR),
// SSIM, depth L1, the input depth's maximum and the residual maps of src/utils/Visualizer.py:53-65, one launch per batch.
// Included by nsr_api.cpp AFTER nsr_kernels.h, whose device primitives it uses.
//
// Numerical contract (tests/imgmetrics_reference.py restates the definitions in fp64):
//   Inputs     rendered colour a [B][H][W][3], input colour b [B][H][W][3], rendered depth d [B][H][W], input depth g [B][H][W],
//              all fp32.  A pixel is valid iff g != 0 (Visualizer.py:63).
//   Sq. error  per pixel s = sum_c ((double)clip(a_c) - (double)clip(b_c))^2, clip(v) = min(max(v, 0), 1) (Visualizer.py:85-87):
//              the difference is exact in fp64.  Summed over all pixels and over the valid ones.
//   Depth L1   sum over valid pixels of |(double)g - (double)d|, with their count; the maximum of g over all pixels.
//   Residuals  (optional) |g - d| and |b_c - a_c| (unclipped), one fp32 subtraction each, 0 where g == 0.
//   SSIM       Wang et al. 2004 on the clipped colours, per channel: an 11 x 11 Gaussian (sigma 1.5; the 1-D weights are
//              normalised in fp64 on the host and rounded to fp32), windows wholly inside the image ((H - 10) (W - 10) of them),
//              biased moments, C1 = 0.01^2, C2 = 0.03^2, the mean of the map over windows and channels; not masked by depth.
//              Moment arithmetic: the five moments of a window are taken in fp32 of the SHIFTED values x' = clip(a) - sa,
//              y' = clip(b) - sb, where sa, sb are the clipped values of the pixel at the centre of the block's patch (one shift
//              per block, image and channel).  Variances and the covariance do not depend on a shift, and the means are sa + E[x'],
//              sb + E[y']; but the shifted values of a smooth image are small, so E[x'^2] - E[x']^2 does not cancel the way
//              E[x^2] - E[x]^2 of values near 1 does.  Each moment is a separable sum, 11 fmaf along the row then 11 fmaf down the
//              column, taps in ascending order; the map value is formed from the fp32 moments in fp64.
//   Sums       per thread in fp64 in a fixed pixel / window order, per block a tree of 256 (reduce_kernel's pairing), blocks
//              into a workspace, and per frame one block that strides over the tile partials and reduces them with the same
//              tree.  No atomics: two runs give the same bits, and a frame's result does not depend on its place in the batch.
//
// A block owns a kImTile x kImTile tile of window positions of one frame and stages the kImPatch x kImPatch pixels under them,
// both images, three channels, once.  A pixel belongs to the block whose tile holds it; the last tile of a row (column) also
// owns the up to 10 pixels right of (below) its windows, so the sums and the residual stores cover the border that has no
// window of its own.  LDS: the patch [6][42][43] floats (row stride 43: the row pass runs its lanes down a column) and one
// channel's row-pass moments [5][42][33] (stride 33 for the same reason), 71 064 B: two blocks per CU.
#pragma once

namespace nsr {

constexpr int kImTile = 32;                                   // window positions per block edge
constexpr int kImWin = 11;                                    // Gaussian window
constexpr int kImPatch = kImTile + kImWin - 1;                // 42 staged pixels per edge
constexpr int kImPatchStride = kImPatch + 1;                  // 43
constexpr int kImRowStride = kImTile + 1;                     // 33
constexpr int kImThreads = 256;
constexpr int kImPartials = 6;                                // per block: se_all, se_valid, n_valid, ssim sum, l1 sum, depth max
constexpr int kImResults = 8;                                 // per frame, see nsr.h
constexpr int kImPatchFloats = 6 * kImPatch * kImPatchStride;
constexpr int kImRowFloats = 5 * kImPatch * kImRowStride;
constexpr int kImLds = 4 * (kImPatchFloats + kImRowFloats);   // the row-pass buffer doubles as the [6][256] fp64 reduction scratch
constexpr int kImFinalLds = 8 * kImPartials * kImThreads;
static_assert(8 * kImPartials * kImThreads <= 4 * kImRowFloats && (4 * kImPatchFloats) % 8 == 0, "reduction scratch");
static_assert(kImThreads == 8 * kImTile && kImTile % 4 == 0, "thread maps of the two passes");

struct ImgMetricsParams {
    const float *color, *gt_color;   // [B][H][W][3]
    const float *depth, *gt_depth;   // [B][H][W]
    int B, H, W, tx, ty, ntiles;     // tiles per row (tx) and per column (ty) of window positions
    float g[kImWin];                 // the normalised 1-D Gaussian
    double *partial;                 // [B][ntiles][kImPartials]
    double *out;                     // [B][kImResults]
    float *depth_res;                // [B][H][W] or null
    float *color_res;                // [B][H][W][3] or null
};

NSR_DEV float im_clip(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// [kImPartials][kImThreads] fp64 in LDS -> entry [q][0]: sums for q < 5, the maximum for q = 5
NSR_DEV void im_block_reduce(double *red, int t) {
    block_sync();
    for (int w = kImThreads / 2; w >= 1; w >>= 1) {
        if (t < w) {
            for (int q = 0; q < kImPartials - 1; ++q) red[q * kImThreads + t] = red[q * kImThreads + t] + red[q * kImThreads + t + w];
            double *m = red + (kImPartials - 1) * kImThreads;
            m[t] = fmax(m[t], m[t + w]);
        }
        block_sync();
    }
}

NSR_KERNEL NSR_BOUNDS(kImThreads) void imgmetrics_tile_kernel(const ImgMetricsParams P) {
    float *patch = reinterpret_cast<float *>(lds_base());
    float *rowm = patch + kImPatchFloats;
    const int t = tid(), k = bid_y(), tile = bid_x();
    const int tj = tile / P.tx, ti = tile - tj * P.tx;
    const int gx0 = ti * kImTile, gy0 = tj * kImTile, H = P.H, W = P.W;
    const bool lastx = ti == P.tx - 1, lasty = tj == P.ty - 1;
    const long long frame = (long long)k * H * W;
    const float *col = P.color + 3 * frame, *gcol = P.gt_color + 3 * frame;

    float sh[6];                                      // the block's shifts: the patch's centre pixel (clamped into the image)
    {
        const int sx = gx0 + kImPatch / 2 < W ? gx0 + kImPatch / 2 : W - 1, sy = gy0 + kImPatch / 2 < H ? gy0 + kImPatch / 2 : H - 1;
        const long long sp = 3 * ((long long)sy * W + sx);
        for (int c = 0; c < 3; ++c) {
            sh[c] = im_clip(col[sp + c]);
            sh[3 + c] = im_clip(gcol[sp + c]);
        }
    }

    double se_all = 0.0, se_valid = 0.0, n_valid = 0.0, ssim = 0.0, l1 = 0.0;
    float dmax = -INFINITY;
    for (int e = t; e < kImPatch * kImPatch; e += kImThreads) {
        const int py = e / kImPatch, px = e - py * kImPatch;
        const int gx = gx0 + px, gy = gy0 + py;
        float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
        if (gx < W && gy < H) {
            const long long pix = (long long)gy * W + gx;
            float ra[3], rb[3], ca[3], cb[3];
            for (int c = 0; c < 3; ++c) {
                ra[c] = col[3 * pix + c];
                rb[c] = gcol[3 * pix + c];
                ca[c] = im_clip(ra[c]);
                cb[c] = im_clip(rb[c]);
                a[c] = ca[c] - sh[c];
                b[c] = cb[c] - sh[3 + c];
            }
            if ((px < kImTile || lastx) && (py < kImTile || lasty)) {          // this block's pixel
                const float gd = P.gt_depth[frame + pix], d = P.depth[frame + pix];
                const bool valid = gd != 0.f;
                double s = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double df = (double)ca[c] - (double)cb[c];
                    s = s + df * df;
                }
                se_all = se_all + s;
                if (valid) {
                    se_valid = se_valid + s;
                    l1 = l1 + fabs((double)gd - (double)d);
                    n_valid = n_valid + 1.0;
                }
                dmax = fmaxf(dmax, gd);
                if (P.depth_res) P.depth_res[frame + pix] = valid ? fabsf(gd - d) : 0.f;
                if (P.color_res)
                    for (int c = 0; c < 3; ++c) P.color_res[3 * (frame + pix) + c] = valid ? fabsf(rb[c] - ra[c]) : 0.f;
            }
        }
        for (int c = 0; c < 3; ++c) {
            patch[(c * kImPatch + py) * kImPatchStride + px] = a[c];
            patch[((3 + c) * kImPatch + py) * kImPatchStride + px] = b[c];
        }
    }
    block_sync();

    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    for (int c = 0; c < 3; ++c) {
        // row pass: an item is 4 neighbouring outputs of one patch row (14 staged pixels of each image); lanes run down a column
        const float *pa = patch + c * kImPatch * kImPatchStride, *pb = patch + (3 + c) * kImPatch * kImPatchStride;
        for (int it = t; it < kImPatch * (kImTile / 4); it += kImThreads) {
            const int xg = it / kImPatch, r = it - xg * kImPatch;
            const float *xa = pa + r * kImPatchStride + 4 * xg, *xb = pb + r * kImPatchStride + 4 * xg;
            float acc[4][5];
            for (int q = 0; q < 4; ++q)
                for (int m = 0; m < 5; ++m) acc[q][m] = 0.f;
#pragma unroll
            for (int j = 0; j < kImWin + 3; ++j) {
                const float x = xa[j], y = xb[j];
                const float v[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int w = j - q;
                    if (w < 0 || w >= kImWin) continue;
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[q][m] = fmaf(P.g[w], v[m], acc[q][m]);
                }
            }
            for (int q = 0; q < 4; ++q)
                for (int m = 0; m < 5; ++m) rowm[(m * kImPatch + r) * kImRowStride + 4 * xg + q] = acc[q][m];
        }
        block_sync();
        // column pass: a thread owns 4 windows below one another (14 rows of the row-pass moments); lanes run along a row
        {
            const int x = t & (kImTile - 1), yb = (t / kImTile) * 4;
            float acc[4][5];
            for (int q = 0; q < 4; ++q)
                for (int m = 0; m < 5; ++m) acc[q][m] = 0.f;
#pragma unroll
            for (int j = 0; j < kImWin + 3; ++j) {
                float v[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) v[m] = rowm[(m * kImPatch + yb + j) * kImRowStride + x];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int w = j - q;
                    if (w < 0 || w >= kImWin) continue;
#pragma unroll
                    for (int m = 0; m < 5; ++m) acc[q][m] = fmaf(P.g[w], v[m], acc[q][m]);
                }
            }
            for (int q = 0; q < 4; ++q) {
                if (gx0 + x >= W - (kImWin - 1) || gy0 + yb + q >= H - (kImWin - 1)) continue;      // no such window
                const double ex = acc[q][0], ey = acc[q][1];
                const double mx = (double)sh[c] + ex, my = (double)sh[3 + c] + ey;
                const double vx = (double)acc[q][2] - ex * ex, vy = (double)acc[q][3] - ey * ey, vxy = (double)acc[q][4] - ex * ey;
                const double num = (2.0 * mx * my + C1) * (2.0 * vxy + C2), den = (mx * mx + my * my + C1) * (vx + vy + C2);
                ssim = ssim + num / den;
            }
        }
        block_sync();
    }

    double *red = reinterpret_cast<double *>(rowm);
    red[t] = se_all;
    red[kImThreads + t] = se_valid;
    red[2 * kImThreads + t] = n_valid;
    red[3 * kImThreads + t] = ssim;
    red[4 * kImThreads + t] = l1;
    red[5 * kImThreads + t] = (double)dmax;
    im_block_reduce(red, t);
    if (t < kImPartials) P.partial[((long long)k * P.ntiles + tile) * kImPartials + t] = red[t * kImThreads];
}

// one block per frame: thread t takes the tiles t, t + 256, ... in order, then the tree
NSR_KERNEL NSR_BOUNDS(kImThreads) void imgmetrics_final_kernel(const ImgMetricsParams P) {
    double *red = reinterpret_cast<double *>(lds_base());
    const int t = tid(), k = bid_x();
    double acc[kImPartials] = {0.0, 0.0, 0.0, 0.0, 0.0, -INFINITY};
    for (int b = t; b < P.ntiles; b += kImThreads) {
        const double *p = P.partial + ((long long)k * P.ntiles + b) * kImPartials;
        for (int q = 0; q < kImPartials - 1; ++q) acc[q] = acc[q] + p[q];
        acc[kImPartials - 1] = fmax(acc[kImPartials - 1], p[kImPartials - 1]);
    }
    for (int q = 0; q < kImPartials; ++q) red[q * kImThreads + t] = acc[q];
    im_block_reduce(red, t);
    if (t == 0) {
        double *o = P.out + (long long)k * kImResults;
        const double nwin = (double)(P.H - (kImWin - 1)) * (double)(P.W - (kImWin - 1));
        o[0] = red[0];                                        // colour squared error, all pixels
        o[1] = (double)P.H * (double)P.W;                     // ... their count
        o[2] = red[kImThreads];                               // colour squared error, valid pixels
        o[3] = red[2 * kImThreads];                           // ... their count (also the depth L1's)
        o[4] = red[3 * kImThreads] / (3.0 * nwin);            // SSIM
        o[5] = red[4 * kImThreads];                           // sum of |g - d| over valid pixels
        o[6] = red[5 * kImThreads];                           // max g
        o[7] = 0.0;
    }
}

}  // namespace nsr
