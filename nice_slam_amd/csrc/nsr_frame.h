// nsr_frame.h -- frame preparation (include/nsr.h, "Frame preparation"): what src/utils/datasets.py:77-113 (BaseDataset.__getitem__)
// does to a decoded colour / depth pair between the file and the tensors the tracker and the mapper read, on the raw bytes of a
// batch of frames of one geometry.  Included by nsr_api.cpp AFTER nsr_kernels.h.
//
// Numerical contract (tests/frames_reference.py restates it on the host):
//   Inputs     raw colour u8 [B][Hc][Wc][3], channels in file order BGR (cv2.imread) or RGB (PIL); raw depth u16 or fp32 [B][Hd][Wd].
//   Outputs    colour fp32 [B][H][W][3] RGB, depth fp32 [B][H][W]; (Hs, Ws) = crop_size if given, else (Hd, Wd); H = Hs - 2e,
//              W = Ws - 2e, e = crop_edge.
//   1 Undistortion (:85-88; only with distortion [k1, k2, p1, p2, k3], colour only).  For the integer pixel (u, v), all in fp64, no
//              contraction, in this association:
//                x = (u - cx) / fx, y = (v - cy) / fy, r2 = x x + y y, rad = ((1 + k1 r2) + k2 (r2 r2)) + k3 ((r2 r2) r2)
//                x' = (x rad + ((2 p1) x) y) + p2 (r2 + (2 x) x),  y' = (y rad + p1 (r2 + (2 y) y)) + ((2 p2) x) y
//                (sx, sy) = (fx x' + cx, fy y' + cy); x0 = floor(sx), ax = sx - x0, likewise y0, ay;
//                val = (1 - ay) ((1 - ax) p00 + ax p01) + ay ((1 - ax) p10 + ax p11), a tap outside the image counting as 0 (a
//                position that is not finite, or a pixel or more outside: all four taps 0); the u8 result is floor(val + 0.5).
//              Its own launch into a u8 workspace [B][Hc][Wc][3], the one intermediate.  This is the continuous bilinear remap;
//              cv2.undistort quantises the position to 1/32 pixel and the weights to 2^-15, so it can differ by a grey level.
//   2 To [0, 1] q = (double)u8 / 255.0 (:90-91).  If (Hc, Wc) != (Hd, Wd): bilinear with half-pixel centres (cv2.resize INTER_LINEAR,
//              :94; F.interpolate(align_corners=False)): per axis s = max(((double)in / out) (dst + 0.5) - 0.5, 0), i0 = min((int)s,
//              in - 1), i1 = i0 + (i0 < in - 1), w1 = s - i0, w0 = 1 - w1; value = wy0 (wx0 q00 + wx1 q01) + wy1 (wx0 q10 + wx1 q11).
//   3 Depth    ((float)raw / png_depth_scale) * scale: one correctly rounded fp32 division, one fp32 product (:92, :96).
//   4 crop_size (:97-104).  Colour: bilinear, align_corners=True, on the stage-2 image: per axis s = ((double)(in - 1) / (out - 1)) dst
//              (ratio 0 when out = 1), taps and combination as in 2.  Depth: legacy nearest, min((int)floorf(dst * ((float)in /
//              out)), in - 1), the ratio held in fp32 as ATen holds it.
//   5 crop_edge (:106-110): output pixel (y, x) is stage-4 pixel (y + e, x + e).
//   6 Rounding colour is rounded once, fp64 -> fp32, at the store.  Without stages 1, 2-resize and 4 it is (float)(u8 / 255.0): a
//              256-entry table the host forms in fp64 gives exactly that, and the kernel is a stream -- a lane takes kFrLane
//              neighbouring pixels of a row (12 bytes of colour in, 48 out), the last lane of a row the W % kFrLane that are left.
//
// Everything after the undistortion is one launch: an output pixel gathers its own taps (at most 4 x 4 per channel), so there are
// no atomics and a frame's result does not depend on its place in the batch.  Every index above is clamped into its image: the
// kernels read inside the given arrays only.
#pragma once

namespace nsr {

constexpr int kFrThreads = 256;
constexpr int kFrLane = 4;              // neighbouring pixels per lane on the stream path

struct FrameParams {
    const unsigned char *color;         // [B][Hc][Wc][3]: the raw colour, or the undistorted workspace
    const void *depth;                  // [B][Hd][Wd] u16 / fp32
    float *out_color, *out_depth;       // [B][H][W][3], [B][H][W]
    long long items;                    // B H ceil(W / kFrLane) on the stream path, else B H W
    int Hc, Wc, Hd, Wd, H, W, edge;
    int depth_f32, bgr, resize, crop, stream;
    float png_depth_scale, scale;
    float nn_h, nn_w;                   // (float)Hd / Hs, (float)Wd / Ws
    double rs_h, rs_w;                  // (double)Hc / Hd, (double)Wc / Wd
    double ac_h, ac_w;                  // (double)(Hd - 1) / (Hs - 1), 0 when Hs = 1; likewise for the width
    float tab[256];                     // (float)(i / 255.0)
};

struct UndistortParams {
    const unsigned char *src;           // [B][H][W][3]
    unsigned char *dst;
    long long items;                    // B H W
    int H, W;
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

struct FrTap { int i0, i1; double w0, w1; };

NSR_DEV FrTap fr_tap(double s, int in) {
    FrTap t;
    t.i0 = (int)s;
    if (t.i0 > in - 1) t.i0 = in - 1;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.w1 = s - (double)t.i0;
    t.w0 = 1.0 - t.w1;
    return t;
}
NSR_DEV FrTap fr_tap_half_pixel(int dst, double ratio, int in) {
    double s = ratio * ((double)dst + 0.5) - 0.5;
    if (s < 0.0) s = 0.0;
    return fr_tap(s, in);
}
NSR_DEV FrTap fr_tap_corners(int dst, double ratio, int in) { return fr_tap(ratio * (double)dst, in); }
NSR_DEV FrTap fr_tap_at(int i) {
    FrTap t;
    t.i0 = t.i1 = i;
    t.w0 = 1.0;
    t.w1 = 0.0;
    return t;
}

NSR_DEV float fr_depth(const FrameParams &P, long long idx) {
    const float raw = P.depth_f32 ? static_cast<const float *>(P.depth)[idx] : (float)static_cast<const unsigned short *>(P.depth)[idx];
    return (raw / P.png_depth_scale) * P.scale;
}

// pixel (i, j), channel c (file order) of the stage-2 image of one frame
NSR_DEV double fr_stage2(const FrameParams &P, const unsigned char *img, const FrTap &ty, const FrTap &tx, int c) {
    const long long r0 = (long long)ty.i0 * P.Wc, r1 = (long long)ty.i1 * P.Wc;
    const double q00 = (double)img[3 * (r0 + tx.i0) + c] / 255.0;
    if (!P.resize) return q00;
    const double q01 = (double)img[3 * (r0 + tx.i1) + c] / 255.0;
    const double q10 = (double)img[3 * (r1 + tx.i0) + c] / 255.0, q11 = (double)img[3 * (r1 + tx.i1) + c] / 255.0;
    return ty.w0 * (tx.w0 * q00 + tx.w1 * q01) + ty.w1 * (tx.w0 * q10 + tx.w1 * q11);
}

NSR_DEV void fr_stream(const FrameParams &P, long long item) {
    const int groups = (P.W + kFrLane - 1) / kFrLane;
    const long long row = item / groups;
    const int x0 = (int)(item - row * groups) * kFrLane;
    const long long k = row / P.H;
    const int y = (int)(row - k * P.H);
    const long long sp = (k * P.Hd + (y + P.edge)) * P.Wd + (P.edge + x0), dp = row * P.W + x0;
    const int fl = P.bgr ? 2 : 0;
    if (x0 + kFrLane <= P.W) {
        unsigned char px[3 * kFrLane];
        float col[3 * kFrLane], dep[kFrLane];
        __builtin_memcpy(px, P.color + 3 * sp, sizeof(px));
#pragma unroll
        for (int i = 0; i < kFrLane; ++i) {
            col[3 * i] = P.tab[px[3 * i + fl]];
            col[3 * i + 1] = P.tab[px[3 * i + 1]];
            col[3 * i + 2] = P.tab[px[3 * i + 2 - fl]];
        }
        if (P.depth_f32) {
            float raw[kFrLane];
            __builtin_memcpy(raw, static_cast<const float *>(P.depth) + sp, sizeof(raw));
#pragma unroll
            for (int i = 0; i < kFrLane; ++i) dep[i] = (raw[i] / P.png_depth_scale) * P.scale;
        } else {
            unsigned short raw[kFrLane];
            __builtin_memcpy(raw, static_cast<const unsigned short *>(P.depth) + sp, sizeof(raw));
#pragma unroll
            for (int i = 0; i < kFrLane; ++i) dep[i] = ((float)raw[i] / P.png_depth_scale) * P.scale;
        }
        __builtin_memcpy(P.out_color + 3 * dp, col, sizeof(col));
        __builtin_memcpy(P.out_depth + dp, dep, sizeof(dep));
    } else {
        for (int i = 0; x0 + i < P.W; ++i) {              // the row's tail
            const unsigned char *px = P.color + 3 * (sp + i);
            float *o = P.out_color + 3 * (dp + i);
            o[0] = P.tab[px[fl]];
            o[1] = P.tab[px[1]];
            o[2] = P.tab[px[2 - fl]];
            P.out_depth[dp + i] = fr_depth(P, sp + i);
        }
    }
}

NSR_DEV void fr_gather(const FrameParams &P, long long item) {
    const long long row = item / P.W;
    const int x = (int)(item - row * P.W);
    const long long k = row / P.H;
    const int y = (int)(row - k * P.H);
    const int ys = y + P.edge, xs = x + P.edge;          // the stage-4 pixel
    int dy = ys, dx = xs;
    if (P.crop) {
        dy = (int)floorf((float)ys * P.nn_h);
        dx = (int)floorf((float)xs * P.nn_w);
        if (dy > P.Hd - 1) dy = P.Hd - 1;
        if (dx > P.Wd - 1) dx = P.Wd - 1;
    }
    P.out_depth[item] = fr_depth(P, (k * P.Hd + dy) * P.Wd + dx);

    const FrTap cy = P.crop ? fr_tap_corners(ys, P.ac_h, P.Hd) : fr_tap_at(ys);
    const FrTap cx = P.crop ? fr_tap_corners(xs, P.ac_w, P.Wd) : fr_tap_at(xs);
    // the raw rows / columns under the two stage-2 rows / columns this pixel reads
    const FrTap ry0 = P.resize ? fr_tap_half_pixel(cy.i0, P.rs_h, P.Hc) : fr_tap_at(cy.i0);
    const FrTap ry1 = P.resize ? fr_tap_half_pixel(cy.i1, P.rs_h, P.Hc) : fr_tap_at(cy.i1);
    const FrTap rx0 = P.resize ? fr_tap_half_pixel(cx.i0, P.rs_w, P.Wc) : fr_tap_at(cx.i0);
    const FrTap rx1 = P.resize ? fr_tap_half_pixel(cx.i1, P.rs_w, P.Wc) : fr_tap_at(cx.i1);
    const unsigned char *img = P.color + 3 * k * P.Hc * P.Wc;
    float *o = P.out_color + 3 * item;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cs = P.bgr ? 2 - c : c;
        double v = fr_stage2(P, img, ry0, rx0, cs);
        if (P.crop) {
            const double p01 = fr_stage2(P, img, ry0, rx1, cs), p10 = fr_stage2(P, img, ry1, rx0, cs), p11 = fr_stage2(P, img, ry1, rx1, cs);
            v = cy.w0 * (cx.w0 * v + cx.w1 * p01) + cy.w1 * (cx.w0 * p10 + cx.w1 * p11);
        }
        o[c] = (float)v;
    }
}

// one launch per batch: the stream path or the gather path, the same for every lane
NSR_KERNEL NSR_BOUNDS(kFrThreads) void frame_prepare_kernel(const FrameParams P) {
    const long long item = (long long)bid_x() * kFrThreads + tid();
    if (item >= P.items) return;
    if (P.stream) fr_stream(P, item);
    else fr_gather(P, item);
}

NSR_DEV double fr_px(const UndistortParams &P, const unsigned char *img, int yy, int xx, int c) {
    if (yy < 0 || yy >= P.H || xx < 0 || xx >= P.W) return 0.0;
    return (double)img[3 * ((long long)yy * P.W + xx) + c];
}

NSR_KERNEL NSR_BOUNDS(kFrThreads) void frame_undistort_kernel(const UndistortParams P) {
    const long long item = (long long)bid_x() * kFrThreads + tid();
    if (item >= P.items) return;
    const long long row = item / P.W;
    const int u = (int)(item - row * P.W);
    const long long k = row / P.H;
    const int v = (int)(row - k * P.H);
    const double x = ((double)u - P.cx) / P.fx, y = ((double)v - P.cy) / P.fy;
    const double r2 = x * x + y * y;
    const double rad = ((1.0 + P.k1 * r2) + P.k2 * (r2 * r2)) + P.k3 * ((r2 * r2) * r2);
    const double xd = (x * rad + ((2.0 * P.p1) * x) * y) + P.p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * rad + P.p1 * (r2 + (2.0 * y) * y)) + ((2.0 * P.p2) * x) * y;
    const double sx = P.fx * xd + P.cx, sy = P.fy * yd + P.cy;
    unsigned char *o = P.dst + 3 * item;
    if (!(sx > -1.0 && sx < (double)P.W && sy > -1.0 && sy < (double)P.H)) {      // (also a position that is not a number)
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const double fx0 = floor(sx), fy0 = floor(sy);
    const double ax = sx - fx0, ay = sy - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;
    const unsigned char *img = P.src + 3 * k * P.H * P.W;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p00 = fr_px(P, img, y0, x0, c), p01 = fr_px(P, img, y0, x0 + 1, c);
        const double p10 = fr_px(P, img, y0 + 1, x0, c), p11 = fr_px(P, img, y0 + 1, x0 + 1, c);
        const double val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
        const double r = floor(val + 0.5);
        o[c] = (unsigned char)(r > 255.0 ? 255 : (int)r);
    }
}

}  // namespace nsr
