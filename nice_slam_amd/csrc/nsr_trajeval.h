// nsr_trajeval.h -- trajectory evaluation on the device (include/nsr.h, "Trajectory evaluation"): what src/tools/eval_ate.py does with a
// run's two pose lists -- the mask and scale of convert_poses (:239-256), Horn's alignment (:44-78), the statistics of the
// alignment error (:215-223) and the figure of both trajectories (:196-204) -- without the trajectory leaving device memory.
// Included by nsr_api.cpp AFTER nsr_pose.h.
//
// Numerical contract (tests/trajeval_reference.py restates it in numpy):
//   Pairs      frame i <= last[b] is USED iff none of the 16 floats of gt[i] is an infinity or a NaN; the used frames keep their
//              order.  An est pose of a used frame with such a float is counted as bad; any bad pose makes every statistic,
//              rot, trans and the limits NaN.
//   Positions  m_i (estimate), d_i (ground truth) = (double)(t / scale), the division in fp32.
//   Alignment  all in fp64 without contraction.  Means = sum / n.  S = sum of outer(m_i - mean m, d_i - mean d).  The rotation is
//              Horn's: the 4 x 4 symmetric matrix
//                  N = | Sxx+Syy+Szz  Syz-Szy      Szx-Sxz      Sxy-Syx     |
//                      | .            Sxx-Syy-Szz  Sxy+Syx      Szx+Sxz     |
//                      | .            .            -Sxx+Syy-Szz Syz+Szy     |
//                      | .            .            .            -Sxx-Syy+Szz|
//              is diagonalised by cyclic Jacobi rotations (kAteSweeps sweeps of the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
//              Rutishauser's formulas, a zero element skipped); the unit quaternion (w, x, y, z) is the normalised column of the
//              largest diagonal entry (the first of equal ones) and rot its rotation matrix.  This is the proper rotation
//              U S Vh of eval_ate.py:65-69 -- both maximise sum d_i . rot m_i over the rotations -- and its sensitivity is that
//              one's: 1 / (2 (s2 +- s3)) in the singular values of S.  S = 0 (one pair, or all positions equal) gives the identity.
//              trans = mean d - rot mean m, a row as ((r0 m0 + r1 m1) + r2 m2); e_i = sqrt((a0 a0 + a1 a1) + a2 a2) with
//              a = ((r0 m0 + r1 m1) + r2 m2) + trans - d_i.
//   Statistics rmse = sqrt(sum e e / n), mean = sum e / n, std = sqrt(sum (e - mean)^2 / n), min, max, and numpy's median:
//              the element of rank (n - 1) / 2, or with n even (that one + the next) / 2.  The rank is found by radix
//              selection on the bit pattern of e (e >= +0: its bits order like the values), eight rounds of a 256-bin
//              histogram in LDS, so the block needs no memory proportional to n; the next one is the same value if the
//              last round's bin holds more, else the smallest e above it (one more pass).
//   Sums       thread t of the block's kAteThreads takes the frames [t c, (t + 1) c), c = ceil((last + 1) / kAteThreads), in
//              increasing order; the threads' partial sums are folded in a fixed binary tree.  No atomics on global memory,
//              one block per problem, nothing handed between blocks: a record is bit-identical run to run and does not depend
//              on the other problems of the launch.
//
// Record of a problem, kAteRec = 32 doubles:
//    [0] pairs n            [1] dropped ground-truth frames among 0..last   [2] bad estimate poses among the used frames
//    [3] rmse  [4] mean  [5] median  [6] std  [7] min  [8] max
//    [9..17] rot, row-major     [18..20] trans
//    [21] xmin [22] xmax [23] ymin [24] ymax over the ground-truth positions and the ALIGNED estimate positions of the used frames
//    [25] flags: 1 fewer than two pairs (eval_ate.py:140-143 raises), 2 last outside [0, n_frames), 4 a bad estimate pose
//    [26..31] 0
// With flag 2 the record holds 0 pairs, 0 dropped, 0 bad and NaN in [3..24], and nothing else is written; with 0 pairs [3..24] are NaN.
//
// The figure (ate_plot_kernel): u8 [H][W][3]; pixel (r, c) has the centre p = (c + 0.5, r + 0.5).  With the record's limits
// widened like matplotlib's autoscale (equal limits lo == hi first become -0.05, 0.05 if lo == 0, else lo - 0.05 |lo|,
// hi + 0.05 |hi|; then lo - 0.05 (hi - lo), hi + 0.05 (hi - lo)) and the axes box [0.125 W, 0.9 W] x [0.11 H, 0.88 H],
//     X = ax0 + (x - xlo) ((ax1 - ax0) / (xhi - xlo)),   Y = H - (ay0 + (y - ylo) ((ay1 - ay0) / (yhi - ylo))).
// p belongs to the segment a -> b of half-width hw, with u = p - a, s = b - a, dot = ux sx + uy sy, len2 = sx sx + sy sy:
//     dot <= 0       iff ux ux + uy uy <= hw hw                    (a zero-length segment lands here)
//     dot >= len2    iff vx vx + vy vy <= hw hw, v = p - b
//     otherwise      iff (ux sy - uy sx)^2 <= hw hw len2
// (a NaN fails every comparison: such a segment is not drawn).  Segments join consecutive USED frames.  A pixel is blue
// (0, 0, 255) on a segment of the aligned estimate (hw 0.9375), else black on one of the ground truth (hw 0.9375) or of the four
// sides of the axes box (hw 0.5), else white.
#pragma once

namespace nsr {

constexpr int kAteThreads = 256;
constexpr int kAteRec = 32;
constexpr int kAteSweeps = 12;
constexpr int kAteLds = 9 * kAteThreads * 8;          // the widest reduction: nine doubles per thread
constexpr int kPlotThreads = 256;
constexpr int kPlotLds = kPlotThreads * (4 * 8 + 4);  // a chunk of frames: four doubles and a flag each
static_assert(kAteThreads == 256, "a thread owns one bin of the selection histogram");

struct AteParams {
    const float *est, *gt;      // [n_frames][4][4]
    long long n_frames;
    const long long *last;      // [B] inclusive last frames
    float scale;
    double *rec;                // [B][kAteRec]
    double *err;                // [B][n_frames] or NULL: e of the used frames in their order; the rest is left alone
};

struct AtePlotParams {
    const float *est, *gt;
    long long n_frames;
    const long long *last;      // the problem's entry
    float scale;
    const double *rec;          // the problem's record
    unsigned char *out;         // [H][W][3]
    int H, W;
};

NSR_DEV bool ate_finite16(const float *p) {
    bool ok = true;
    for (int k = 0; k < 16; ++k) ok = ok && ((__builtin_bit_cast(unsigned, p[k]) & 0x7f800000u) != 0x7f800000u);
    return ok;
}

NSR_DEV void ate_position(const float *pose, float scale, double *x) {
    x[0] = (double)(pose[3] / scale);
    x[1] = (double)(pose[7] / scale);
    x[2] = (double)(pose[11] / scale);
}

// frame i of a problem: false if it is dropped, else its two positions
template <typename Params>
NSR_DEV bool ate_pair(const Params &P, long long i, double *m, double *d) {
    if (!ate_finite16(P.gt + i * 16)) return false;
    ate_position(P.est + i * 16, P.scale, m);
    ate_position(P.gt + i * 16, P.scale, d);
    return true;
}

// rot (row-major) m + trans
NSR_DEV void ate_apply(const double *rot, const double *trans, const double *m, double *a) {
    for (int r = 0; r < 3; ++r) a[r] = ((rot[3 * r] * m[0] + rot[3 * r + 1] * m[1]) + rot[3 * r + 2] * m[2]) + trans[r];
}

NSR_DEV double ate_error(const double *rot, const double *trans, const double *m, const double *d) {
    double a[3];
    ate_apply(rot, trans, m, a);
    const double x = a[0] - d[0], y = a[1] - d[1], z = a[2] - d[2];
    return sqrt((x * x + y * y) + z * z);
}

// OP 0: sum, 1: min, 2: max (fmin / fmax: a NaN does not win) of K values per thread, the same pairing whatever the values;
// every thread gets the results
template <int K, int OP>
NSR_DEV void ate_reduce(double *red, double *v, int t) {
    block_sync();                                      // the previous use of `red` has been read
    for (int k = 0; k < K; ++k) red[k * kAteThreads + t] = v[k];
    block_sync();
    for (int w = kAteThreads / 2; w >= 1; w >>= 1) {
        if (t < w)
            for (int k = 0; k < K; ++k) {
                const double a = red[k * kAteThreads + t], b = red[k * kAteThreads + t + w];
                red[k * kAteThreads + t] = OP == 0 ? a + b : (OP == 1 ? fmin(a, b) : fmax(a, b));
            }
        block_sync();
    }
    for (int k = 0; k < K; ++k) v[k] = red[k * kAteThreads];
}

// Horn's rotation of S (row-major, S[3 i + j] = sum m_i d_j): one lane
NSR_DEV void ate_horn(const double *S, double *rot) {
    double a[4][4], v[4][4];
    a[0][0] = (S[0] + S[4]) + S[8];
    a[1][1] = (S[0] - S[4]) - S[8];
    a[2][2] = (S[4] - S[0]) - S[8];
    a[3][3] = (S[8] - S[0]) - S[4];
    a[0][1] = a[1][0] = S[5] - S[7];
    a[0][2] = a[2][0] = S[6] - S[2];
    a[0][3] = a[3][0] = S[1] - S[3];
    a[1][2] = a[2][1] = S[1] + S[3];
    a[1][3] = a[3][1] = S[6] + S[2];
    a[2][3] = a[3][2] = S[5] + S[7];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kAteSweeps; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double tn = theta < 0.0 ? -tt : tt;
                const double c = 1.0 / sqrt(tn * tn + 1.0), s = tn * c;
                for (int k = 0; k < 4; ++k) {              // A := A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {              // A := J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = 0.0;
                a[q][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
    double best = a[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
    for (int i = 1; i < 4; ++i)                            // (no run-time index: the matrices stay in registers)
        if (a[i][i] > best) { best = a[i][i]; qw = v[0][i]; qx = v[1][i]; qy = v[2][i]; qz = v[3][i]; }
    const double nn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw /= nn; qx /= nn; qy /= nn; qz /= nn;
    rot[0] = 1.0 - 2.0 * (qy * qy + qz * qz); rot[1] = 2.0 * (qx * qy - qw * qz); rot[2] = 2.0 * (qx * qz + qw * qy);
    rot[3] = 2.0 * (qx * qy + qw * qz); rot[4] = 1.0 - 2.0 * (qx * qx + qz * qz); rot[5] = 2.0 * (qy * qz - qw * qx);
    rot[6] = 2.0 * (qx * qz - qw * qy); rot[7] = 2.0 * (qy * qz + qw * qx); rot[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
}

// the e of rank `rank` (0-based) among the used frames of [lo, hi) of every thread: radix selection, most significant byte first.
// A round's 256 bins are walked in two levels (16 sums of 16 bins, then one group's bins): 31 dependent LDS reads, not 255.
// *next_same: the element of rank + 1 has the same value.
NSR_DEV double ate_select(const AteParams &P, const double *rot, const double *trans, long long lo, long long hi, long long rank,
                          int *hist, int t, bool *next_same) {
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        block_sync();                                  // the previous round's histogram has been read
        hist[t] = 0;
        block_sync();
        const unsigned long long high = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (long long i = lo; i < hi; ++i) {
            double m[3], d[3];
            if (!ate_pair(P, i, m, d)) continue;
            const unsigned long long key = __builtin_bit_cast(unsigned long long, ate_error(rot, trans, m, d));
            if ((key & high) == prefix) atomic_add_lds_i(hist + (int)((key >> shift) & 255u), 1);
        }
        block_sync();
        if (t < 16) {
            int sum = 0;
            for (int k = 0; k < 16; ++k) sum += lds_load_i(hist + 16 * t + k);
            hist[kAteThreads + t] = sum;
        }
        block_sync();
        long long before = 0;
        int group = 0;
        for (; group < 15; ++group) {
            const int h = lds_load_i(hist + kAteThreads + group);
            if (before + h > rank) break;
            before += h;
        }
        int bin = 16 * group;
        for (; bin < 16 * group + 15; ++bin) {
            const int h = lds_load_i(hist + bin);
            if (before + h > rank) break;
            before += h;
        }
        rank -= before;
        prefix |= (unsigned long long)bin << shift;
        if (shift == 0) *next_same = rank + 1 < lds_load_i(hist + bin);
    }
    return __builtin_bit_cast(double, prefix);
}

// one block per problem
NSR_KERNEL NSR_BOUNDS(kAteThreads) void ate_eval_kernel(const AteParams P) {
    double *red = reinterpret_cast<double *>(lds_base());
    int *hist = reinterpret_cast<int *>(lds_base());
    const int t = tid();
    const long long b = bid_x();
    double *rec = P.rec + b * kAteRec;
    const long long last = P.last[b];
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    if (last < 0 || last >= P.n_frames) {              // (the whole block leaves: no barrier is left waiting)
        if (t < kAteRec) rec[t] = t < 3 ? 0.0 : (t < 25 ? qnan : (t == 25 ? 3.0 : 0.0));
        return;
    }
    const long long L = last + 1, c = (L + kAteThreads - 1) / kAteThreads;
    const long long lo = t * c < L ? t * c : L, hi = lo + c < L ? lo + c : L;

    // 1: the pairs and the means
    double s1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};        // used, bad, sum m, sum d, frames
    for (long long i = lo; i < hi; ++i) {
        s1[8] += 1.0;
        if (!ate_finite16(P.gt + i * 16)) continue;
        s1[0] += 1.0;
        if (!ate_finite16(P.est + i * 16)) s1[1] += 1.0;
        double m[3], d[3];
        ate_position(P.est + i * 16, P.scale, m);
        ate_position(P.gt + i * 16, P.scale, d);
        for (int k = 0; k < 3; ++k) { s1[2 + k] += m[k]; s1[5 + k] += d[k]; }
    }
    const long long mine = (long long)s1[0];
    ate_reduce<9, 0>(red, s1, t);
    const double n = s1[0], bad = s1[1];
    const long long pairs = (long long)n;
    const double flags = (pairs < 2 ? 1.0 : 0.0) + (bad > 0.0 ? 4.0 : 0.0);
    if (t == 0) {
        rec[0] = n; rec[1] = s1[8] - n; rec[2] = bad; rec[25] = flags;
        for (int k = 26; k < kAteRec; ++k) rec[k] = 0.0;
    }
    if (pairs == 0 || bad > 0.0) {
        if (t >= 3 && t < 25) rec[t] = qnan;
        return;
    }
    double mm[3], dm[3];
    for (int k = 0; k < 3; ++k) { mm[k] = s1[2 + k] / n; dm[k] = s1[5 + k] / n; }

    // where this thread's used frames start in the compacted order
    long long first = 0;
    if (P.err) {
        block_sync();
        red[t] = (double)mine;
        block_sync();
        for (int k = 0; k < t; ++k) first += (long long)red[k];
    }

    // 2: S, then the rotation (every thread forms it from the same S: no broadcast)
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = lo; i < hi; ++i) {
        double m[3], d[3];
        if (!ate_pair(P, i, m, d)) continue;
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) S[3 * r + k] += (m[r] - mm[r]) * (d[k] - dm[k]);
    }
    ate_reduce<9, 0>(red, S, t);
    double rot[9], trans[3];
    ate_horn(S, rot);
    for (int r = 0; r < 3; ++r) trans[r] = dm[r] - ((rot[3 * r] * mm[0] + rot[3 * r + 1] * mm[1]) + rot[3 * r + 2] * mm[2]);

    // 3: the errors, their sums and extremes, the data limits
    const double inf = __builtin_bit_cast(double, 0x7ff0000000000000ull);
    double sum[2] = {0, 0}, mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    long long at = first;
    for (long long i = lo; i < hi; ++i) {
        double m[3], d[3], a[3];
        if (!ate_pair(P, i, m, d)) continue;
        const double e = ate_error(rot, trans, m, d);
        ate_apply(rot, trans, m, a);
        if (P.err) P.err[b * P.n_frames + at++] = e;
        sum[0] += e;
        sum[1] += e * e;
        mn[0] = fmin(mn[0], e); mx[0] = fmax(mx[0], e);
        mn[1] = fmin(mn[1], fmin(a[0], d[0])); mx[1] = fmax(mx[1], fmax(a[0], d[0]));
        mn[2] = fmin(mn[2], fmin(a[1], d[1])); mx[2] = fmax(mx[2], fmax(a[1], d[1]));
    }
    ate_reduce<2, 0>(red, sum, t);
    ate_reduce<3, 1>(red, mn, t);
    ate_reduce<3, 2>(red, mx, t);
    const double mean = sum[0] / n;

    // 4: the population variance about the mean
    double var[1] = {0};
    for (long long i = lo; i < hi; ++i) {
        double m[3], d[3];
        if (!ate_pair(P, i, m, d)) continue;
        const double dv = ate_error(rot, trans, m, d) - mean;
        var[0] += dv * dv;
    }
    ate_reduce<1, 0>(red, var, t);

    // 5: the median; with an even count the next element is the same value (a tie) or the smallest one above it
    bool same = false;
    double med = ate_select(P, rot, trans, lo, hi, (pairs - 1) / 2, hist, t, &same);
    if ((pairs & 1) == 0) {
        double next[1] = {same ? med : inf};
        if (!same)
            for (long long i = lo; i < hi; ++i) {
                double m[3], d[3];
                if (!ate_pair(P, i, m, d)) continue;
                const double e = ate_error(rot, trans, m, d);
                if (e > med) next[0] = fmin(next[0], e);
            }
        ate_reduce<1, 1>(red, next, t);
        med = (med + next[0]) / 2.0;
    }

    if (t == 0) {
        rec[3] = sqrt(sum[1] / n); rec[4] = mean; rec[5] = med; rec[6] = sqrt(var[0] / n); rec[7] = mn[0]; rec[8] = mx[0];
        for (int k = 0; k < 9; ++k) rec[9 + k] = rot[k];
        for (int k = 0; k < 3; ++k) rec[18 + k] = trans[k];
        rec[21] = mn[1]; rec[22] = mx[1]; rec[23] = mn[2]; rec[24] = mx[2];
    }
}

// matplotlib's view limits of the data limits [lo, hi]
NSR_DEV void plot_limits(double lo, double hi, double *out) {
    if (hi == lo) {
        if (lo == 0.0) { lo = -0.05; hi = 0.05; }
        else { lo = lo - 0.05 * fabs(lo); hi = hi + 0.05 * fabs(hi); }
    }
    const double d = (hi - lo) * 0.05;
    out[0] = lo - d;
    out[1] = hi + d;
}

NSR_DEV bool plot_on_segment(double px, double py, double ax, double ay, double bx, double by, double hw2) {
    const double sx = bx - ax, sy = by - ay, ux = px - ax, uy = py - ay;
    const double dot = ux * sx + uy * sy, len2 = sx * sx + sy * sy;
    if (dot <= 0.0) return ux * ux + uy * uy <= hw2;
    if (dot >= len2) {
        const double vx = px - bx, vy = py - by;
        return vx * vx + vy * vy <= hw2;
    }
    const double cr = ux * sy - uy * sx;
    return cr * cr <= hw2 * len2;
}

// a thread per pixel; the block walks the frames in chunks of kPlotThreads staged in LDS as display coordinates
NSR_KERNEL NSR_BOUNDS(kPlotThreads) void ate_plot_kernel(const AtePlotParams P) {
    double *pts = reinterpret_cast<double *>(lds_base());                 // [kPlotThreads][4]: ground truth X, Y, estimate X, Y
    int *used = reinterpret_cast<int *>(pts + 4 * kPlotThreads);
    const int t = tid();
    const long long pix = (long long)bid_x() * kPlotThreads + t;
    const int r = (int)(pix / P.W), c = (int)(pix - (long long)r * P.W);
    const double px = (double)c + 0.5, py = (double)r + 0.5;
    const double W = (double)P.W, H = (double)P.H;
    const double ax0 = 0.125 * W, ax1 = 0.9 * W, ay0 = 0.11 * H, ay1 = 0.88 * H;
    const double top = H - ay1, bot = H - ay0;
    const double hwf = 0.5 * 0.5, hwt = 0.9375 * 0.9375;
    bool black = plot_on_segment(px, py, ax0, bot, ax1, bot, hwf) || plot_on_segment(px, py, ax1, bot, ax1, top, hwf) ||
                 plot_on_segment(px, py, ax1, top, ax0, top, hwf) || plot_on_segment(px, py, ax0, top, ax0, bot, hwf);
    bool blue = false;

    const long long last = P.last[0];
    const long long L = (last < 0 || last >= P.n_frames) ? 0 : last + 1;
    double rot[9], trans[3], xl[2], yl[2];
    for (int k = 0; k < 9; ++k) rot[k] = P.rec[9 + k];
    for (int k = 0; k < 3; ++k) trans[k] = P.rec[18 + k];
    plot_limits(P.rec[21], P.rec[22], xl);
    plot_limits(P.rec[23], P.rec[24], yl);
    const double kx = (ax1 - ax0) / (xl[1] - xl[0]), ky = (ay1 - ay0) / (yl[1] - yl[0]);

    bool have = false;
    double g0 = 0, g1 = 0, e0 = 0, e1 = 0;                                  // the previous used frame
    for (long long base = 0; base < L; base += kPlotThreads) {
        block_sync();                                                      // the previous chunk has been read
        const long long i = base + t;
        int u = 0;
        double m[3], d[3], a[3];
        if (i < L && ate_pair(P, i, m, d)) {
            ate_apply(rot, trans, m, a);
            pts[4 * t] = ax0 + (d[0] - xl[0]) * kx;
            pts[4 * t + 1] = H - (ay0 + (d[1] - yl[0]) * ky);
            pts[4 * t + 2] = ax0 + (a[0] - xl[0]) * kx;
            pts[4 * t + 3] = H - (ay0 + (a[1] - yl[0]) * ky);
            u = 1;
        }
        used[t] = u;
        block_sync();
        const int count = L - base < kPlotThreads ? (int)(L - base) : kPlotThreads;
        for (int k = 0; k < count; ++k) {
            if (!used[k]) continue;
            const double n0 = pts[4 * k], n1 = pts[4 * k + 1], n2 = pts[4 * k + 2], n3 = pts[4 * k + 3];
            if (have) {
                black = black || plot_on_segment(px, py, g0, g1, n0, n1, hwt);
                blue = blue || plot_on_segment(px, py, e0, e1, n2, n3, hwt);
            }
            g0 = n0; g1 = n1; e0 = n2; e1 = n3;
            have = true;
        }
    }
    if (pix < (long long)P.H * P.W) {
        unsigned char *o = P.out + 3 * pix;
        o[0] = blue ? 0 : (black ? 0 : 255);
        o[1] = o[0];
        o[2] = blue ? 255 : o[0];
    }
}

}  // namespace nsr
