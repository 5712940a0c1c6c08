// nsr_pose.h -- pose algebra of a SLAM run on the device (include/nsr.h, "Pose algebra"): the trajectory [N][4][4] and the
// keyframe pose table stay in device memory, and what the reference does with them on the host between two renders --
// get_tensor_from_camera (src/common.py:179-201), the tracker's motion model (src/Tracker.py:192-201), its choice of the
// iteration with the smallest loss (src/Tracker.py:224,245-247) and the write-back of the bundle-adjusted window
// (src/Mapper.py:527-541) -- is four launches of one small block.  Included by nsr_api.cpp AFTER nsr_kernels.h.
//
// Numerical contract (tests/test_pose_emu.py restates it in numpy):
//   Every input is fp32 and is widened to fp64; all arithmetic is fp64 without contraction, in the association written
//   below; every output is rounded to fp32 once, at its store.
//   Quaternion of a rotation (Shepperd): with t = r00 + r11 + r22
//       t > 0                    s = 2 sqrt(t + 1),             q = (s / 4, (r21 - r12) / s, (r02 - r20) / s, (r10 - r01) / s)
//       r00 > r11 and r00 > r22  s = 2 sqrt(1 + r00 - r11 - r22), q = ((r21 - r12) / s, s / 4, (r01 + r10) / s, (r02 + r20) / s)
//       r11 > r22                s = 2 sqrt(1 + r11 - r00 - r22), q = ((r02 - r20) / s, (r01 + r10) / s, s / 4, (r12 + r21) / s)
//       else                     s = 2 sqrt(1 + r22 - r00 - r11), q = ((r10 - r01) / s, (r02 + r20) / s, (r12 + r21) / s, s / 4)
//   then q / sqrt(((q0 q0 + q1 q1) + q2 q2) + q3 q3); the 7-vector is [w, x, y, z | tx, ty, tz].  Its sign is the branch's.
//   Rotation of a quaternion: quad2rotation in the operation order of camera_from_tensor_kernel (nsr_kernels.h), in fp64.
//   Inverse of a 4x4: Gauss-Jordan on [A | I] with partial pivoting (the first row of the largest |pivot| from the diagonal
//   down), the pivot row divided by the pivot, then eliminated from every other row in increasing row order.
//
// Indices come from device memory (one captured graph serves every frame), so every kernel checks them against the table's
// length and writes nothing for an index outside it.  Plain stores, no atomics, nothing synchronises.
#pragma once

namespace nsr {

constexpr int kPoseThreads = 64;

struct PoseFromParams {
    const float *rt;        // [n][row_floats]: rows of 4, the first three read
    long long n;
    int row_floats;         // 12 or 16
    float *cam;             // [n][7]
};

struct PosePredictParams {
    float *traj;            // [n_frames][4][4]
    long long n_frames;
    const long long *idx;   // the frame to predict
    int const_speed;
    float *cam;             // [7]
};

struct PoseCommitParams {
    const float *hist;      // [n_iters][8]: loss | cam
    int n_iters;
    float *traj;
    long long n_frames;
    const long long *idx;
    float *best;            // [8] or NULL
};

struct PoseStoreParams {
    const float *cams;      // [m][7]
    int m;
    const long long *index; // [m] rows of dst
    float *dst;             // [n_dst][4][4]
    long long n_dst;
};

// m: row-major rotation with row stride 4 -> normalised quaternion (w, x, y, z)
NSR_DEV void pose_quat(const double *m, double *q) {
    const double r00 = m[0], r11 = m[5], r22 = m[10];
    const double t = r00 + r11 + r22;
    if (t > 0.0) {
        const double s = 2.0 * sqrt(t + 1.0);
        q[0] = 0.25 * s; q[1] = (m[9] - m[6]) / s; q[2] = (m[2] - m[8]) / s; q[3] = (m[4] - m[1]) / s;
    } else if (r00 > r11 && r00 > r22) {
        const double s = 2.0 * sqrt(1.0 + r00 - r11 - r22);
        q[0] = (m[9] - m[6]) / s; q[1] = 0.25 * s; q[2] = (m[1] + m[4]) / s; q[3] = (m[2] + m[8]) / s;
    } else if (r11 > r22) {
        const double s = 2.0 * sqrt(1.0 + r11 - r00 - r22);
        q[0] = (m[2] - m[8]) / s; q[1] = (m[1] + m[4]) / s; q[2] = 0.25 * s; q[3] = (m[6] + m[9]) / s;
    } else {
        const double s = 2.0 * sqrt(1.0 + r22 - r00 - r11);
        q[0] = (m[4] - m[1]) / s; q[1] = (m[2] + m[8]) / s; q[2] = (m[6] + m[9]) / s; q[3] = 0.25 * s;
    }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// [quaternion | translation] in fp64 -> the 4x4 pose at `o`, rounded at the store (src/common.py:137-176, bottom row 0 0 0 1)
NSR_DEV void pose_store44(const double *c, float *o) {
    const double qr = c[0], qi = c[1], qj = c[2], qk = c[3];
    const double nn = ((qr * qr + qi * qi) + qj * qj) + qk * qk;
    const double s = 2.0 / nn;
    const double a[9] = {qj * qj + qk * qk, qi * qj - qk * qr, qi * qk + qj * qr,
                         qi * qj + qk * qr, qi * qi + qk * qk, qj * qk - qi * qr,
                         qi * qk - qj * qr, qj * qk + qi * qr, qi * qi + qj * qj};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[r * 4 + k] = (float)((r == k) ? 1.0 - s * a[r * 3 + k] : s * a[r * 3 + k]);
        o[r * 4 + 3] = (float)c[4 + r];
    }
    o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
}

// c = a b, 4x4 row-major, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
NSR_DEV void pose_mul44(const double *a, const double *b, double *c) {
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k)
            c[r * 4 + k] = ((a[r * 4] * b[k] + a[r * 4 + 1] * b[4 + k]) + a[r * 4 + 2] * b[8 + k]) + a[r * 4 + 3] * b[12 + k];
}

// inv = a^-1 (a is overwritten); a singular matrix leaves what the divisions by zero give, as .inverse() of it has no value either
NSR_DEV void pose_inv44(double *a, double *inv) {
    for (int i = 0; i < 16; ++i) inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (fabs(a[r * 4 + c]) > fabs(a[p * 4 + c])) p = r;
        if (p != c)
            for (int k = 0; k < 4; ++k) {
                const double ta = a[c * 4 + k], ti = inv[c * 4 + k];
                a[c * 4 + k] = a[p * 4 + k]; a[p * 4 + k] = ta;
                inv[c * 4 + k] = inv[p * 4 + k]; inv[p * 4 + k] = ti;
            }
        const double d = a[c * 4 + c];
        for (int k = 0; k < 4; ++k) { a[c * 4 + k] /= d; inv[c * 4 + k] /= d; }
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r * 4 + c];
            for (int k = 0; k < 4; ++k) { a[r * 4 + k] -= f * a[c * 4 + k]; inv[r * 4 + k] -= f * inv[c * 4 + k]; }
        }
    }
}

// get_tensor_from_camera (src/common.py:179-201): one block, a lane takes every kPoseThreads-th pose
NSR_KERNEL NSR_BOUNDS(kPoseThreads) void pose_tensor_from_camera_kernel(const PoseFromParams P) {
    for (long long i = tid(); i < P.n; i += kPoseThreads) {
        const float *src = P.rt + i * P.row_floats;
        double m[12], q[4];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = (double)src[k];
        pose_quat(m, q);
        float *o = P.cam + i * 7;
        o[0] = (float)q[0]; o[1] = (float)q[1]; o[2] = (float)q[2]; o[3] = (float)q[3];
        o[4] = (float)m[3]; o[5] = (float)m[7]; o[6] = (float)m[11];
    }
}

// the tracker's initial pose of frame idx (src/Tracker.py:192-201): one lane
NSR_KERNEL NSR_BOUNDS(kPoseThreads) void pose_predict_kernel(const PosePredictParams P) {
    if (tid() != 0) return;
    const long long idx = P.idx[0];
    if (idx < 1 || idx >= P.n_frames) return;
    double pre[16], init[16];
    const float *src = P.traj + (idx - 1) * 16;
    for (int k = 0; k < 16; ++k) pre[k] = (double)src[k];
    if (P.const_speed && idx >= 2) {
        double pp[16], inv[16], delta[16];
        const float *src2 = P.traj + (idx - 2) * 16;
        for (int k = 0; k < 16; ++k) pp[k] = (double)src2[k];
        pose_inv44(pp, inv);
        pose_mul44(pre, inv, delta);
        pose_mul44(delta, pre, init);
    } else {
        for (int k = 0; k < 16; ++k) init[k] = pre[k];
    }
    double c[7];
    pose_quat(init, c);
    c[4] = init[3]; c[5] = init[7]; c[6] = init[11];
    for (int k = 0; k < 7; ++k) P.cam[k] = (float)c[k];
    pose_store44(c, P.traj + idx * 16);       // the pose of the 7-vector the iterations start from
}

// the iteration with the smallest loss (src/Tracker.py:224,245-247): one lane
NSR_KERNEL NSR_BOUNDS(kPoseThreads) void pose_commit_kernel(const PoseCommitParams P) {
    if (tid() != 0) return;
    const long long idx = P.idx[0];
    if (idx < 0 || idx >= P.n_frames) return;
    double low = 1e10;
    int taken = -1;
    for (int i = 0; i < P.n_iters; ++i) {
        const double loss = (double)P.hist[i * 8];
        if (loss < low) { low = loss; taken = i; }        // (false for a NaN)
    }
    if (taken < 0) return;
    const float *row = P.hist + taken * 8;
    double c[7];
    for (int k = 0; k < 7; ++k) c[k] = (double)row[1 + k];
    pose_store44(c, P.traj + idx * 16);
    if (P.best)
        for (int k = 0; k < 8; ++k) P.best[k] = row[k];
}

// the window's poses back into a pose table (src/Mapper.py:527-541): one block, a lane takes every kPoseThreads-th pose
NSR_KERNEL NSR_BOUNDS(kPoseThreads) void pose_store_kernel(const PoseStoreParams P) {
    for (int i = tid(); i < P.m; i += kPoseThreads) {
        const long long at = P.index[i];
        if (at < 0 || at >= P.n_dst) continue;
        double c[7];
        for (int k = 0; k < 7; ++k) c[k] = (double)P.cams[i * 7 + k];
        pose_store44(c, P.dst + at * 16);
    }
}

}  // namespace nsr
