// nsr_bound.h -- the mesh bound from keyframes (include/nsr.h, "Mesh bound from keyframes"): TSDF fusion of the keyframes'
// depth, the surface points of that volume, a pre-filter for the convex hull, an exact fp64 quickhull on the host, and the
// point-in-hull test (src/utils/Mesher.py:214-279, get_bound_from_frames, and its two uses in get_mesh, :420-433 / :468-482).
// Included by nsr_api.cpp AFTER nsr_kernels.h, whose device primitives (nsr_dev.h, or the CPU emulator's shadow of it) it uses.
//
// The contract restates Open3D's legacy ScalableTSDFVolume as the reference configures it: volume unit = 16^3 voxels,
// depth_sampling_stride = 4, voxel_length vl = 4 scale / 512, sdf_trunc = 0.04 scale, depth_scale = 1, depth_trunc = 1000.
// Geometry only: the reference fuses colour too, but the hull reads nothing but vertex positions, so no colour is integrated.
//   Poses     the caller flips c2w as the reference does (c2w[:3,1] *= -1, c2w[:3,2] *= -1), passes that c2w in fp64 for the
//             back-projection and w2c = inv(c2w) computed in fp64 and rounded to fp32 for the integration.
//   Depth     a pixel is valid iff 0 < d <= depth_trunc (what create_from_color_and_depth leaves non-zero).
//   Touched units  every 4th pixel along each image axis (u, v = 0, 4, 8, ...) with valid depth is back-projected in fp64:
//             pc = (((u - cx) d) / fx, ((v - cy) d) / fy, d), p = ((R0 pc.x + R1 pc.y) + R2 pc.z) + t per row.  Frame k touches
//             every unit (index floor(x / (16 vl)) per axis) that the box p +- sdf_trunc intersects: floor((p -+ trunc) / (16 vl)).
//             A voxel is updated by frame k only if its unit is touched by frame k (Open3D's per-(unit, frame) rule).  Data:
//             a dense unit bitmap over the box of all touched units (atomicOr), its rank (per-word popcount prefix), the unit
//             list in linear-index order, per-unit touch bits per frame (atomicOr: order-independent).
//   Integration  voxel centre c = (double)U 16 vl + ((double)l + 0.5) vl in fp64, rounded to fp32; p_cam = w2c c in fp32,
//             ((w0 x + w1 y) + w2 z) + w3; skip z <= 0.  Nearest pixel: u = (x / z) fx + cx, v = (y / z) fy + cy in fp32,
//             rounded half up: ui = floor(u + 0.5f); skip when off-image or the depth is not valid.
//             sdf = (d - z) sqrtf((1 + a a) + b b), a = (ui - cx) / fx, b = (vi - cy) / fy (fp32); if sdf >= -trunc:
//             tsdf <- (tsdf w + min(1, sdf / trunc)) / (w + 1), w <- w + 1.  One block per touched unit, frames in keyframe
//             order inside the kernel, every voxel written once: no atomics, bit-identical run to run.
//   Surface points  the vertex set of Open3D's extract_triangle_mesh: a point on every voxel edge (G, G + e_a) whose TSDF
//             changes sign ((f0 < 0) != (f1 < 0)) and that belongs to at least one cube whose 8 corners all have weight > 0;
//             at c(G) + |f0| / (|f0| + |f1|) vl along a (fp64).  Order: units in list order, voxels in linear order
//             (x slowest), axes x, y, z.  Cubes cross unit borders through the neighbour units.
//   Pre-filter  the extreme point along each of the 26 directions (a, b, c) in {-1, 0, 1}^3 \ 0 (score ((a x + b y) + c z) in
//             fp64, ties -> smallest index, blocks combined in order); the caller hulls those extremes and drops every point
//             whose signed distance to every plane of that hull is < -margin: it is strictly inside the hull of all points.
//   Exact hull  host fp64 quickhull (hull_build below); contains: fp64 ((nx x + ny y) + nz z) + off <= 0 for every plane.
#pragma once
#include <unordered_map>
#include <vector>

namespace nsr {

constexpr int kTsdfUnit = 16;                    // voxels per unit edge
constexpr int kTsdfVox = kTsdfUnit * kTsdfUnit * kTsdfUnit;
constexpr int kTsdfStride = 4;                   // depth_sampling_stride
constexpr int kTsdfThreads = 256;                // integrate / surface: 16 voxels per thread
constexpr int kTsdfPerThread = kTsdfVox / kTsdfThreads;
constexpr int kBitsPerBlock = 256;               // words per block of the bitmap rank
constexpr int kHullDirs = 26;
constexpr int kHullBlocks = 256;
constexpr int kHullMaxPlanes = 64;               // the hull of 26 extremes has at most 2 * 26 - 4 = 48 faces
constexpr int kContainsChunk = 1024;             // planes per LDS chunk (32 KB)
constexpr float kDepthTrunc = 1000.f;

#if defined(__HIP__)
NSR_DEV void bnd_atomic_or(unsigned *p, unsigned v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
NSR_DEV void bnd_atomic_min(int *p, int v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
NSR_DEV void bnd_atomic_max(int *p, int v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
inline void bnd_atomic_or(unsigned *p, unsigned v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline void bnd_atomic_min(int *p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
inline void bnd_atomic_max(int *p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}
#endif

struct TsdfParams {
    const float *depth;              // [K][H][W]
    int K, H, W, su, sv;             // su, sv: sampled columns / rows
    long long npts;                  // K * sv * su sampled pixels
    const double *c2w;               // [K][12] fp64 rows 0..2 of the flipped c2w (back-projection)
    const float *w2c;                // [K][12] fp32 rows 0..2 of inv(c2w) (integration)
    double fx, fy, cx, cy, vl, ul, trunc;
    float fxf, fyf, cxf, cyf, truncf;
    int *box;                        // [6] device: unit box lo xyz, hi xyz (inclusive)
    int lo[3], dim[3];               // HOST copy of the box
    long long nbits, nwords, nwblocks;
    unsigned *bitmap;                // [nwords]
    int *wprefix;                    // [nwords] units before word w
    long long *bsum;                 // [nwblocks] units before word block b
    long long *nunits;               // [1] out
    long long n_units;
    int *units;                      // [n_units][3] absolute unit index
    unsigned *touch;                 // [n_units][tw]
    int tw;
    float *tsdf, *weight;            // [n_units][4096]
    long long *counts;               // [n_units + 1] surface points per unit -> exclusive scan, total at n_units
    double *points;                  // [total][3]
};

NSR_DEV int bnd_floor_int(double x) {
    double f = floor(x);
    if (!(f > -1073741824.0)) f = -1073741824.0;                     // NaN or far away: the host rejects such a box
    if (f > 1073741824.0) f = 1073741824.0;
    return (int)f;
}

// the back-projection of sampled pixel s (frame k); false when its depth is not valid
NSR_DEV bool tsdf_point(const TsdfParams &P, long long s, int &k, double p[3]) {
    const long long per = (long long)P.su * P.sv;
    k = (int)(s / per);
    const long long r = s - (long long)k * per;
    const int v = (int)(r / P.su) * kTsdfStride, u = (int)(r % P.su) * kTsdfStride;
    const float df = P.depth[((long long)k * P.H + v) * P.W + u];
    if (!(df > 0.f && df <= kDepthTrunc)) return false;
    const double d = (double)df;
    const double pc[3] = {(((double)u - P.cx) * d) / P.fx, (((double)v - P.cy) * d) / P.fy, d};
    const double *m = P.c2w + 12ll * k;
    for (int i = 0; i < 3; ++i) p[i] = ((m[4 * i] * pc[0] + m[4 * i + 1] * pc[1]) + m[4 * i + 2] * pc[2]) + m[4 * i + 3];
    return true;
}

NSR_DEV void tsdf_unit_range(const TsdfParams &P, const double p[3], int a[3], int b[3]) {
    for (int i = 0; i < 3; ++i) { a[i] = bnd_floor_int((p[i] - P.trunc) / P.ul); b[i] = bnd_floor_int((p[i] + P.trunc) / P.ul); }
}

NSR_KERNEL void tsdf_box_init_kernel(const TsdfParams P) {
    if (tid() < 3) { P.box[tid()] = 2147483647; P.box[3 + tid()] = -2147483647 - 1; }
}

NSR_KERNEL void tsdf_box_kernel(const TsdfParams P) {
    int a[3], b[3], lo[3] = {2147483647, 2147483647, 2147483647}, hi[3] = {-2147483647 - 1, -2147483647 - 1, -2147483647 - 1};
    bool any = false;
    for (long long s = (long long)bid_x() * nthreads() + tid(); s < P.npts; s += (long long)nblk_x() * nthreads()) {
        int k;
        double p[3];
        if (!tsdf_point(P, s, k, p)) continue;
        tsdf_unit_range(P, p, a, b);
        for (int i = 0; i < 3; ++i) { lo[i] = a[i] < lo[i] ? a[i] : lo[i]; hi[i] = b[i] > hi[i] ? b[i] : hi[i]; }
        any = true;
    }
    if (any)
        for (int i = 0; i < 3; ++i) { bnd_atomic_min(P.box + i, lo[i]); bnd_atomic_max(P.box + 3 + i, hi[i]); }
}

NSR_DEV long long tsdf_linear(const TsdfParams &P, int ux, int uy, int uz) {
    const int x = ux - P.lo[0], y = uy - P.lo[1], z = uz - P.lo[2];
    if (x < 0 || y < 0 || z < 0 || x >= P.dim[0] || y >= P.dim[1] || z >= P.dim[2]) return -1;
    return ((long long)x * P.dim[1] + y) * P.dim[2] + z;
}

// compact id of a unit, -1 when it is not touched (or outside the box)
NSR_DEV long long tsdf_rank(const TsdfParams &P, int ux, int uy, int uz) {
    const long long L = tsdf_linear(P, ux, uy, uz);
    if (L < 0) return -1;
    const unsigned w = P.bitmap[L >> 5], bit = 1u << (L & 31);
    if (!(w & bit)) return -1;
    return (long long)P.wprefix[L >> 5] + __builtin_popcount(w & (bit - 1u));
}

NSR_KERNEL void tsdf_clear_kernel(const TsdfParams P) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i < P.nwords) P.bitmap[i] = 0u;
}

NSR_KERNEL void tsdf_mark_kernel(const TsdfParams P) {
    const long long s = (long long)bid_x() * nthreads() + tid();
    if (s >= P.npts) return;
    int k, a[3], b[3];
    double p[3];
    if (!tsdf_point(P, s, k, p)) return;
    tsdf_unit_range(P, p, a, b);
    for (int x = a[0]; x <= b[0]; ++x)
        for (int y = a[1]; y <= b[1]; ++y)
            for (int z = a[2]; z <= b[2]; ++z) {
                const long long L = tsdf_linear(P, x, y, z);
                if (L < 0) continue;                                   // cannot happen for the box this pass was sized by
                const unsigned bit = 1u << (L & 31);
                if (!(P.bitmap[L >> 5] & bit)) bnd_atomic_or(P.bitmap + (L >> 5), bit);
            }
}

// per block of kBitsPerBlock words: exclusive popcount prefix inside the block, block total into bsum
NSR_KERNEL void tsdf_wscan_kernel(const TsdfParams P) {
    int *cnt = reinterpret_cast<int *>(lds_base());                   // [kBitsPerBlock]
    const long long w = (long long)bid_x() * kBitsPerBlock + tid();
    cnt[tid()] = w < P.nwords ? __builtin_popcount(P.bitmap[w]) : 0;
    block_sync();
    if (tid() == 0) {
        int run = 0;
        for (int j = 0; j < kBitsPerBlock; ++j) { const int c = cnt[j]; cnt[j] = run; run += c; }
        P.bsum[bid_x()] = run;
    }
    block_sync();
    if (w < P.nwords) P.wprefix[w] = cnt[tid()];
}

NSR_KERNEL void tsdf_bscan_kernel(const TsdfParams P) {
    if (tid() != 0) return;
    long long run = 0;
    for (long long b = 0; b < P.nwblocks; ++b) { const long long c = P.bsum[b]; P.bsum[b] = run; run += c; }
    P.nunits[0] = run;
}

NSR_KERNEL void tsdf_wfix_kernel(const TsdfParams P) {
    const long long w = (long long)bid_x() * nthreads() + tid();
    if (w < P.nwords) P.wprefix[w] = (int)(P.bsum[w / kBitsPerBlock] + P.wprefix[w]);
}

NSR_KERNEL void tsdf_units_kernel(const TsdfParams P) {
    const long long w = (long long)bid_x() * nthreads() + tid();
    if (w >= P.nwords) return;
    const unsigned word = P.bitmap[w];
    long long id = P.wprefix[w];
    for (int j = 0; j < 32; ++j) {
        if (!(word & (1u << j))) continue;
        const long long L = 32 * w + j;
        if (id < P.n_units) {
            const long long yz = (long long)P.dim[1] * P.dim[2];
            P.units[3 * id] = (int)(L / yz) + P.lo[0];
            P.units[3 * id + 1] = (int)((L / P.dim[2]) % P.dim[1]) + P.lo[1];
            P.units[3 * id + 2] = (int)(L % P.dim[2]) + P.lo[2];
            for (int t = 0; t < P.tw; ++t) P.touch[id * P.tw + t] = 0u;
        }
        ++id;
    }
}

NSR_KERNEL void tsdf_touch_kernel(const TsdfParams P) {
    const long long s = (long long)bid_x() * nthreads() + tid();
    if (s >= P.npts) return;
    int k, a[3], b[3];
    double p[3];
    if (!tsdf_point(P, s, k, p)) return;
    tsdf_unit_range(P, p, a, b);
    const unsigned bit = 1u << (k & 31);
    for (int x = a[0]; x <= b[0]; ++x)
        for (int y = a[1]; y <= b[1]; ++y)
            for (int z = a[2]; z <= b[2]; ++z) {
                const long long id = tsdf_rank(P, x, y, z);
                if (id < 0 || id >= P.n_units) continue;
                unsigned *word = P.touch + id * P.tw + (k >> 5);
                if (!(*word & bit)) bnd_atomic_or(word, bit);
            }
}

NSR_DEV float tsdf_centre(const TsdfParams &P, int u, int l) { return (float)((double)u * P.ul + ((double)l + 0.5) * P.vl); }

// one block per touched unit; thread t owns voxels v = t + 256 j (x = j, y = t / 16, z = t % 16), frames in keyframe order
NSR_KERNEL void tsdf_integrate_kernel(const TsdfParams P) {
    const long long c = bid_x();
    const int t = tid();
    const int *U = P.units + 3 * c;
    const int ly = t >> 4, lz = t & 15;
    const float py = tsdf_centre(P, U[1], ly), pz = tsdf_centre(P, U[2], lz);
    float px[kTsdfPerThread], ts[kTsdfPerThread], ws[kTsdfPerThread];
#pragma unroll
    for (int j = 0; j < kTsdfPerThread; ++j) { px[j] = tsdf_centre(P, U[0], j); ts[j] = 0.f; ws[j] = 0.f; }
    for (int k = 0; k < P.K; ++k) {
        if (!((P.touch[c * P.tw + (k >> 5)] >> (k & 31)) & 1u)) continue;     // block-uniform
        const float *m = P.w2c + 12ll * k;
        const float *dk = P.depth + (long long)k * P.H * P.W;
#pragma unroll                                                        // the per-voxel arrays stay in registers
        for (int j = 0; j < kTsdfPerThread; ++j) {
            const float X = ((m[0] * px[j] + m[1] * py) + m[2] * pz) + m[3];
            const float Y = ((m[4] * px[j] + m[5] * py) + m[6] * pz) + m[7];
            const float Z = ((m[8] * px[j] + m[9] * py) + m[10] * pz) + m[11];
            if (!(Z > 0.f)) continue;
            const float uu = (X / Z) * P.fxf + P.cxf + 0.5f, vv = (Y / Z) * P.fyf + P.cyf + 0.5f;
            if (!(uu >= 0.f && uu < (float)P.W && vv >= 0.f && vv < (float)P.H)) continue;
            const int ui = (int)floorf(uu), vi = (int)floorf(vv);
            const float d = dk[(long long)vi * P.W + ui];
            if (!(d > 0.f && d <= kDepthTrunc)) continue;
            const float a = ((float)ui - P.cxf) / P.fxf, b = ((float)vi - P.cyf) / P.fyf;
            const float sdf = (d - Z) * sqrtf((1.f + a * a) + b * b);
            if (!(sdf >= -P.truncf)) continue;
            float s = sdf / P.truncf;
            s = s < 1.f ? s : 1.f;
            ts[j] = (ts[j] * ws[j] + s) / (ws[j] + 1.f);
            ws[j] = ws[j] + 1.f;
        }
    }
#pragma unroll
    for (int j = 0; j < kTsdfPerThread; ++j) {
        P.tsdf[c * kTsdfVox + j * kTsdfThreads + t] = ts[j];
        P.weight[c * kTsdfVox + j * kTsdfThreads + t] = ws[j];
    }
}

// tsdf / weight of global voxel g (weight 0 outside the touched units)
NSR_DEV float tsdf_voxel(const TsdfParams &P, const int g[3], float &f) {
    int u[3], l[3];
    for (int i = 0; i < 3; ++i) { u[i] = g[i] >= 0 ? g[i] / kTsdfUnit : -((-g[i] + kTsdfUnit - 1) / kTsdfUnit); l[i] = g[i] - u[i] * kTsdfUnit; }
    const long long id = tsdf_rank(P, u[0], u[1], u[2]);
    if (id < 0 || id >= P.n_units) { f = 0.f; return 0.f; }
    const long long i = id * kTsdfVox + (l[0] * kTsdfUnit + l[1]) * kTsdfUnit + l[2];
    f = P.tsdf[i];
    return P.weight[i];
}

// does the edge (g, g + e_a) carry a surface point?  (t: |f0| / (|f0| + |f1|))
NSR_DEV bool tsdf_edge(const TsdfParams &P, const int g[3], int a, double &t) {
    float f0, f1;
    if (!(tsdf_voxel(P, g, f0) > 0.f)) return false;
    int h[3] = {g[0], g[1], g[2]};
    ++h[a];
    if (!(tsdf_voxel(P, h, f1) > 0.f)) return false;
    if ((f0 < 0.f) == (f1 < 0.f)) return false;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    for (int ob = 0; ob >= -1; --ob)
        for (int oc = 0; oc >= -1; --oc) {
            bool ok = true;
            for (int corner = 0; corner < 8 && ok; ++corner) {
                int q[3] = {g[0], g[1], g[2]};
                q[b] += ob; q[c] += oc;
                q[0] += corner & 1; q[1] += (corner >> 1) & 1; q[2] += (corner >> 2) & 1;
                float f;
                ok = tsdf_voxel(P, q, f) > 0.f;
            }
            if (ok) {
                const double a0 = fabs((double)f0), a1 = fabs((double)f1);
                t = a0 / (a0 + a1);
                return true;
            }
        }
    return false;
}

// per unit: count (EMIT = false) or write (EMIT = true) its surface points in (voxel, axis) order
template <bool EMIT>
NSR_KERNEL void tsdf_surface_kernel(const TsdfParams P) {
    int *sc = reinterpret_cast<int *>(lds_base());                    // [kTsdfThreads + 1]
    const long long c = bid_x();
    const int t = tid();
    const int *U = P.units + 3 * c;
    long long base = EMIT ? P.counts[c] : 0;
    for (int j = 0; j < kTsdfPerThread; ++j) {
        const int v = j * kTsdfThreads + t;
        const int g[3] = {U[0] * kTsdfUnit + (v >> 8), U[1] * kTsdfUnit + ((v >> 4) & 15), U[2] * kTsdfUnit + (v & 15)};
        double tt[3];
        bool e[3];
        int n = 0;
        for (int a = 0; a < 3; ++a) { e[a] = tsdf_edge(P, g, a, tt[a]); n += e[a] ? 1 : 0; }
        sc[t] = n;
        block_sync();
        if (t == 0) {
            int run = 0;
            for (int i = 0; i < kTsdfThreads; ++i) { const int x = sc[i]; sc[i] = run; run += x; }
            sc[kTsdfThreads] = run;
        }
        block_sync();
        if (EMIT) {
            long long o = base + sc[t];
            for (int a = 0; a < 3; ++a) {
                if (!e[a]) continue;
                for (int i = 0; i < 3; ++i) {
                    const double ctr = (double)U[i] * P.ul + ((double)(g[i] - U[i] * kTsdfUnit) + 0.5) * P.vl;
                    P.points[3 * o + i] = i == a ? ctr + tt[a] * P.vl : ctr;
                }
                ++o;
            }
        }
        base += sc[kTsdfThreads];
        block_sync();                                                 // sc is reused by the next j
    }
    if (!EMIT && t == 0) P.counts[c] = base;
}

NSR_KERNEL void tsdf_count_scan_kernel(const TsdfParams P) {
    if (tid() != 0) return;
    long long run = 0;
    for (long long c = 0; c < P.n_units; ++c) { const long long x = P.counts[c]; P.counts[c] = run; run += x; }
    P.counts[P.n_units] = run;
}

// ------------------------------------------------------------------------------------------------
// Hull pre-filter and point-in-hull test
// ------------------------------------------------------------------------------------------------
struct HullParams {
    const void *pts;                 // [n][3] fp64 (extremes / prefilter) or fp32 / fp64 (contains)
    long long n;
    int fp64;
    double *partial;                 // [kHullBlocks][kHullDirs][2] (score, index as double)
    long long *ext;                  // [kHullDirs] out
    double planes[kHullMaxPlanes][4];
    int n_planes;
    double margin;
    const double *dplanes;           // [n_planes][4] device (contains)
    unsigned char *out;              // [n]
};

NSR_DEV void hull_dir(int j, double d[3]) {
    const int code = j < 13 ? j : j + 1;                              // skip (0, 0, 0) = code 13
    d[0] = (double)(code / 9 - 1); d[1] = (double)((code / 3) % 3 - 1); d[2] = (double)(code % 3 - 1);
}

NSR_DEV bool hull_better(double s, long long i, double bs, long long bi) { return s > bs || (s == bs && i < bi); }

NSR_KERNEL void hull_extreme_kernel(const HullParams P) {
    double *rs = reinterpret_cast<double *>(lds_base());              // [256] scores
    long long *ri = reinterpret_cast<long long *>(rs + 256);          // [256] indices
    const int t = tid();
    const double *p = static_cast<const double *>(P.pts);
    for (int j = 0; j < kHullDirs; ++j) {
        double d[3];
        hull_dir(j, d);
        double bs = -__builtin_huge_val();
        long long bi = -1;
        for (long long i = (long long)bid_x() * 256 + t; i < P.n; i += (long long)kHullBlocks * 256) {
            const double s = (d[0] * p[3 * i] + d[1] * p[3 * i + 1]) + d[2] * p[3 * i + 2];
            if (s == s && (bi < 0 || hull_better(s, i, bs, bi))) { bs = s; bi = i; }
        }
        rs[t] = bs; ri[t] = bi;
        block_sync();
        for (int w = 128; w >= 1; w >>= 1) {
            if (t < w && ri[t + w] >= 0 && (ri[t] < 0 || hull_better(rs[t + w], ri[t + w], rs[t], ri[t]))) { rs[t] = rs[t + w]; ri[t] = ri[t + w]; }
            block_sync();
        }
        if (t == 0) { P.partial[2 * (bid_x() * kHullDirs + j)] = rs[0]; P.partial[2 * (bid_x() * kHullDirs + j) + 1] = (double)ri[0]; }
        block_sync();
    }
}

NSR_KERNEL void hull_extreme_final_kernel(const HullParams P) {
    const int j = tid();
    if (j >= kHullDirs) return;
    double bs = -__builtin_huge_val();
    long long bi = -1;
    for (int b = 0; b < kHullBlocks; ++b) {
        const double s = P.partial[2 * (b * kHullDirs + j)];
        const long long i = (long long)P.partial[2 * (b * kHullDirs + j) + 1];
        if (i >= 0 && (bi < 0 || hull_better(s, i, bs, bi))) { bs = s; bi = i; }
    }
    P.ext[j] = bi;
}

NSR_DEV double hull_dist(const double *pl, double x, double y, double z) { return ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3]; }

NSR_KERNEL void hull_prefilter_kernel(const HullParams P) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i >= P.n) return;
    const double *p = static_cast<const double *>(P.pts) + 3 * i;
    bool inside = true;
    for (int j = 0; j < P.n_planes && inside; ++j) inside = hull_dist(P.planes[j], p[0], p[1], p[2]) < -P.margin;
    P.out[i] = inside ? 0 : 1;                                        // 1 = survives
}

// one thread per point; the planes pass through LDS in chunks; a thread stops testing at its first separating plane
NSR_KERNEL void hull_contains_kernel(const HullParams P) {
    double *pl = reinterpret_cast<double *>(lds_base());              // [kContainsChunk][4]
    const long long i = (long long)bid_x() * nthreads() + tid();
    const bool live = i < P.n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) nn_load(P.pts, P.fp64, i, x, y, z);
    bool inside = live;
    for (int j0 = 0; j0 < P.n_planes; j0 += kContainsChunk) {
        const int nj = P.n_planes - j0 < kContainsChunk ? P.n_planes - j0 : kContainsChunk;
        block_sync();
        for (int e = tid(); e < 4 * nj; e += nthreads()) pl[e] = P.dplanes[4ll * j0 + e];
        block_sync();
        for (int j = 0; j < nj && inside; ++j) inside = hull_dist(pl + 4 * j, x, y, z) <= 0.0;
    }
    if (live) P.out[i] = inside ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// Host fp64 quickhull.  Initial simplex from the axis extremes (the farthest pair, then the point farthest from its line,
// then from its plane; ties -> smallest index); a point is outside a face iff its distance exceeds tol; a face's outside set
// is processed at its farthest point (ties -> smallest index), the faces visible from it (distance > tol) are found by a
// search over edge neighbours, and the horizon is coned to the point.  Faces are processed in creation order, so the output
// order is deterministic.  Coplanar facets come out triangulated.  Returns 0, or -1 (fewer than 4 points / all points within
// tol of a plane: no volume), -2 (the surface is not closed: numerical breakdown).
// ------------------------------------------------------------------------------------------------
struct HullFace { int v[3]; double n[3], off; bool alive; std::vector<int> out; };

inline void hull_plane(const double *p, HullFace &f) {
    const double *a = p + 3ll * f.v[0], *b = p + 3ll * f.v[1], *c = p + 3ll * f.v[2];
    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const double len = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    for (int i = 0; i < 3; ++i) f.n[i] = len > 0.0 ? n[i] / len : 0.0;
    f.off = -((f.n[0] * a[0] + f.n[1] * a[1]) + f.n[2] * a[2]);
}

inline double hull_fdist(const double *p, const HullFace &f, long long i) {
    return ((f.n[0] * p[3 * i] + f.n[1] * p[3 * i + 1]) + f.n[2] * p[3 * i + 2]) + f.off;
}

inline unsigned long long hull_ekey(int a, int b) { return ((unsigned long long)(unsigned)a << 32) | (unsigned)b; }

inline int hull_build(const double *p, long long n, double tol, std::vector<HullFace> &F) {
    F.clear();
    if (n < 4) return -1;
    auto d2 = [&](long long i, long long j) {
        const double x = p[3 * i] - p[3 * j], y = p[3 * i + 1] - p[3 * j + 1], z = p[3 * i + 2] - p[3 * j + 2];
        return (x * x + y * y) + z * z;
    };
    long long ex[6] = {0, 0, 0, 0, 0, 0};
    for (long long i = 1; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            if (p[3 * i + d] < p[3 * ex[d] + d]) ex[d] = i;
            if (p[3 * i + d] > p[3 * ex[3 + d] + d]) ex[3 + d] = i;
        }
    long long i0 = ex[0], i1 = ex[3];
    double best = -1.0;
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (d2(ex[a], ex[b]) > best) { best = d2(ex[a], ex[b]); i0 = ex[a]; i1 = ex[b]; }
    if (!(std::sqrt(best) > tol)) return -1;
    long long i2 = -1;
    best = -1.0;
    for (long long i = 0; i < n; ++i) {
        const double u[3] = {p[3 * i1] - p[3 * i0], p[3 * i1 + 1] - p[3 * i0 + 1], p[3 * i1 + 2] - p[3 * i0 + 2]};
        const double w[3] = {p[3 * i] - p[3 * i0], p[3 * i + 1] - p[3 * i0 + 1], p[3 * i + 2] - p[3 * i0 + 2]};
        const double c[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        const double v = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) / ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        if (v > best) { best = v; i2 = i; }
    }
    if (!(std::sqrt(best) > tol)) return -1;
    HullFace base;
    base.v[0] = (int)i0; base.v[1] = (int)i1; base.v[2] = (int)i2;
    hull_plane(p, base);
    long long i3 = -1;
    best = -1.0;
    for (long long i = 0; i < n; ++i) {
        const double v = std::fabs(hull_fdist(p, base, i));
        if (v > best) { best = v; i3 = i; }
    }
    if (!(best > tol)) return -1;
    const int s[4] = {(int)i0, (int)i1, (int)i2, (int)i3};
    const int tri[4][4] = {{0, 1, 2, 3}, {0, 3, 1, 2}, {0, 2, 3, 1}, {1, 3, 2, 0}};   // three corners + the opposite one
    std::unordered_map<unsigned long long, int> edge;
    for (int f = 0; f < 4; ++f) {
        HullFace h;
        h.v[0] = s[tri[f][0]]; h.v[1] = s[tri[f][1]]; h.v[2] = s[tri[f][2]];
        hull_plane(p, h);
        if (hull_fdist(p, h, s[tri[f][3]]) > 0.0) { std::swap(h.v[1], h.v[2]); hull_plane(p, h); }
        h.alive = true;
        F.push_back(h);
    }
    for (int f = 0; f < 4; ++f)
        for (int e = 0; e < 3; ++e) edge[hull_ekey(F[f].v[e], F[f].v[(e + 1) % 3])] = f;
    for (long long i = 0; i < n; ++i) {
        if (i == i0 || i == i1 || i == i2 || i == i3) continue;
        for (int f = 0; f < 4; ++f)
            if (hull_fdist(p, F[f], i) > tol) { F[f].out.push_back((int)i); break; }
    }
    std::vector<int> vis, nvis, visible, fresh;                          // vis / nvis: the iteration that found a face (not) visible
    int iter = 0;
    std::vector<std::pair<int, int>> horizon;
    for (size_t fi = 0; fi < F.size(); ++fi) {
        if (!F[fi].alive || F[fi].out.empty()) continue;
        int apex = -1;
        double far = -1.0;
        for (int i : F[fi].out) {
            const double v = hull_fdist(p, F[fi], i);
            if (v > far || (v == far && i < apex)) { far = v; apex = i; }
        }
        ++iter;
        vis.resize(F.size(), 0);
        nvis.resize(F.size(), 0);
        visible.assign(1, (int)fi);
        horizon.clear();
        vis[fi] = iter;
        for (size_t q = 0; q < visible.size(); ++q) {
            const HullFace &f = F[visible[q]];
            for (int e = 0; e < 3; ++e) {
                const int a = f.v[e], b = f.v[(e + 1) % 3];
                auto it = edge.find(hull_ekey(b, a));
                if (it == edge.end()) return -2;
                const int nb = it->second;
                if (vis[nb] != iter && nvis[nb] != iter) {
                    if (hull_fdist(p, F[nb], apex) > tol) { vis[nb] = iter; visible.push_back(nb); }
                    else nvis[nb] = iter;
                }
                if (nvis[nb] == iter) horizon.emplace_back(a, b);
            }
        }
        for (int vf : visible)
            for (int e = 0; e < 3; ++e) edge.erase(hull_ekey(F[vf].v[e], F[vf].v[(e + 1) % 3]));
        fresh.clear();
        for (auto &hz : horizon) {
            HullFace h;
            h.v[0] = hz.first; h.v[1] = hz.second; h.v[2] = apex;
            h.alive = true;
            hull_plane(p, h);
            fresh.push_back((int)F.size());
            F.push_back(h);
            for (int e = 0; e < 3; ++e) edge[hull_ekey(h.v[e], h.v[(e + 1) % 3])] = (int)F.size() - 1;
        }
        for (int vf : visible) {
            for (int i : F[vf].out) {
                if (i == apex) continue;
                for (int nf : fresh)
                    if (hull_fdist(p, F[nf], i) > tol) { F[nf].out.push_back(i); break; }
            }
            F[vf].alive = false;
            std::vector<int>().swap(F[vf].out);
        }
    }
    // closed surface: every directed edge of a live face has its reverse
    for (const HullFace &f : F) {
        if (!f.alive) continue;
        for (int e = 0; e < 3; ++e) {
            auto it = edge.find(hull_ekey(f.v[(e + 1) % 3], f.v[e]));
            if (it == edge.end() || !F[it->second].alive) return -2;
        }
    }
    return 0;
}

}  // namespace nsr
