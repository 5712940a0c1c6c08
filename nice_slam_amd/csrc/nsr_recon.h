// nsr_recon.h -- reconstruction evaluation (include/nsr.h, "Reconstruction evaluation"): exact nearest neighbour over a
// uniform cell grid, area-weighted surface sampling, fixed-order fp64 reductions for the metrics and ICP, and frustum
// culling of mesh vertices over a trajectory (src/tools/eval_recon.py, src/tools/cull_mesh.py).
// Included by nsr_api.cpp AFTER nsr_kernels.h, whose device primitives (nsr_dev.h, or the CPU emulator's shadow of it) and
// philox_word it uses; it includes nothing itself, so that both builds resolve those names to their own versions.
// No global fp64 atomics anywhere: every sum is taken in a fixed order (block trees, then blocks in index order), so every
// result is bit-identical from run to run.
#pragma once

namespace nsr {

// ------------------------------------------------------------------------------------------------
// Exact nearest neighbour.  The reference set is binned into a uniform grid of fine cells (about 2 cells per reference point;
// the plan is made on the host from the bounding box, nsr_nn_plan); fine cells are grouped into coarse cells of 8^3 and the
// key of a point is (coarse cell id) * 512 + (fine cell inside its coarse cell), so that sorting by key makes every fine cell
// AND every coarse cell a contiguous run.  A query walks shells of fine cells at Chebyshev radius 0..kNnFineShells-1 around its
// (clamped) cell and stops as soon as the exact lower bound on the distance to any cell outside the walked box exceeds its best
// distance (nn_walk); a query that is still open after that (far from the set, or in an empty region) scans the occupied coarse
// cells by their bounding boxes instead: bounded by the number of coarse cells, never by an unbounded shell walk.
// Distances: fp64, dx*dx + dy*dy + dz*dz in that order (no contraction), correctly rounded sqrt; ties -> smallest index.
// The grid (NnGrid), its keys, the clear and the run marking of its tables, and the walk (nn_walk<Sink>) are also the
// mesh-distance index's (nsr_meshdist.h), which supplies a sink of its own and its own coarse route.
// ------------------------------------------------------------------------------------------------
constexpr int kNnLocal = 8;                     // fine cells per coarse cell along each axis (key = coarse * 512 + local)
constexpr int kNnFineShells = 3;
constexpr int kNnBoundBlocks = 256;
// plan layout (doubles), written by nsr_nn_plan
enum { kNnLo = 0, kNnHi = 3, kNnH = 6, kNnDim = 7, kNnCDim = 10, kNnCells = 13, kNnCoarse = 14, kNnSlack = 15, kNnPlanSize = 16 };

// The grid of an index, whatever it holds (reference points here, (cell, face) pairs in nsr_meshdist.h): the plan's geometry
// and the runs of every fine and coarse cell in the index's key-ordered table.
struct NnGrid {
    int nd[3], nc[3];                // fine and coarse grid dimensions
    double lo[3], hi[3], h, slack;   // bounding box of the indexed set, cell edge, absolute slack of the pruning bounds
    long long ncell, ncoarse;
    int *fstart, *fend;              // [ncell] fine-cell runs in key order
    int *cstart, *cend;              // [ncoarse] coarse-cell runs
};

struct NnParams {
    NnGrid G;
    const void *pts;                 // [n][3] fp32 or fp64 (ref for bounds / keys / build, query for keys / query)
    long long n;
    int fp64;
    long long m;                     // reference points
    double *bounds;                  // [1 + kNnBoundBlocks][6] (nn_bounds)
    long long *keys;                 // [n] (nn_keys out; nn_build in: sorted)
    const long long *order;          // [m] reference permutation that sorts the keys (nn_build); query order (nn_query)
    double *sref;                    // [m][3] reference points in key order, fp64
    long long *sidx;                 // [m] their original index
    double *cbox;                    // [ncoarse][6] bounding box of a coarse cell's points
    double *dist;                    // [n] out
    long long *idx;                  // [n] out
    int *ncand;                      // [n] out (optional): points examined
};

NSR_DEV void nn_load(const void *p, int fp64, long long i, double &x, double &y, double &z) {
    if (fp64) {
        const double *d = static_cast<const double *>(p) + 3 * i;
        x = d[0]; y = d[1]; z = d[2];
    } else {
        const float *f = static_cast<const float *>(p) + 3 * i;
        x = (double)f[0]; y = (double)f[1]; z = (double)f[2];
    }
}

NSR_DEV double nn_min(double a, double v) { return (v < a || v != v) ? v : a; }   // a NaN sticks (the plan rejects it)
NSR_DEV double nn_max(double a, double v) { return (v > a || v != v) ? v : a; }

// bounding box: kNnBoundBlocks blocks stride over the points, one partial box per block, then one block combines them in order
NSR_KERNEL void nn_bounds_kernel(const NnParams P) {
    double *red = reinterpret_cast<double *>(lds_base());          // [6][nthreads]
    const int t = tid(), nt = nthreads();
    double b[6] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val(),
                   -__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    for (long long i = (long long)bid_x() * nt + t; i < P.n; i += (long long)nblk_x() * nt) {
        double p[3];
        nn_load(P.pts, P.fp64, i, p[0], p[1], p[2]);
        for (int d = 0; d < 3; ++d) { b[d] = nn_min(b[d], p[d]); b[3 + d] = nn_max(b[3 + d], p[d]); }
    }
    for (int k = 0; k < 6; ++k) red[k * nt + t] = b[k];
    block_sync();
    if (t < 6) {
        double v = red[t * nt];
        for (int j = 1; j < nt; ++j) v = t < 3 ? nn_min(v, red[t * nt + j]) : nn_max(v, red[t * nt + j]);
        P.bounds[6 * (1 + bid_x()) + t] = v;
    }
}

NSR_KERNEL void nn_bounds_final_kernel(const NnParams P) {
    const int t = tid();
    if (t >= 6) return;
    double v = P.bounds[6 + t];
    for (int b = 1; b < kNnBoundBlocks; ++b) v = t < 3 ? nn_min(v, P.bounds[6 * (1 + b) + t]) : nn_max(v, P.bounds[6 * (1 + b) + t]);
    P.bounds[t] = v;
}

NSR_DEV int nn_cell(const NnGrid &G, int d, double x) {
    double f = floor((x - G.lo[d]) / G.h);
    if (!(f >= 0.0)) f = 0.0;                                      // below the box, or NaN
    if (f > (double)(G.nd[d] - 1)) f = (double)(G.nd[d] - 1);
    return (int)f;
}

NSR_DEV long long nn_key(const NnGrid &G, int cx, int cy, int cz) {
    const long long coarse = ((long long)(cx / kNnLocal) * G.nc[1] + cy / kNnLocal) * G.nc[2] + cz / kNnLocal;
    return coarse * 512 + (cx % kNnLocal) * 64 + (cy % kNnLocal) * 8 + cz % kNnLocal;
}

NSR_DEV long long nn_fine_id(const NnGrid &G, int cx, int cy, int cz) { return ((long long)cx * G.nd[1] + cy) * G.nd[2] + cz; }

NSR_KERNEL void nn_keys_kernel(const NnParams P) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i >= P.n) return;
    double x, y, z;
    nn_load(P.pts, P.fp64, i, x, y, z);
    P.keys[i] = nn_key(P.G, nn_cell(P.G, 0, x), nn_cell(P.G, 1, y), nn_cell(P.G, 2, z));
}

NSR_KERNEL void nn_clear_kernel(const NnGrid G) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i < G.ncell) { G.fstart[i] = 0; G.fend[i] = 0; }
    if (i < G.ncoarse) { G.cstart[i] = 0; G.cend[i] = 0; }
}

// decode a key into its fine-cell id; -1 for a key outside the plan (the table is never written out of range)
NSR_DEV long long nn_key_fine(const NnGrid &G, long long key) {
    if (key < 0) return -1;
    const long long c = key >> 9;
    const int l = (int)(key & 511);
    if (c >= G.ncoarse) return -1;
    const int cz = (int)(c % G.nc[2]), cy = (int)((c / G.nc[2]) % G.nc[1]), cx = (int)(c / ((long long)G.nc[2] * G.nc[1]));
    const int fx = cx * kNnLocal + (l >> 6), fy = cy * kNnLocal + ((l >> 3) & 7), fz = cz * kNnLocal + (l & 7);
    if (fx >= G.nd[0] || fy >= G.nd[1] || fz >= G.nd[2]) return -1;
    return nn_fine_id(G, fx, fy, fz);
}

// position j of n sorted keys: the fine-cell and coarse-cell runs that start or end there are marked in the run tables.
// Returns the coarse cell whose run starts at j, -1 if none does (or the key is outside the plan: nothing is marked).
NSR_DEV long long nn_mark_runs(const NnGrid &G, const long long *keys, long long j, long long n) {
    const long long k = keys[j], f = nn_key_fine(G, k);
    if (f < 0) return -1;
    if (j == 0 || keys[j - 1] != k) G.fstart[f] = (int)j;
    if (j == n - 1 || keys[j + 1] != k) G.fend[f] = (int)(j + 1);
    const long long c = k >> 9;
    const bool starts = j == 0 || (keys[j - 1] >> 9) != c;
    if (starts) G.cstart[c] = (int)j;
    if (j == n - 1 || (keys[j + 1] >> 9) != c) G.cend[c] = (int)(j + 1);
    return starts ? c : -1;
}

// reference points in key order (fp64) + the runs of every fine and coarse cell
NSR_KERNEL void nn_gather_kernel(const NnParams P) {
    const long long j = (long long)bid_x() * nthreads() + tid();
    if (j >= P.m) return;
    const long long o = P.order[j];
    if (o < 0 || o >= P.m) return;
    double x, y, z;
    nn_load(P.pts, P.fp64, o, x, y, z);
    P.sref[3 * j] = x; P.sref[3 * j + 1] = y; P.sref[3 * j + 2] = z;
    P.sidx[j] = o;
    nn_mark_runs(P.G, P.keys, j, P.m);
}

NSR_KERNEL void nn_box_kernel(const NnParams P) {
    const long long c = (long long)bid_x() * nthreads() + tid();
    if (c >= P.G.ncoarse) return;
    double b[6] = {__builtin_huge_val(), __builtin_huge_val(), __builtin_huge_val(),
                   -__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()};
    for (int j = P.G.cstart[c]; j < P.G.cend[c]; ++j)
        for (int d = 0; d < 3; ++d) { b[d] = nn_min(b[d], P.sref[3ll * j + d]); b[3 + d] = nn_max(b[3 + d], P.sref[3ll * j + d]); }
    for (int k = 0; k < 6; ++k) P.cbox[6 * c + k] = b[k];
}

// The walk both searches share.  One query q walks the shells of fine cells at Chebyshev radius 0..kNnFineShells-1 around its
// (clamped) cell and hands every cell's run [fstart, fend) of the key-ordered table to the sink; after each shell it stops if
// the walked box covers the grid, or if the exact lower bound on the distance to anything outside the walked box, less the
// slack, exceeds the sink's best distance.  Returns whether the query is closed; an open one takes the caller's coarse route,
// which prunes with the same slack (handed back).  What a run holds is the sink's business:
//   scan(q, s, e)      examine the entries [s, e) of the table;
//   best2()            the smallest squared distance found so far (huge before any).
// Both are resolved at compile time: NnPointSink below, MdFaceSink in nsr_meshdist.h.
template <class Sink>
NSR_DEV bool nn_walk(const NnGrid &G, const double q[3], Sink &sink, double &slack) {
    int c[3];
    double o[3], o2 = 0.0, qabs = 0.0;
    for (int d = 0; d < 3; ++d) {
        c[d] = nn_cell(G, d, q[d]);
        const double below = G.lo[d] - q[d], above = q[d] - G.hi[d];
        o[d] = below > 0.0 ? below : (above > 0.0 ? above : 0.0);    // distance to the grid's box along d
        o2 += o[d] * o[d];
        qabs += fabs(q[d]);
    }
    slack = G.slack + 1e-12 * qabs;
    for (int r = 0; r < kNnFineShells; ++r) {
        const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < G.nd[0] - 1 ? c[0] + r : G.nd[0] - 1;
        const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < G.nd[1] - 1 ? c[1] + r : G.nd[1] - 1;
        const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < G.nd[2] - 1 ? c[2] + r : G.nd[2] - 1;
        for (int x = x0; x <= x1; ++x)
            for (int y = y0; y <= y1; ++y)
                for (int z = z0; z <= z1; ++z) {
                    const int ax = abs(x - c[0]), ay = abs(y - c[1]), az = abs(z - c[2]);
                    const int cheb = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
                    if (cheb != r) continue;
                    const long long f = nn_fine_id(G, x, y, z);
                    sink.scan(q, G.fstart[f], G.fend[f]);
                }
        // everything outside the walked box (a point; the part of a face in a cell out there) lies beyond one of its sides (along
        // d: a gap g_d) and, along the other axes, at least as far as the grid's box is: |p - q|^2 >= g_d^2 + sum_{e != d} o_e^2
        double L2 = __builtin_huge_val();
        for (int d = 0; d < 3; ++d) {
            const double rest = o2 - o[d] * o[d] > 0.0 ? o2 - o[d] * o[d] : 0.0;
            const int b0 = c[d] - r, b1 = c[d] + r + 1;                // the walked box along d, in cells: [b0, b1)
            if (b0 > 0) {
                double g = q[d] - (G.lo[d] + (double)b0 * G.h);
                g = g > 0.0 ? g : 0.0;
                L2 = g * g + rest < L2 ? g * g + rest : L2;
            }
            if (b1 < G.nd[d]) {
                double g = (G.lo[d] + (double)b1 * G.h) - q[d];
                g = g > 0.0 ? g : 0.0;
                L2 = g * g + rest < L2 ? g * g + rest : L2;
            }
        }
        if (L2 == __builtin_huge_val()) return true;                 // the walked box covers the whole grid
        const double L = sqrt(L2) - slack;
        if (L > 0.0 && L * L > sink.best2() * (1.0 + 1e-12)) return true;
    }
    return false;
}

struct NnBest { double d2; long long i; int cand; };

NSR_DEV void nn_scan(const NnParams &P, const double q[3], int s, int e, NnBest &B) {
    for (int j = s; j < e; ++j) {
        const double dx = q[0] - P.sref[3ll * j], dy = q[1] - P.sref[3ll * j + 1], dz = q[2] - P.sref[3ll * j + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const long long oi = P.sidx[j];
        ++B.cand;
        if (d2 < B.d2 || (d2 == B.d2 && oi < B.i)) { B.d2 = d2; B.i = oi; }
    }
}

struct NnPointSink {                                            // the table is sref / sidx: the reference points in key order
    const NnParams &P;
    NnBest &B;
    NSR_DEV void scan(const double q[3], int s, int e) const { nn_scan(P, q, s, e, B); }
    NSR_DEV double best2() const { return B.d2; }
};

// one thread per query, in key order (P.order), so that a wave's lanes walk neighbouring cells
NSR_KERNEL void nn_query_kernel(const NnParams P) {
    const long long t = (long long)bid_x() * nthreads() + tid();
    if (t >= P.n) return;
    const long long qi = P.order ? P.order[t] : t;
    if (qi < 0 || qi >= P.n) return;
    double q[3], slack;
    nn_load(P.pts, P.fp64, qi, q[0], q[1], q[2]);
    NnBest B{__builtin_huge_val(), -1, 0};
    NnPointSink sink{P, B};
    if (!nn_walk(P.G, q, sink, slack)) {
        // coarse fallback: an upper bound on the answer from the farthest corner of every occupied coarse box, then a scan of
        // every coarse cell whose box can hold a point at or below the current bound
        double U2 = B.d2;
        for (long long k = 0; k < P.G.ncoarse; ++k) {
            if (P.G.cstart[k] >= P.G.cend[k]) continue;
            const double *bx = P.cbox + 6 * k;
            double far2 = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double a = q[d] - bx[d], b = bx[3 + d] - q[d];
                far2 += a * a > b * b ? a * a : b * b;
            }
            U2 = far2 < U2 ? far2 : U2;
        }
        for (long long k = 0; k < P.G.ncoarse; ++k) {
            if (P.G.cstart[k] >= P.G.cend[k]) continue;
            const double *bx = P.cbox + 6 * k;
            double near2 = 0.0;
            for (int d = 0; d < 3; ++d) {
                const double a = bx[d] - q[d], b = q[d] - bx[3 + d];
                const double g = a > 0.0 ? a : (b > 0.0 ? b : 0.0);
                near2 += g * g;
            }
            const double lim2 = B.d2 < U2 ? B.d2 : U2;
            const double nr = sqrt(near2) - slack;
            if (nr <= 0.0 || nr * nr <= lim2 * (1.0 + 1e-12)) nn_scan(P, q, P.G.cstart[k], P.G.cend[k], B);
        }
    }
    P.dist[qi] = sqrt(B.d2);
    P.idx[qi] = B.i;
    if (P.ncand) P.ncand[qi] = B.cand;
}

// ------------------------------------------------------------------------------------------------
// Area-weighted surface sampling (trimesh.sample.sample_surface, which eval_recon.py:103,106 calls): face areas in fp64 as
// trimesh's area_faces, an inclusive scan in a fixed order (a sequential scan inside tiles of kSurfTile faces, a
// sequential exclusive scan of the tile totals, cum = tile prefix + in-tile scan), the face picked by the first cum >= u0 *
// total (np.searchsorted, side 'left'), the point v0 + a (v1 - v0) + b (v2 - v0) with (a, b) -> |(a, b) - 1| when a + b > 1.
// Uniforms: caller-supplied [n][3] (u0, a, b), or philox(counter = (point, 2 draw + half), key = seed) with 53 bits each.
// ------------------------------------------------------------------------------------------------
constexpr int kSurfTile = 256;

struct SurfSampleParams {
    const double *verts;             // [V][3]
    const int *faces;                // [F][3]
    long long nv, nf, ntiles, n;
    double *cum;                     // [F] inclusive scan of the areas
    double *tile;                    // [ntiles + 1]: tile totals, then their exclusive scan
    const double *uniforms;          // [n][3] or null: philox
    unsigned long long seed;
    double *points;                  // [n][3] out
    long long *face_index;           // [n] out
};

NSR_DEV double surf_area(const SurfSampleParams &P, long long f) {
    const int i0 = P.faces[3 * f], i1 = P.faces[3 * f + 1], i2 = P.faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= P.nv || i1 >= P.nv || i2 >= P.nv) return 0.0;
    const double *a = P.verts + 3ll * i0, *b = P.verts + 3ll * i1, *c = P.verts + 3ll * i2;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return sqrt((cx * cx + cy * cy) + cz * cz) / 2.0;
}

NSR_KERNEL void surf_tile_kernel(const SurfSampleParams P) {
    const long long t = (long long)bid_x() * nthreads() + tid();
    if (t >= P.ntiles) return;
    const long long f1 = (t + 1) * kSurfTile < P.nf ? (t + 1) * kSurfTile : P.nf;
    double acc = 0.0;
    for (long long f = t * kSurfTile; f < f1; ++f) { acc += surf_area(P, f); P.cum[f] = acc; }
    P.tile[t] = acc;
}

NSR_KERNEL void surf_tile_scan_kernel(const SurfSampleParams P) {
    if (tid() != 0) return;
    double run = 0.0;
    for (long long t = 0; t < P.ntiles; ++t) { const double v = P.tile[t]; P.tile[t] = run; run += v; }
}

NSR_KERNEL void surf_cum_kernel(const SurfSampleParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f < P.nf) P.cum[f] = P.tile[f / kSurfTile] + P.cum[f];
}

NSR_DEV double surf_uniform(unsigned long long seed, long long i, unsigned draw) {
    const unsigned hi = philox_word((unsigned)i, (unsigned)((unsigned long long)i >> 32), 2 * draw, 0u, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned lo = philox_word((unsigned)i, (unsigned)((unsigned long long)i >> 32), 2 * draw + 1, 0u, (unsigned)seed, (unsigned)(seed >> 32));
    return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) * (1.0 / 9007199254740992.0);
}

NSR_KERNEL void surf_point_kernel(const SurfSampleParams P) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i >= P.n) return;
    double u0, a, b;
    if (P.uniforms) {
        u0 = P.uniforms[3 * i]; a = P.uniforms[3 * i + 1]; b = P.uniforms[3 * i + 2];
    } else {
        u0 = surf_uniform(P.seed, i, 0); a = surf_uniform(P.seed, i, 1); b = surf_uniform(P.seed, i, 2);
    }
    const double pick = u0 * P.cum[P.nf - 1];
    long long lo = 0, hi = P.nf - 1;                                // first f with cum[f] >= pick (the last face if none)
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (P.cum[mid] >= pick) hi = mid; else lo = mid + 1;
    }
    if (a + b > 1.0) { a = fabs(a - 1.0); b = fabs(b - 1.0); }
    const int i0 = P.faces[3 * lo], i1 = P.faces[3 * lo + 1], i2 = P.faces[3 * lo + 2];
    const bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < P.nv && i1 < P.nv && i2 < P.nv;
    for (int d = 0; d < 3; ++d) {
        const double v0 = ok ? P.verts[3ll * i0 + d] : 0.0, v1 = ok ? P.verts[3ll * i1 + d] : 0.0, v2 = ok ? P.verts[3ll * i2 + d] : 0.0;
        P.points[3 * i + d] = ((v1 - v0) * a + (v2 - v0) * b) + v0;
    }
    P.face_index[i] = lo;
}

// ------------------------------------------------------------------------------------------------
// Fixed-order fp64 reductions: one value vector per element, a tree over the 256 threads of a block (fixed pairing), one
// partial per block, then the partials summed in block order by one thread per component.
//   DIST: (dist, dist < th)                                          -> mean distance, completion ratio (eval_recon.py:24-43)
//   ICP1: inliers dist < th: (1, |s - t|^2, s, t)                    -> count, squared error, centroids
//   ICP2: inliers: (t - mu_t)(s - mu_s)^T, mu from ICP1's output     -> the cross-covariance of Umeyama's estimate
//   NORMAL: (|s . t|, 1) unless s or t is the zero vector, t = tgt[idx] -> nsr_normal_stats (nsr_meshdist.h, "Normals");
//           finished as DIST is
// ------------------------------------------------------------------------------------------------
constexpr int kRedThreads = 256;
enum { kRedDist = 0, kRedIcp1 = 1, kRedIcp2 = 2, kRedNormal = 3 };
constexpr int red_width(int mode) { return mode == kRedDist || mode == kRedNormal ? 2 : (mode == kRedIcp1 ? 8 : 9); }

struct RedParams {
    const double *dist;              // [n] (not NORMAL)
    const double *src;               // [n][3] (ICP, NORMAL)
    const double *tgt;               // [m][3] (ICP, NORMAL)
    const long long *idx;            // [n] into tgt (ICP, NORMAL)
    long long n, m, nblocks;
    double th;
    double *partial;                 // [nblocks][9]
    double *out;                     // DIST, NORMAL: [2]; ICP: [17] count, sse, mu_s[3], mu_t[3], cov[9]
};

template <int MODE>
NSR_KERNEL void reduce_kernel(const RedParams P) {
    constexpr int V = red_width(MODE);
    double *red = reinterpret_cast<double *>(lds_base());          // [V][kRedThreads]
    const int t = tid();
    const long long i = (long long)bid_x() * kRedThreads + t;
    double v[V];
    for (int k = 0; k < V; ++k) v[k] = 0.0;
    if (MODE == kRedNormal) {
        if (i < P.n && P.idx[i] >= 0 && P.idx[i] < P.m) {
            const double *a = P.src + 3 * i, *b = P.tgt + 3 * P.idx[i];
            const bool za = a[0] == 0.0 && a[1] == 0.0 && a[2] == 0.0, zb = b[0] == 0.0 && b[1] == 0.0 && b[2] == 0.0;
            if (!za && !zb) { v[0] = fabs((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]); v[1] = 1.0; }
        }
    } else if (i < P.n) {
        const double dd = P.dist[i];
        if (MODE == kRedDist) {
            v[0] = dd;
            v[1] = dd < P.th ? 1.0 : 0.0;
        } else if (dd < P.th && P.idx[i] >= 0 && P.idx[i] < P.m) {
            const double *s = P.src + 3 * i, *g = P.tgt + 3 * P.idx[i];
            if (MODE == kRedIcp1) {
                const double dx = s[0] - g[0], dy = s[1] - g[1], dz = s[2] - g[2];
                v[0] = 1.0;
                v[1] = (dx * dx + dy * dy) + dz * dz;
                for (int d = 0; d < 3; ++d) { v[2 + d] = s[d]; v[5 + d] = g[d]; }
            } else {
                for (int r = 0; r < 3; ++r)
                    for (int c = 0; c < 3; ++c) v[3 * r + c] = (g[r] - P.out[5 + r]) * (s[c] - P.out[2 + c]);
            }
        }
    }
    for (int k = 0; k < V; ++k) red[k * kRedThreads + t] = v[k];
    block_sync();
    for (int w = kRedThreads / 2; w >= 1; w >>= 1) {
        if (t < w)
            for (int k = 0; k < V; ++k) red[k * kRedThreads + t] = red[k * kRedThreads + t] + red[k * kRedThreads + t + w];
        block_sync();
    }
    if (t < V) P.partial[9 * bid_x() + t] = red[t * kRedThreads];
}

template <int MODE>
NSR_KERNEL void reduce_final_kernel(const RedParams P) {
    constexpr int V = red_width(MODE);
    const int t = tid();
    if (t >= V) return;
    double acc = 0.0;
    for (long long b = 0; b < P.nblocks; ++b) acc += P.partial[9 * b + t];
    if (MODE == kRedDist) { P.out[t] = acc; return; }
    if (MODE == kRedIcp2) { P.out[8 + t] = acc; return; }
    // ICP1: count, sse, then the centroids (sum / count; 0 without inliers)
    if (t < 2) P.out[t] = acc;
    else {
        double cnt = 0.0;
        for (long long b = 0; b < P.nblocks; ++b) cnt += P.partial[9 * b];
        P.out[t] = cnt > 0.0 ? acc / cnt : 0.0;
    }
}

// p <- R p + t in fp64 (rows of the 3x4 [R | t]; each component ((r0 x + r1 y) + r2 z) + t)
struct XformParams {
    double *pts;
    long long n;
    double m[12];
};

NSR_KERNEL void transform_points_kernel(const XformParams P) {
    const long long i = (long long)bid_x() * nthreads() + tid();
    if (i >= P.n) return;
    const double x = P.pts[3 * i], y = P.pts[3 * i + 1], z = P.pts[3 * i + 2];
    for (int r = 0; r < 3; ++r) P.pts[3 * i + r] = ((P.m[4 * r] * x + P.m[4 * r + 1] * y) + P.m[4 * r + 2] * z) + P.m[4 * r + 3];
}

// ------------------------------------------------------------------------------------------------
// Frustum culling of mesh vertices over a whole trajectory in one launch (cull_mesh.py:45-75).  The poses travel through LDS
// in chunks of kCullChunk; the reference's fp32 arithmetic in its order: p -> fp32, cam = w2c[:3] @ [p, 1] (sequential
// sums), x *= -1, uvz = K @ cam, z = uvz[2] + 1e-5, (u, v) = uvz[:2] / z; seen by a pose iff 0 <= -z, 0 < u < W, 0 < v < H.
// A vertex is kept if any pose sees it; a face is kept unless none of its three vertices is seen.
// ------------------------------------------------------------------------------------------------
constexpr int kCullChunk = 1024;
constexpr int kCullThreads = 256;

struct CullParams {
    const void *verts;               // [n][3] fp32 or fp64
    long long n, nf;
    int fp64, K;
    const float *w2c;                // [K][12] rows 0..2 of inv(c2w), fp32
    float kf[9];                     // K.float()
    float W, H;
    const int *faces;                // [nf][3]
    unsigned char *seen;             // [n]
    unsigned char *keep;             // [nf]
};

NSR_DEV bool cull_sees(const CullParams &P, const float *w, float px, float py, float pz) {
    float cam[3];
    for (int r = 0; r < 3; ++r) cam[r] = ((w[r * 4 + 0] * px + w[r * 4 + 1] * py) + w[r * 4 + 2] * pz) + w[r * 4 + 3] * 1.f;
    const float X = cam[0] * -1.f, Y = cam[1], Z = cam[2];
    const float uh = (P.kf[0] * X + P.kf[1] * Y) + P.kf[2] * Z;
    const float vh = (P.kf[3] * X + P.kf[4] * Y) + P.kf[5] * Z;
    const float z = ((P.kf[6] * X + P.kf[7] * Y) + P.kf[8] * Z) + 1e-5f;
    const float u = uh / z, v = vh / z;
    return (0.f <= -z) && (u < P.W) && (u > 0.f) && (v < P.H) && (v > 0.f);
}

NSR_KERNEL void cull_vertex_kernel(const CullParams P) {
    float *pose = reinterpret_cast<float *>(lds_base());           // [kCullChunk][12]
    const long long i = (long long)bid_x() * kCullThreads + tid();
    const bool live = i < P.n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) {
        double x, y, z;
        nn_load(P.verts, P.fp64, i, x, y, z);
        px = (float)x; py = (float)y; pz = (float)z;
    }
    bool seen = false;
    for (int k0 = 0; k0 < P.K; k0 += kCullChunk) {
        const int nk = P.K - k0 < kCullChunk ? P.K - k0 : kCullChunk;
        block_sync();                                               // the previous chunk is no longer read
        for (int e = tid(); e < 12 * nk; e += kCullThreads) pose[e] = P.w2c[12ll * k0 + e];
        block_sync();
        if (live)
            for (int k = 0; k < nk && !seen; ++k) seen = cull_sees(P, pose + 12 * k, px, py, pz);
    }
    if (live) P.seen[i] = seen ? 1 : 0;
}

NSR_KERNEL void cull_face_kernel(const CullParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f >= P.nf) return;
    bool keep = false;
    for (int c = 0; c < 3; ++c) {
        const int v = P.faces[3 * f + c];
        keep = keep || (v >= 0 && v < P.n && P.seen[v]);
    }
    P.keep[f] = keep ? 1 : 0;
}

}  // namespace nsr
