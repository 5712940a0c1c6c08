// nsr_meshdist.h -- exact point-to-triangle-mesh distance (include/nsr.h, "Point-to-mesh distance"): the closest point of a
// triangle list to every query, the faces' unit normals and the fixed-order sum of |n . m| over matched normals.
// Included by nsr_api.cpp AFTER nsr_recon.h, whose grid (NnGrid, nn_cell, nn_key, nn_load, nn_clear_kernel, nn_mark_runs), shell
// walk (nn_walk<Sink>: the query's prologue, the shells, the bound and the stop test live there, once) and reductions
// (reduce_kernel<kRedNormal>, reduce_final_kernel) it uses; it includes nothing itself, so that the library and the CPU emulator
// resolve the device primitives to their own versions.  fp64 throughout, no contraction, no atomics: every table and every result is
// bit-identical from run to run.
//
// Per-face distance (md_face).  a, b, c the corners, p the query, dot(u, v) = (ux*vx + uy*vy) + uz*vz, every difference and
// product a single fp64 operation in the order written:
//   ab = b - a, ac = c - a, n = (aby*acz - abz*acy, abz*acx - abx*acz, abx*acy - aby*acx)
//   ap = p - a, bp = p - b, cp = p - c
//   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
//   vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4
// and the first region of this walk that holds gives the closest point x:
//   0  n == (0, 0, 0)                                   degenerate
//   1  d1 <= 0 and d2 <= 0                              x = a
//   2  d3 >= 0 and d4 <= d3                             x = b
//   3  vc <= 0 and d1 >= 0 and d3 <= 0                  den = d1 - d3,            x = a + ab * (d1 / den)
//   4  d6 >= 0 and d5 <= d6                             x = c
//   5  vb <= 0 and d2 >= 0 and d6 <= 0                  den = d2 - d6,            x = a + ac * (d2 / den)
//   6  va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0        den = (d4 - d3) + (d5 - d6),  x = b + (c - b) * ((d4 - d3) / den)
//   7  otherwise (interior)                             den = (va + vb) + vc,     x = (a + ab * (vb / den)) + ac * (vc / den)
// A region whose den is not > 0 or < 0 (zero, or not a number) is degenerate too, and so is region 7 unless va, vb and vc are
// all > 0: exact arithmetic reaches the interior only with all three positive, so anything else is cancellation in a face
// that is degenerate to rounding (three corners collinear after a rotation), where vb / den and vc / den would be noise and
// the point they give could lie far off the face.  Every other region's point lies on the face whatever the rounding (its
// parameter is in [0, 1] by the signs its condition tests).  Degenerate: the nearest of the three
// segments ab, bc, ca in that order (a later one only if strictly nearer); a segment s -> e with d = e - s, l = dot(d, d):
// t = dot(p - s, d) / l; x = s if l == 0 or t <= 0, e if t >= 1, else s + d * t.
// The squared distance is (dx*dx + dy*dy) + dz*dz with d = p - x; the square root is taken once per query.
//
// Index.  The grid plan is nsr_nn_plan's made for nf "points" over the box of the vertices (about two cells per face, a
// degenerate extent collapsed to one cell; fine cells grouped into coarse cells of 8^3 by the key).  A face is registered in every
// fine cell the box of its corners overlaps: a count per face, an inclusive scan by the caller, a fill of (cell key, face) at the
// face's own offset, a stable sort by key -- so a cell's faces stand in ascending order and the table is the same on every run.
// A face whose box overlaps more than kMdCellCap cells is not registered: it goes to the oversize list, which every query
// tests first.  The pair table therefore holds at most kMdCellCap * nf entries.
//
// Query.  Every point of a face lies in a cell the face is registered in, so
//     dist(q, mesh) = min over (cell C, face f in C) of dist(q, f within C)   and   dist(q, f within C) >= dist(q, C).
// A cell is skipped only when a lower bound on dist(q, C), less the plan's slack, exceeds the best distance found; a face that
// is examined contributes its full distance.  The lane walks shells of fine cells by nn_walk (nsr_recon.h), whose bound on
// everything outside the walked box holds for the part of a face out there as it does for a point; a query still open after
// kNnFineShells shells takes the coarse route: an upper bound from one corner of one face per occupied coarse cell, then every
// coarse cell, and inside it every fine cell, whose box can hold a point at or below the bound.  Ties of bit-equal squared
// distance go to the smallest face index.
#pragma once

namespace nsr {

constexpr int kMdCellCap = 32;                  // cells a face may be registered in; more: the oversize list

struct MdParams {
    NnGrid G;                        // the grid over the box of the vertices; its runs are runs of pface
    const void *verts;               // [nv][3] fp32 or fp64
    const int *faces;                // [nf][3]
    long long nv, nf;
    int vfp64, qfp64;
    long long npairs, nover;
    long long *count, *over;         // [nf] out (count): cells of the face (0: oversize or invalid), 1 if oversize
    const long long *cum;            // [nf] inclusive scan of count (fill)
    const long long *ocum;           // [nf] inclusive scan of over (build)
    long long *keys, *pair_face;     // [npairs] out (fill)
    const long long *skeys, *order;  // [npairs] sorted keys and the permutation that sorts them (build)
    const long long *pairs;          // [npairs] the fill's pair_face (build)
    double *tri;                     // [nf][9] the corners, fp64 (zeros for an invalid face)
    int *pface;                      // [npairs] faces in key order
    int *olist;                      // [nover] oversize faces, ascending
    double *crep;                    // [ncoarse][3] a corner of a face registered in the coarse cell
    const void *q;                   // [n][3] queries
    long long n;
    const long long *qorder;
    double *dist;                    // [n]
    long long *face;                 // [n]
    double *closest;                 // [n][3]
    int *ncand;                      // [n] optional: faces examined
};

NSR_DEV double md_dot(double ax, double ay, double az, double bx, double by, double bz) { return (ax * bx + ay * by) + az * bz; }

// closest point of the segment s -> e; returns the squared distance
NSR_DEV double md_segment(double px, double py, double pz, double sx, double sy, double sz, double ex, double ey, double ez,
                          double &x, double &y, double &z) {
    const double dx = ex - sx, dy = ey - sy, dz = ez - sz;
    const double l = md_dot(dx, dy, dz, dx, dy, dz);
    const double t = md_dot(px - sx, py - sy, pz - sz, dx, dy, dz) / l;       // 0 / 0 when the segment is a point: l == 0 decides
    if (l == 0.0 || !(t > 0.0)) { x = sx; y = sy; z = sz; }
    else if (t >= 1.0) { x = ex; y = ey; z = ez; }
    else { x = sx + dx * t; y = sy + dy * t; z = sz + dz * t; }
    const double rx = px - x, ry = py - y, rz = pz - z;
    return (rx * rx + ry * ry) + rz * rz;
}

// closest point (x, y, z) of the closed triangle t[0..8] = (a, b, c) to p; returns the squared distance
NSR_DEV double md_face(const double *t, double px, double py, double pz, double &x, double &y, double &z) {
    const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
    const double abx = bx - ax, aby = by - ay, abz = bz - az;
    const double acx = cx - ax, acy = cy - ay, acz = cz - az;
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    bool degen = nx == 0.0 && ny == 0.0 && nz == 0.0;
    if (!degen) {
        const double d1 = md_dot(abx, aby, abz, px - ax, py - ay, pz - az), d2 = md_dot(acx, acy, acz, px - ax, py - ay, pz - az);
        const double d3 = md_dot(abx, aby, abz, px - bx, py - by, pz - bz), d4 = md_dot(acx, acy, acz, px - bx, py - by, pz - bz);
        const double d5 = md_dot(abx, aby, abz, px - cx, py - cy, pz - cz), d6 = md_dot(acx, acy, acz, px - cx, py - cy, pz - cz);
        const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
        if (d1 <= 0.0 && d2 <= 0.0) { x = ax; y = ay; z = az; }
        else if (d3 >= 0.0 && d4 <= d3) { x = bx; y = by; z = bz; }
        else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
            const double den = d1 - d3, v = d1 / den;
            degen = !(den > 0.0 || den < 0.0);
            x = ax + abx * v; y = ay + aby * v; z = az + abz * v;
        } else if (d6 >= 0.0 && d5 <= d6) { x = cx; y = cy; z = cz; }
        else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
            const double den = d2 - d6, w = d2 / den;
            degen = !(den > 0.0 || den < 0.0);
            x = ax + acx * w; y = ay + acy * w; z = az + acz * w;
        } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
            const double den = (d4 - d3) + (d5 - d6), w = (d4 - d3) / den;
            degen = !(den > 0.0 || den < 0.0);
            x = bx + (cx - bx) * w; y = by + (cy - by) * w; z = bz + (cz - bz) * w;
        } else {
            const double den = (va + vb) + vc, v = vb / den, w = vc / den;
            degen = !(den > 0.0 || den < 0.0) || !(va > 0.0 && vb > 0.0 && vc > 0.0);
            x = (ax + abx * v) + acx * w; y = (ay + aby * v) + acy * w; z = (az + abz * v) + acz * w;
        }
    }
    if (!degen) {
        const double rx = px - x, ry = py - y, rz = pz - z;
        return (rx * rx + ry * ry) + rz * rz;
    }
    double best = md_segment(px, py, pz, ax, ay, az, bx, by, bz, x, y, z);
    double sx, sy, sz;
    double d = md_segment(px, py, pz, bx, by, bz, cx, cy, cz, sx, sy, sz);
    if (d < best) { best = d; x = sx; y = sy; z = sz; }
    d = md_segment(px, py, pz, cx, cy, cz, ax, ay, az, sx, sy, sz);
    if (d < best) { best = d; x = sx; y = sy; z = sz; }
    return best;
}

// the corners of face f, fp64; false for an index outside the vertex array
NSR_DEV bool md_corners(const void *verts, int fp64, long long nv, const int *faces, long long f, double *t) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return false;
    nn_load(verts, fp64, i0, t[0], t[1], t[2]);
    nn_load(verts, fp64, i1, t[3], t[4], t[5]);
    nn_load(verts, fp64, i2, t[6], t[7], t[8]);
    return true;
}

// the fine cells the box of face f overlaps: [c0, c1] per axis; returns their number (0: invalid face)
NSR_DEV long long md_range(const MdParams &P, long long f, int &x0, int &x1, int &y0, int &y1, int &z0, int &z1) {
    double t[9];
    if (!md_corners(P.verts, P.vfp64, P.nv, P.faces, f, t)) return 0;
    x0 = nn_cell(P.G, 0, nn_min(nn_min(t[0], t[3]), t[6])); x1 = nn_cell(P.G, 0, nn_max(nn_max(t[0], t[3]), t[6]));
    y0 = nn_cell(P.G, 1, nn_min(nn_min(t[1], t[4]), t[7])); y1 = nn_cell(P.G, 1, nn_max(nn_max(t[1], t[4]), t[7]));
    z0 = nn_cell(P.G, 2, nn_min(nn_min(t[2], t[5]), t[8])); z1 = nn_cell(P.G, 2, nn_max(nn_max(t[2], t[5]), t[8]));
    if (x1 < x0 || y1 < y0 || z1 < z0) return 0;                    // (a NaN corner: the Python layer rejects it)
    return (long long)(x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1);
}

NSR_KERNEL void md_count_kernel(const MdParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f >= P.nf) return;
    int x0, x1, y0, y1, z0, z1;
    const long long c = md_range(P, f, x0, x1, y0, y1, z0, z1);
    P.count[f] = c > kMdCellCap ? 0 : c;
    P.over[f] = c > kMdCellCap ? 1 : 0;
}

NSR_KERNEL void md_fill_kernel(const MdParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f >= P.nf) return;
    int x0, x1, y0, y1, z0, z1;
    const long long c = md_range(P, f, x0, x1, y0, y1, z0, z1);
    if (c < 1 || c > kMdCellCap) return;
    const long long end = P.cum[f], base = end - c;
    if (base < 0 || end > P.npairs) return;                          // a scan that is not the count's: nothing is written
    long long j = base;
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y)
            for (int z = z0; z <= z1; ++z) {
                if (j >= end) return;
                P.keys[j] = nn_key(P.G, x, y, z);
                P.pair_face[j] = f;
                ++j;
            }
}

NSR_KERNEL void md_tri_kernel(const MdParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f >= P.nf) return;
    double t[9];
    const bool ok = md_corners(P.verts, P.vfp64, P.nv, P.faces, f, t);
    for (int k = 0; k < 9; ++k) P.tri[9 * f + k] = ok ? t[k] : 0.0;
    if (P.over[f] != 0) {
        const long long o = P.ocum[f] - 1;
        if (o >= 0 && o < P.nover) P.olist[o] = (int)f;
    }
}

// faces in key order + the runs of every fine and coarse cell (after md_tri_kernel: a coarse cell's corner is read from tri)
NSR_KERNEL void md_gather_kernel(const MdParams P) {
    const long long j = (long long)bid_x() * nthreads() + tid();
    if (j >= P.npairs) return;
    const long long o = P.order[j];
    long long fi = (o >= 0 && o < P.npairs) ? P.pairs[o] : 0;
    if (fi < 0 || fi >= P.nf) fi = 0;
    P.pface[j] = (int)fi;
    const long long c = nn_mark_runs(P.G, P.skeys, j, P.npairs);
    if (c >= 0)
        for (int d = 0; d < 3; ++d) P.crep[3 * c + d] = P.tri[9 * fi + d];
}

struct MdBest { double d2; long long f; double x, y, z; int cand; };

NSR_DEV void md_try(const MdParams &P, double qx, double qy, double qz, long long f, MdBest &B) {
    if (f < 0 || f >= P.nf) return;
    double x, y, z;
    const double d2 = md_face(P.tri + 9 * f, qx, qy, qz, x, y, z);
    ++B.cand;
    if (d2 < B.d2 || (d2 == B.d2 && f < B.f)) { B.d2 = d2; B.f = f; B.x = x; B.y = y; B.z = z; }
}

NSR_DEV void md_scan(const MdParams &P, double qx, double qy, double qz, int s, int e, MdBest &B) {
    for (int j = s; j < e; ++j) md_try(P, qx, qy, qz, P.pface[j], B);
}

// squared distance from q to the box of the cells [c0, c1) along every axis (cell units of h from lo)
NSR_DEV double md_box_near2(const MdParams &P, const double q[3], const int c0[3], const int c1[3]) {
    double near2 = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double a = (P.G.lo[d] + (double)c0[d] * P.G.h) - q[d], b = q[d] - (P.G.lo[d] + (double)c1[d] * P.G.h);
        const double g = a > 0.0 ? a : (b > 0.0 ? b : 0.0);
        near2 += g * g;
    }
    return near2;
}

// the fine cells of coarse cell k whose box can hold a point at or below the current bound min(B.d2, U2)
NSR_DEV void md_scan_coarse(const MdParams &P, const double q[3], long long k, double U2, double slack, MdBest &B) {
    const NnGrid &G = P.G;
    const int kz = (int)(k % G.nc[2]), ky = (int)((k / G.nc[2]) % G.nc[1]), kx = (int)(k / ((long long)G.nc[2] * G.nc[1]));
    const int c0[3] = {kx * kNnLocal, ky * kNnLocal, kz * kNnLocal};
    int c1[3];
    for (int d = 0; d < 3; ++d) c1[d] = c0[d] + kNnLocal < G.nd[d] ? c0[d] + kNnLocal : G.nd[d];
    {
        const double lim2 = B.d2 < U2 ? B.d2 : U2;
        const double nr = sqrt(md_box_near2(P, q, c0, c1)) - slack;
        if (!(nr <= 0.0 || nr * nr <= lim2 * (1.0 + 1e-12))) return;
    }
    for (int x = c0[0]; x < c1[0]; ++x)
        for (int y = c0[1]; y < c1[1]; ++y)
            for (int z = c0[2]; z < c1[2]; ++z) {
                const long long f = nn_fine_id(G, x, y, z);
                const int s = G.fstart[f], e = G.fend[f];
                if (s >= e) continue;
                const int f0[3] = {x, y, z}, f1[3] = {x + 1, y + 1, z + 1};
                const double lim2 = B.d2 < U2 ? B.d2 : U2;
                const double nr = sqrt(md_box_near2(P, q, f0, f1)) - slack;
                if (nr <= 0.0 || nr * nr <= lim2 * (1.0 + 1e-12)) md_scan(P, q[0], q[1], q[2], s, e, B);
            }
}

struct MdFaceSink {                                             // the table is pface: the faces of every cell in key order
    const MdParams &P;
    MdBest &B;
    NSR_DEV void scan(const double q[3], int s, int e) const { md_scan(P, q[0], q[1], q[2], s, e, B); }
    NSR_DEV double best2() const { return B.d2; }
};

// one thread per query, in key order (P.qorder), so that a wave's lanes walk neighbouring cells
NSR_KERNEL void md_query_kernel(const MdParams P) {
    const long long t = (long long)bid_x() * nthreads() + tid();
    if (t >= P.n) return;
    const long long qi = P.qorder ? P.qorder[t] : t;
    if (qi < 0 || qi >= P.n) return;
    const NnGrid &G = P.G;
    double q[3], slack;
    nn_load(P.q, P.qfp64, qi, q[0], q[1], q[2]);
    MdBest B{__builtin_huge_val(), -1, 0.0, 0.0, 0.0, 0};
    for (long long k = 0; k < P.nover; ++k) md_try(P, q[0], q[1], q[2], P.olist[k], B);
    MdFaceSink sink{P, B};
    if (P.npairs != 0 && !nn_walk(G, q, sink, slack)) {
        // coarse route: an upper bound on the answer from one corner of one face of every occupied coarse cell, then a scan of
        // the fine cells, coarse cell by coarse cell, whose box can hold a point at or below the current bound
        double U2 = B.d2;
        for (long long k = 0; k < G.ncoarse; ++k) {
            if (G.cstart[k] >= G.cend[k]) continue;
            const double dx = q[0] - P.crep[3 * k], dy = q[1] - P.crep[3 * k + 1], dz = q[2] - P.crep[3 * k + 2];
            const double u = (dx * dx + dy * dy) + dz * dz;
            U2 = u < U2 ? u : U2;
        }
        for (long long k = 0; k < G.ncoarse; ++k)
            if (G.cstart[k] < G.cend[k]) md_scan_coarse(P, q, k, U2, slack, B);
    }
    P.dist[qi] = sqrt(B.d2);
    P.face[qi] = B.f;
    P.closest[3 * qi] = B.x; P.closest[3 * qi + 1] = B.y; P.closest[3 * qi + 2] = B.z;
    if (P.ncand) P.ncand[qi] = B.cand;
}

// ------------------------------------------------------------------------------------------------
// Normals.  n = (b - a) x (c - a) in the expression order of md_face, divided by sqrt((nx*nx + ny*ny) + nz*nz); the zero
// vector when that length is not > 0 (a degenerate face).  The statistics pair query normal i with the normal of face[i]:
// (|n . m|, 1) when neither is the zero vector and the face index is valid, else (0, 0); summed as nsr_dist_stats sums, by
// the same kernels (reduce_kernel<kRedNormal>, nsr_recon.h).
// ------------------------------------------------------------------------------------------------
struct MdNormalParams {
    const void *verts;
    const int *faces;
    long long nv, nf;
    int vfp64;
    double *normals;                 // [nf][3] out
};

NSR_KERNEL void md_normals_kernel(const MdNormalParams P) {
    const long long f = (long long)bid_x() * nthreads() + tid();
    if (f >= P.nf) return;
    double t[9];
    double nx = 0.0, ny = 0.0, nz = 0.0;
    if (md_corners(P.verts, P.vfp64, P.nv, P.faces, f, t)) {
        const double abx = t[3] - t[0], aby = t[4] - t[1], abz = t[5] - t[2];
        const double acx = t[6] - t[0], acy = t[7] - t[1], acz = t[8] - t[2];
        nx = aby * acz - abz * acy; ny = abz * acx - abx * acz; nz = abx * acy - aby * acx;
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        if (len > 0.0) { nx = nx / len; ny = ny / len; nz = nz / len; }
        else { nx = 0.0; ny = 0.0; nz = 0.0; }
    }
    P.normals[3 * f] = nx; P.normals[3 * f + 1] = ny; P.normals[3 * f + 2] = nz;
}

}  // namespace nsr
