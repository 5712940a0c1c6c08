// nsr_view.h -- the colour side of the rasterizer, for the headless replay of a SLAM run (include/nsr.h, "Replay view"): what the
// reference's visualizer.py draws in an Open3D window (src/tools/viz.py: a shaded mesh with back faces hidden, camera wireframes
// and trajectories as point clouds).  Three pieces: area-weighted vertex normals, a mesh layer (depth, owning face, shaded colour)
// over the bins of nsr_raster.h, and a point layer drawn over a base layer with a depth test.
// Included by nsr_api.cpp after nsr_raster.h: the mesh layer runs that header's fragment pass (raster_tile_pass) over its
// parameters and bins with a sink of its own, so coverage, depth and near / far are one piece of code for both.
//
// Numerical contract (tests/view_reference.py restates it in numpy, in this operation order):
//   Normals    per vertex the sum of (V1 - V0) x (V2 - V0) over its incident faces: area-weighted, which is what Open3D's
//              compute_vertex_normals does as recalled.  Differences, products and sums in fp64 from the fp32 coordinates
//              (x: uy wz - uz wy, y: uz wx - ux wz, z: ux wy - uy wx), added per component in the order of the incidence list
//              (ascending face id; a face that names the vertex twice is listed twice and is degenerate: it adds zeros).  No
//              atomics: one thread per vertex walks its CSR list.  Stored twice: the fp64 sums, and (float)(s / sqrt((sx sx + sy
//              sy) + sz sz)) per component; a sum of length 0 (or a non-finite one) stays (0, 0, 0).
//   Mesh       camera, vertex pass, coverage, edge values, depth, near / far: nsr_raster.h's own code (raster_tile_pass).  Cull mode,
//              per face, by the sign of the plane numerator num = n . V0 (n = (V1 - V0) x (V2 - V0), the camera at the origin):
//              none keeps every face, back keeps the faces with num < 0 (the normal points to the camera: counter-clockwise on
//              screen in a right-handed frame, OpenGL's front face), front keeps the others.  A culled face produces no fragment;
//              with none the depth image is nsr_raster_depth's bit for bit.
//   Owner      of a pixel: among the kept fragments whose (float)Z is the smallest, the smallest face id.  One ds_min_u64 on the
//              key (bits of (float)Z) << 32 | face id resolves both in one pass over the bin, order-independently (a second
//              32-bit tile would need the finished z-buffer first, that is the bin and its fp64 fragment work twice).
//   Weights    of the owner at the pixel: its three sign-corrected edge values e01, e12, e20 (recomputed by the coverage's own
//              expression), s = (e01 + e12) + e20, w0 = e12 / s, w1 = e20 / s, w2 = e01 / s in fp64.  The edge values are taken
//              in camera space, so the weights are perspective-correct.  A quantity q is interpolated as (w0 q0 + w1 q1) + w2 q2.
//   Shading    a headlight, two-sided: N = the interpolated vertex normal (world space, fp32 inputs), D = the pixel ray in world
//              space, D_j = ((double)w_0j dx + (double)w_1j dy) + (double)w_2j (the rotation of w2c transposed), c = (Nx Dx + Ny
//              Dy) + Nz Dz, nn = (Nx Nx + Ny Ny) + Nz Nz, dd likewise; s = a + (1 - a) (|c| / sqrt(nn dd)), a = 0.35; nn = 0
//              gives s = a.  Albedo: the interpolated vertex colour, (double)u8 / 255 per vertex, or 0.8 per channel for a mesh
//              without colours.  x = albedo s clipped to [0, 1]; channel = (u8)floor(255 x + 0.5).  Background: white, depth 0,
//              face -1.
//   Points     B frames; frame b draws points offsets[b] .. offsets[b + 1] of one array (xyz fp32, rgb u8) with its own w2c over
//              base layer b (or over the one shared base layer) into output image b.  Vertex pass as above (fp32).  A point with
//              (double)c_z < near or > far is dropped.  u = ((double)c_x / z) fx + cx, v likewise, fp64; a point of size s covers
//              columns i0 <= i < i0 + s, i0 = floor((u - s / 2) + 0.5), rows likewise, clipped to the image.  A pixel of it is
//              drawn iff the base depth there is 0 or c_z <= the base depth (fp32).  Among the points drawn on a pixel the
//              smallest c_z wins, then the smallest index in the frame (one ds_min_u64 on bits(c_z) << 32 | index).  The pixel
//              takes the point's colour unshaded; every other pixel copies the base.
//
// Launches: normals: one thread per vertex.  Mesh: nsr_raster_bin as it is, raster_emit_kernel, then view_resolve_kernel, one
// block per (tile, view): raster_tile_pass with 64-bit keys (ViewKeySink), then 4 pixels a thread for weights and shading.
// Points: one block per (tile, frame), every thread takes a point per round of 256.  No global atomics, each pixel stored once:
// every result is bit-identical run to run.
#pragma once

namespace nsr {

constexpr int kViewCullNone = 0, kViewCullBack = 1, kViewCullFront = 2;
constexpr int kViewMaxPointSize = 64;
constexpr double kViewAmbient = 0.35;
constexpr unsigned long long kViewEmpty = ~0ull;

// ------------------------------------------------------------------------------------------------
// Vertex normals
// ------------------------------------------------------------------------------------------------
struct NormalParams {
    const float *verts;              // [nv][3]
    const int *faces;                // [nf][3]
    long long nv, nf;
    const long long *start;          // [nv + 1] CSR offsets into incident
    const int *incident;             // [start[nv]] face ids, ascending per vertex
    long long n_incident;            // entries the caller's list holds: nothing beyond is read
    double *sums;                    // [nv][3] (may be null)
    float *normals;                  // [nv][3]
};

NSR_KERNEL void view_normals_kernel(const NormalParams P) {
    const long long v = (long long)bid_x() * kRasterThreads + tid();
    if (v >= P.nv) return;
    long long e0 = P.start[v], e1 = P.start[v + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > P.n_incident ? P.n_incident : e1;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (long long e = e0; e < e1; ++e) {
        const long long f = P.incident[e];
        if (f < 0 || f >= P.nf) continue;
        const int i0 = P.faces[3 * f], i1 = P.faces[3 * f + 1], i2 = P.faces[3 * f + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= P.nv || i1 >= P.nv || i2 >= P.nv) continue;
        const float *A = P.verts + 3ll * i0, *B = P.verts + 3ll * i1, *C = P.verts + 3ll * i2;
        const double ax = A[0], ay = A[1], az = A[2];
        const double ux = (double)B[0] - ax, uy = (double)B[1] - ay, uz = (double)B[2] - az;
        const double wx = (double)C[0] - ax, wy = (double)C[1] - ay, wz = (double)C[2] - az;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    if (P.sums) { P.sums[3 * v] = sx; P.sums[3 * v + 1] = sy; P.sums[3 * v + 2] = sz; }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    const bool ok = len > 0.0 && len <= 1.7976931348623157e308;
    P.normals[3 * v] = ok ? (float)(sx / len) : 0.f;
    P.normals[3 * v + 1] = ok ? (float)(sy / len) : 0.f;
    P.normals[3 * v + 2] = ok ? (float)(sz / len) : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Mesh layer
// ------------------------------------------------------------------------------------------------
struct MeshViewParams {
    RasterParams R;                  // as nsr_raster_depth sets it up (R.depth: the depth image)
    const float *normals;            // [nv][3] world-space vertex normals
    const unsigned char *colors;     // [nv][3] (null: 0.8 grey)
    int cull;
    int *face;                       // [K][H][W]
    unsigned char *rgb;              // [K][H][W][3]
};

// the mesh layer's sink of raster_tile_pass: the faces the cull mode keeps, depth bits << 32 | face id
struct ViewKeySink {
    typedef unsigned long long Cell;
    static constexpr Cell kEmpty = kViewEmpty;
    static constexpr bool kFaceId = true;
    int cull;
    NSR_DEV bool keeps(double num) const {
        const bool facing = num < 0.0;                               // the normal points to the camera
        return !((cull == kViewCullBack && !facing) || (cull == kViewCullFront && facing));
    }
    NSR_DEV Cell cell(float z, unsigned face) const { return ((unsigned long long)__builtin_bit_cast(unsigned, z) << 32) | face; }
};
constexpr int kViewResolveLds = raster_resolve_lds<ViewKeySink>();

// the sign-corrected value of edge (a, b) of a face at the ray (dx, dy, 1): the coverage's expression
NSR_DEV double view_edge_value(const float *Va, const float *Vb, int ia, int ib, double dx, double dy) {
    double N[3];
    const bool canon = ia <= ib;
    raster_edge(canon ? Va : Vb, canon ? Vb : Va, N);
    if (!canon) { N[0] = -N[0]; N[1] = -N[1]; N[2] = -N[2]; }
    return (dx * N[0] + dy * N[1]) + N[2];
}

NSR_DEV unsigned char view_u8(double x) {
    x = x < 0.0 ? 0.0 : x;
    x = x > 1.0 ? 1.0 : x;
    return (unsigned char)(int)floor(255.0 * x + 0.5);
}

NSR_KERNEL void view_resolve_kernel(const MeshViewParams M) {
    const RasterParams &P = M.R;
    const unsigned long long *zb = raster_tile_pass(P, ViewKeySink{M.cull});
    const double *sD = reinterpret_cast<const double *>(lds_base() + kRzDir);
    const int t = tid(), k = bid_y(), tile = bid_x();
    const int gx0 = (tile % P.tx) * kRasterTile, gy0 = (tile / P.tx) * kRasterTile;
    const float *cam = P.cam + 4 * (long long)k * P.nv;
    const float *w = P.w2c + 12 * k;
    for (int e = t; e < kRasterTile * kRasterTile; e += kRasterThreads) {
        const int lx = e % kRasterTile, ly = e / kRasterTile, x = gx0 + lx, y = gy0 + ly;
        if (x >= P.W || y >= P.H) continue;
        const long long pix = ((long long)k * P.H + y) * P.W + x;
        const unsigned long long key = zb[e];
        unsigned char *o = M.rgb + 3 * pix;
        if (key == kViewEmpty) {
            P.depth[pix] = 0.f;
            M.face[pix] = -1;
            o[0] = 255; o[1] = 255; o[2] = 255;
            continue;
        }
        const int f = (int)(unsigned)(key & 0xffffffffull);
        P.depth[pix] = __builtin_bit_cast(float, (unsigned)(key >> 32));
        M.face[pix] = f;
        const int i0 = P.faces[3ll * f], i1 = P.faces[3ll * f + 1], i2 = P.faces[3ll * f + 2];     // in range: the face drew a fragment
        const float *A = cam + 4ll * i0, *B = cam + 4ll * i1, *C = cam + 4ll * i2;
        const double dx = sD[lx], dy = sD[kRasterTile + ly];
        const double e01 = view_edge_value(A, B, i0, i1, dx, dy);
        const double e12 = view_edge_value(B, C, i1, i2, dx, dy);
        const double e20 = view_edge_value(C, A, i2, i0, dx, dy);
        const double s = (e01 + e12) + e20;
        const double w0 = e12 / s, w1 = e20 / s, w2 = e01 / s;
        const float *n0 = M.normals + 3ll * i0, *n1 = M.normals + 3ll * i1, *n2 = M.normals + 3ll * i2;
        const double Nx = (w0 * (double)n0[0] + w1 * (double)n1[0]) + w2 * (double)n2[0];
        const double Ny = (w0 * (double)n0[1] + w1 * (double)n1[1]) + w2 * (double)n2[1];
        const double Nz = (w0 * (double)n0[2] + w1 * (double)n1[2]) + w2 * (double)n2[2];
        const double Dx = ((double)w[0] * dx + (double)w[4] * dy) + (double)w[8];
        const double Dy = ((double)w[1] * dx + (double)w[5] * dy) + (double)w[9];
        const double Dz = ((double)w[2] * dx + (double)w[6] * dy) + (double)w[10];
        const double c = (Nx * Dx + Ny * Dy) + Nz * Dz;
        const double nn = (Nx * Nx + Ny * Ny) + Nz * Nz, dd = (Dx * Dx + Dy * Dy) + Dz * Dz;
        double shade = kViewAmbient;
        if (nn > 0.0) shade = kViewAmbient + (1.0 - kViewAmbient) * (fabs(c) / sqrt(nn * dd));
        for (int q = 0; q < 3; ++q) {
            double alb = 0.8;
            if (M.colors)
                alb = (w0 * ((double)M.colors[3ll * i0 + q] / 255.0) + w1 * ((double)M.colors[3ll * i1 + q] / 255.0)) +
                      w2 * ((double)M.colors[3ll * i2 + q] / 255.0);
            o[q] = view_u8(alb * shade);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Point layer
// ------------------------------------------------------------------------------------------------
struct PointViewParams {
    const float *pts;                // [n][3]
    const unsigned char *colors;     // [n][3]
    const long long *offsets;        // [B + 1]
    long long n;                     // points the arrays hold: nothing beyond is read
    const float *w2c;                // [B][12]
    int B, H, W, tx, ty, ntiles, size, base_per_frame;
    double fx, fy, cx, cy, near, far;
    const unsigned char *base_rgb;   // [B or 1][H][W][3]
    const float *base_depth;         // [B or 1][H][W]
    unsigned char *rgb;              // [B][H][W][3]
    int *owner;                      // [B][H][W] index in the frame of the point drawn, -1: the base (may be null)
};

NSR_KERNEL void view_points_kernel(const PointViewParams P) {
    unsigned long long *zb = reinterpret_cast<unsigned long long *>(lds_base());     // [32 * 32]
    const int t = tid(), b = bid_y(), tile = bid_x();
    const int gx0 = (tile % P.tx) * kRasterTile, gy0 = (tile / P.tx) * kRasterTile;
    for (int e = t; e < kRasterTile * kRasterTile; e += kRasterThreads) zb[e] = kViewEmpty;
    block_sync();
    long long p0 = P.offsets[b], p1 = P.offsets[b + 1];
    p0 = p0 < 0 ? 0 : p0;
    p1 = p1 > P.n ? P.n : p1;
    const float *w = P.w2c + 12 * b;
    const float *based = P.base_depth + (P.base_per_frame ? (long long)b * P.H * P.W : 0);
    const double half = 0.5 * (double)P.size;
    for (long long p = p0 + t; p < p1; p += kRasterThreads) {
        const float x = P.pts[3 * p], y = P.pts[3 * p + 1], z = P.pts[3 * p + 2];
        const float cz = ((w[8] * x + w[9] * y) + w[10] * z) + w[11];
        const double zd = (double)cz;
        if (!(zd >= P.near && zd <= P.far)) continue;
        const float xc = ((w[0] * x + w[1] * y) + w[2] * z) + w[3];
        const float yc = ((w[4] * x + w[5] * y) + w[6] * z) + w[7];
        const double u = ((double)xc / zd) * P.fx + P.cx, v = ((double)yc / zd) * P.fy + P.cy;
        const double fi = floor((u - half) + 0.5), fj = floor((v - half) + 0.5);
        if (!(fi > -(double)(P.size) && fi < (double)P.W && fj > -(double)(P.size) && fj < (double)P.H)) continue;   // a NaN is outside
        const int i0 = (int)fi, j0 = (int)fj;
        int x0 = i0 - gx0, x1 = i0 + P.size - 1 - gx0, y0 = j0 - gy0, y1 = j0 + P.size - 1 - gy0;
        x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
        x1 = x1 > kRasterTile - 1 ? kRasterTile - 1 : x1; y1 = y1 > kRasterTile - 1 ? kRasterTile - 1 : y1;
        if (gx0 + x1 > P.W - 1) x1 = P.W - 1 - gx0;
        if (gy0 + y1 > P.H - 1) y1 = P.H - 1 - gy0;
        const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, cz) << 32) | (unsigned long long)(unsigned)(p - p0);
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
                const float d = based[(long long)(gy0 + yy) * P.W + gx0 + xx];
                if (d == 0.f || cz <= d) raster_lds_min(zb + yy * kRasterTile + xx, key);
            }
    }
    block_sync();
    const unsigned char *baser = P.base_rgb + (P.base_per_frame ? 3ll * b * P.H * P.W : 0);
    for (int e = t; e < kRasterTile * kRasterTile; e += kRasterThreads) {
        const int x = gx0 + (e % kRasterTile), y = gy0 + (e / kRasterTile);
        if (x >= P.W || y >= P.H) continue;
        const long long pl = (long long)y * P.W + x, pix = (long long)b * P.H * P.W + pl;
        const unsigned long long key = zb[e];
        const bool hit = key != kViewEmpty;
        const long long idx = (long long)(key & 0xffffffffull);
        const unsigned char *src = hit ? P.colors + 3 * (p0 + idx) : baser + 3 * pl;
        unsigned char *o = P.rgb + 3 * pix;
        o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
        if (P.owner) P.owner[pix] = hit ? (int)idx : -1;
    }
}

}  // namespace nsr
