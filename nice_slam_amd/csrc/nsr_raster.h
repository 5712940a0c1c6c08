// nsr_raster.h -- depth rasterization of triangle meshes and the pieces of the 2-D depth metric around it (include/nsr.h,
// "Depth rasterization"): a tiled z-buffer rasterizer, the per-view depth L1 and the view-acceptance test of the candidate
// poses (src/tools/eval_recon.py:131-211, calc_2d_metric, which renders with Open3D's OpenGL visualizer, and check_proj).
// Included by nsr_api.cpp after nsr_recon.h, whose cull_sees it reuses, and nsr_kernels.h, whose device primitives it uses.
// The fragment pass of the resolve (raster_tile_pass) is also the replay view's: nsr_view.h runs it with a sink of its own.
//
// Numerical contract (tests/raster_reference.py restates it in numpy, in this operation order):
//   Camera     c2w in the OpenCV convention (x right, y down, z forward: Open3D's extrinsic = inv(c2w)); the caller inverts it
//              in fp64 and passes w2c rows 0..2 rounded to fp32.  The centre of pixel (i, j) (column i, row j) is the ray
//              d = ((i - cx) / fx, (j - cy) / fy, 1), each component in fp64.
//   Vertices   once per view, in fp32: c_r = ((w_r0 x + w_r1 y) + w_r2 z) + w_r3 (plain products and sums, no contraction:
//              the build uses -ffp-contract=off, as cull_sees).  Every triangle reads this one copy of its vertices, so the
//              two triangles on an edge see the same numbers.
//   Coverage   the pixel-centre ray against the triangle in camera space, no projection, no side clipping.  Edge (a, b) is
//              evaluated in its canonical orientation (smaller vertex index first): N = Va x Vb in fp64 from the fp32
//              coordinates (x: Ay Bz - Az By, y: Az Bx - Ax Bz, z: Ax By - Ay Bx), e = (dx Nx + dy Ny) + Nz, negated when the
//              triangle runs the edge the other way.  Covered iff e01, e12, e20 are all >= 0 or all <= 0 and not all 0: a
//              point on the boundary is inside, a degenerate triangle covers nothing, nothing is back-face culled (the
//              reference sets mesh_show_back_face).  Two triangles on an edge evaluate the same number: no crack.
//   Depth      n = (V1 - V0) x (V2 - V0), Z = ((nx V0x + ny V0y) + nz V0z) / ((nx dx + ny dy) + nz), all fp64 (V0: the face's
//              first vertex).  Kept iff near <= Z <= far (fp64; discarding per fragment is OpenGL's near / far clipping of
//              the geometry), stored as (float)Z; the smallest wins; a pixel without a fragment reads 0 (Open3D's background).
//              fp64 rather than fp32 for the setup and the per-pixel work: products of fp32 coordinates are exact in fp64, so
//              the edge values lose nothing to cancellation on small, distant triangles, and numpy states fp64 bit for bit
//              as easily as fp32; gfx950 issues fp64 adds and multiplies at the rate of unpacked fp32 ones.
//   Depth L1   per view: the fixed-order fp64 sum of |(double)a - (double)b| over the H x W pixels (trees of 256 in block
//              order, as reduce_kernel), divided by H W.
//   Views      check_proj as cull_sees states it: flipped c2w (y, z columns negated), w2c = inv in fp64 rounded to fp32,
//              points rounded to fp32, x negated, z + 1e-5; a candidate "sees" the cloud iff some point projects inside.
//
// Pipeline per batch of K views (one launch each): vertex pass -> per-(view, triangle) pixel bounding box -> binning into
// kRasterTile^2 screen tiles (count per (tile, chunk of kRasterChunk triangles), prefix scans, emit in triangle order) ->
// resolve, one block per (view, tile): the tile's z-buffer in LDS (ds_min_u32 on the bits of positive floats is
// order-independent), work split per (triangle, pixel row), each pixel written once with a plain store.  No global atomics:
// every result is bit-identical run to run.
#pragma once

namespace nsr {

constexpr int kRasterTile = 32;                  // screen tile edge (pixels)
constexpr int kRasterThreads = 256;              // every raster kernel: 4 waves
constexpr int kRasterChunk = kRasterThreads;     // triangles per binning block
constexpr int kRasterMaxTiles = 1024;            // per view: images up to 1024 x 1024
constexpr int kRasterViewChunk = 256;            // candidate poses per LDS chunk of the view test
constexpr unsigned kRasterEmpty = 0x7f800000u;   // +inf: no fragment yet

// min into an LDS cell: 32-bit depth bits, or 64-bit keys (depth bits << 32 | an id: nsr_view.h)
#if defined(__HIP__)
typedef __attribute__((address_space(3))) unsigned nsr_luint;
typedef __attribute__((address_space(3))) unsigned long long nsr_lu64;
NSR_DEV void raster_lds_min(unsigned *p, unsigned v) {
    __hip_atomic_fetch_min((nsr_luint *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
NSR_DEV void raster_lds_min(unsigned long long *p, unsigned long long v) {
    __hip_atomic_fetch_min((nsr_lu64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#else
template <class T> inline void raster_lds_min(T *p, T v) { if (v < *p) *p = v; }   // the emulator runs one lane at a time
#endif

struct RasterParams {
    const float *verts;              // [nv][3]
    const int *faces;                // [nf][3]
    long long nv, nf, nchunks;
    int K, H, W, tx, ty, ntiles;     // tiles per row (tx) and per column (ty)
    const float *w2c;                // [K][12] rows 0..2 of inv(c2w)
    double fx, fy, cx, cy, near, far;
    float fxf, fyf, cxf, cyf, nearf, farf;
    float *cam;                      // [K][nv][4] camera-space vertices
    int *rect;                       // [K][nf][2] pixel box (x0 | x1 << 16, y0 | y1 << 16); x0 > x1: nothing to draw
    int *counts;                     // [K][ntiles][nchunks] entries per (tile, chunk); scanned in place to offsets in the tile
    long long *tile_start;           // [K ntiles + 1] first entry of (view, tile); the last: the total
    long long *n_entries;            // [1] out (may be null)
    int *bins;                       // [cap] triangle ids, (view, tile, triangle) order
    long long cap;                   // entries the caller's bins hold (what nsr_raster_bin counted): nothing beyond is touched
    float *depth;                    // [K][H][W]
};

NSR_KERNEL void raster_vertex_kernel(const RasterParams P) {
    const long long v = (long long)bid_x() * kRasterThreads + tid();
    const int k = bid_y();
    if (v >= P.nv) return;
    const float *w = P.w2c + 12 * k;
    const float x = P.verts[3 * v], y = P.verts[3 * v + 1], z = P.verts[3 * v + 2];
    float c[4];
    for (int r = 0; r < 3; ++r) c[r] = ((w[4 * r] * x + w[4 * r + 1] * y) + w[4 * r + 2] * z) + w[4 * r + 3];
    c[3] = 0.f;
    float *o = P.cam + 4 * ((long long)k * P.nv + v);
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2]; o[3] = c[3];
}

// The pixel box of a triangle: the projections of the part of it in front of z = 0.999 near (vertices in front, edge
// crossings of that plane), widened by one pixel and clamped to the image.  Only a bound: coverage is decided per pixel.
NSR_DEV void raster_box(const RasterParams &P, const float *A, const float *B, const float *C, int &x0, int &x1, int &y0, int &y1) {
    x0 = 1; x1 = 0; y0 = 1; y1 = 0;
    const float zc = P.nearf * 0.999f, zf = P.farf * 1.001f;
    if (A[2] > zf && B[2] > zf && C[2] > zf) return;                 // wholly beyond far
    const float *V[3] = {A, B, C};
    float u0 = __builtin_huge_valf(), u1 = -__builtin_huge_valf(), v0 = __builtin_huge_valf(), v1 = -__builtin_huge_valf();
    bool any = false;
    for (int e = 0; e < 3; ++e) {
        const float *a = V[e], *b = V[(e + 1) % 3];
        float px[2], py[2], pz[2];
        int np = 0;
        if (a[2] >= zc) { px[np] = a[0]; py[np] = a[1]; pz[np] = a[2]; ++np; }
        if ((a[2] >= zc) != (b[2] >= zc)) {
            const float t = (zc - a[2]) / (b[2] - a[2]);
            px[np] = a[0] + t * (b[0] - a[0]); py[np] = a[1] + t * (b[1] - a[1]); pz[np] = zc; ++np;
        }
        for (int q = 0; q < np; ++q) {
            const float u = P.fxf * (px[q] / pz[q]) + P.cxf, v = P.fyf * (py[q] / pz[q]) + P.cyf;
            if (u != u || v != v) return;                              // non-finite geometry draws nothing
            u0 = u < u0 ? u : u0; u1 = u > u1 ? u : u1;
            v0 = v < v0 ? v : v0; v1 = v > v1 ? v : v1;
            any = true;
        }
    }
    if (!any) return;
    const float W = (float)P.W, H = (float)P.H;
    if (u1 < -2.f || v1 < -2.f || u0 > W + 1.f || v0 > H + 1.f) return;
    u0 = u0 < -2.f ? -2.f : u0; v0 = v0 < -2.f ? -2.f : v0;
    u1 = u1 > W + 1.f ? W + 1.f : u1; v1 = v1 > H + 1.f ? H + 1.f : v1;
    int a0 = (int)floorf(u0) - 1, a1 = (int)ceilf(u1) + 1, b0 = (int)floorf(v0) - 1, b1 = (int)ceilf(v1) + 1;
    a0 = a0 < 0 ? 0 : a0; b0 = b0 < 0 ? 0 : b0;
    a1 = a1 > P.W - 1 ? P.W - 1 : a1; b1 = b1 > P.H - 1 ? P.H - 1 : b1;
    if (a0 > a1 || b0 > b1) return;
    x0 = a0; x1 = a1; y0 = b0; y1 = b1;
}

NSR_KERNEL void raster_setup_kernel(const RasterParams P) {
    const long long f = (long long)bid_x() * kRasterThreads + tid();
    const int k = bid_y();
    if (f >= P.nf) return;
    const int i0 = P.faces[3 * f], i1 = P.faces[3 * f + 1], i2 = P.faces[3 * f + 2];
    int x0 = 1, x1 = 0, y0 = 1, y1 = 0;
    if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < P.nv && i1 < P.nv && i2 < P.nv) {    // a bad index draws nothing
        const float *cam = P.cam + 4 * (long long)k * P.nv;
        raster_box(P, cam + 4ll * i0, cam + 4ll * i1, cam + 4ll * i2, x0, x1, y0, y1);
    }
    int *o = P.rect + 2 * ((long long)k * P.nf + f);
    o[0] = x0 | (x1 << 16);
    o[1] = y0 | (y1 << 16);
}

// tile rectangle of a triangle (empty: tx0 > tx1)
NSR_DEV void raster_tiles(const RasterParams &P, long long f, int k, int &tx0, int &tx1, int &ty0, int &ty1) {
    tx0 = 1; tx1 = 0; ty0 = 1; ty1 = 0;
    if (f >= P.nf) return;
    const int *r = P.rect + 2 * ((long long)k * P.nf + f);
    const int x0 = r[0] & 0xffff, x1 = (r[0] >> 16) & 0xffff, y0 = r[1] & 0xffff, y1 = (r[1] >> 16) & 0xffff;
    if (x0 > x1 || y0 > y1) return;
    tx0 = x0 / kRasterTile; tx1 = x1 / kRasterTile; ty0 = y0 / kRasterTile; ty1 = y1 / kRasterTile;
}

NSR_DEV int wave_min_i(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = shfl_i(v, (tid() & 63) ^ m); v = o < v ? o : v; }
    return v;
}
NSR_DEV int wave_max_i(int v) {
    for (int m = 1; m < 64; m <<= 1) { const int o = shfl_i(v, (tid() & 63) ^ m); v = o > v ? o : v; }
    return v;
}

// One pass of a wave over the tiles its 64 triangles touch (the union of their rectangles, the same in every lane): the
// triangles of the wave that touch a tile, as a ballot.  EMIT = false: the per-wave counts into wcnt[wave][tile];
// EMIT = true: every triangle's id at its rank among the wave's, behind the earlier chunks and waves.
template <bool EMIT>
NSR_DEV void raster_wave_pass(const RasterParams &P, int k, long long chunk, int *wcnt) {
    const int lane = tid() & 63, w = tid() >> 6;
    const long long f = chunk * kRasterChunk + tid();
    int tx0, tx1, ty0, ty1;
    raster_tiles(P, f, k, tx0, tx1, ty0, ty1);
    const bool live = tx0 <= tx1;
    const int ux0 = wave_min_i(live ? tx0 : 1 << 20), ux1 = wave_max_i(live ? tx1 : -1);
    const int uy0 = wave_min_i(live ? ty0 : 1 << 20), uy1 = wave_max_i(live ? ty1 : -1);
    for (int ty = uy0; ty <= uy1; ++ty)
        for (int tx = ux0; tx <= ux1; ++tx) {
            const bool in = live && tx >= tx0 && tx <= tx1 && ty >= ty0 && ty <= ty1;
            const unsigned long long m = ballot64(in);
            const int tile = ty * P.tx + tx;
            if (!EMIT) {
                if (lane == 0) wcnt[w * P.ntiles + tile] = __builtin_popcountll(m);
            } else if (in) {
                long long pos = P.tile_start[(long long)k * P.ntiles + tile] + P.counts[((long long)k * P.ntiles + tile) * P.nchunks + chunk];
                for (int v = 0; v < w; ++v) pos += wcnt[v * P.ntiles + tile];
                pos += __builtin_popcountll(m & ((1ull << lane) - 1ull));
                if (pos >= 0 && pos < P.cap) P.bins[pos] = (int)f;
            }
        }
}

NSR_DEV void raster_wcnt_init(const RasterParams &P, int *wcnt) {
    for (int e = tid(); e < 4 * P.ntiles; e += kRasterThreads) wcnt[e] = 0;
    block_sync();
}

// grid (nchunks, K): entries of every (tile, chunk), dense, zeros included
NSR_KERNEL void raster_count_kernel(const RasterParams P) {
    int *wcnt = reinterpret_cast<int *>(lds_base());                // [4][ntiles]
    const int k = bid_y();
    const long long chunk = bid_x();
    raster_wcnt_init(P, wcnt);
    raster_wave_pass<false>(P, k, chunk, wcnt);
    block_sync();
    for (int t = tid(); t < P.ntiles; t += kRasterThreads)
        P.counts[((long long)k * P.ntiles + t) * P.nchunks + chunk] = ((wcnt[t] + wcnt[P.ntiles + t]) + wcnt[2 * P.ntiles + t]) + wcnt[3 * P.ntiles + t];
}

// grid (ntiles, K): exclusive scan of a (view, tile)'s chunk counts in place; its total into tile_start[view ntiles + tile]
NSR_KERNEL void raster_scan_tile_kernel(const RasterParams P) {
    int *s = reinterpret_cast<int *>(lds_base());                   // [2][256]
    const int t = tid();
    int *c = P.counts + ((long long)bid_y() * P.ntiles + bid_x()) * P.nchunks;
    int carry = 0;
    for (long long b = 0; b < P.nchunks; b += kRasterThreads) {
        const int v = b + t < P.nchunks ? c[b + t] : 0;
        int cur = 0;
        s[t] = v;
        block_sync();
        for (int d = 1; d < kRasterThreads; d <<= 1) {             // Hillis-Steele, ping-pong between the two halves
            const int x = s[cur * kRasterThreads + t] + (t >= d ? s[cur * kRasterThreads + t - d] : 0);
            s[(1 - cur) * kRasterThreads + t] = x;
            cur = 1 - cur;
            block_sync();
        }
        const int incl = s[cur * kRasterThreads + t], total = s[cur * kRasterThreads + kRasterThreads - 1];
        if (b + t < P.nchunks) c[b + t] = carry + incl - v;
        carry += total;
        block_sync();
    }
    if (t == 0) P.tile_start[(long long)bid_y() * P.ntiles + bid_x()] = carry;
}

// one block: tile totals -> global starts in (view, tile) order, the total behind them
NSR_KERNEL void raster_scan_view_kernel(const RasterParams P) {
    long long *s = reinterpret_cast<long long *>(lds_base());       // [256]
    const int t = tid();
    const long long n = (long long)P.K * P.ntiles, per = (n + kRasterThreads - 1) / kRasterThreads;
    const long long b0 = t * per < n ? t * per : n, b1 = (t + 1) * per < n ? (t + 1) * per : n;
    long long sum = 0;
    for (long long i = b0; i < b1; ++i) sum += P.tile_start[i];
    s[t] = sum;
    block_sync();
    if (t == 0) {
        long long run = 0;
        for (int j = 0; j < kRasterThreads; ++j) { const long long x = s[j]; s[j] = run; run += x; }
        P.tile_start[n] = run;
        if (P.n_entries) P.n_entries[0] = run;
    }
    block_sync();
    long long run = s[t];
    for (long long i = b0; i < b1; ++i) { const long long x = P.tile_start[i]; P.tile_start[i] = run; run += x; }
}

// grid (nchunks, K)
NSR_KERNEL void raster_emit_kernel(const RasterParams P) {
    int *wcnt = reinterpret_cast<int *>(lds_base());
    const int k = bid_y();
    const long long chunk = bid_x();
    raster_wcnt_init(P, wcnt);
    raster_wave_pass<false>(P, k, chunk, wcnt);
    block_sync();
    raster_wave_pass<true>(P, k, chunk, wcnt);
}

// resolve: one block per (tile, view).  LDS layout (bytes), the same for every sink; the z-buffer comes last, sized by its cell
constexpr int kRzN = 0;                                        // [9][256] double: sign-corrected edge normals
constexpr int kRzPlane = kRzN + 9 * 8 * kRasterThreads;        // [4][256] double: n, n . V0
constexpr int kRzDir = kRzPlane + 4 * 8 * kRasterThreads;      // [2][32] double: the tile's ray x and y components
constexpr int kRzBox = kRzDir + 2 * 8 * kRasterTile;           // [256] int: rows y0 | y1 << 8, cols x0 | x1 << 16 (tile-local)
constexpr int kRzRows = kRzBox + 2 * 4 * kRasterThreads;       // [2][256 + 1] int: row-count scan (ping-pong)
constexpr int kRzZ = kRzRows + 2 * 4 * (kRasterThreads + 1);   // [32 * 32] Sink::Cell: the z-buffer
static_assert(kRzZ % 8 == 0, "64-bit cells need 8-byte alignment");
template <class Sink> constexpr int raster_resolve_lds() { return kRzZ + (int)sizeof(typename Sink::Cell) * kRasterTile * kRasterTile; }

NSR_DEV void raster_edge(const float *a, const float *b, double *N) {
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
    N[0] = ay * bz - az * by;
    N[1] = az * bx - ax * bz;
    N[2] = ax * by - ay * bx;
}

// The fragments of block (tile, view) into its z-buffer in LDS, from the clear to the last fragment of the last batch of 256
// bin entries.  Returns the finished z-buffer, the block synchronised.  What a pixel holds is the sink's business:
//   Cell, kEmpty       the z-buffer cell and its value before any fragment;
//   kFaceId            whether cell() wants the item's face id (one more load per item);
//   keeps(num)         whether a face draws at all, by its plane numerator n . V0;
//   cell(z, face)      what is min-ed into the pixel for a fragment of depth z = (float)Z.
// All of them are compile-time properties: a sink that keeps every face and ignores the id pays for neither.
struct RasterDepthSink {                                        // nsr_raster_depth: every face, the bits of (float)Z
    typedef unsigned Cell;
    static constexpr Cell kEmpty = kRasterEmpty;
    static constexpr bool kFaceId = false;
    NSR_DEV bool keeps(double) const { return true; }
    NSR_DEV Cell cell(float z, unsigned) const { return __builtin_bit_cast(unsigned, z); }
};
constexpr int kRasterResolveLds = raster_resolve_lds<RasterDepthSink>();

template <class Sink>
NSR_DEV const typename Sink::Cell *raster_tile_pass(const RasterParams &P, const Sink &sink) {
    char *lds = lds_base();
    double *sN = reinterpret_cast<double *>(lds + kRzN);
    double *sP = reinterpret_cast<double *>(lds + kRzPlane);
    double *sD = reinterpret_cast<double *>(lds + kRzDir);
    int *sBox = reinterpret_cast<int *>(lds + kRzBox);
    int *sRows = reinterpret_cast<int *>(lds + kRzRows);
    typename Sink::Cell *zb = reinterpret_cast<typename Sink::Cell *>(lds + kRzZ);
    const int t = tid(), k = bid_y(), tile = bid_x();
    const int gx0 = (tile % P.tx) * kRasterTile, gy0 = (tile / P.tx) * kRasterTile;
    for (int e = t; e < kRasterTile * kRasterTile; e += kRasterThreads) zb[e] = Sink::kEmpty;
    if (t < kRasterTile) sD[t] = ((double)(gx0 + t) - P.cx) / P.fx;
    else if (t < 2 * kRasterTile) sD[t] = ((double)(gy0 + t - kRasterTile) - P.cy) / P.fy;
    long long e0 = P.tile_start[(long long)k * P.ntiles + tile], e1 = P.tile_start[(long long)k * P.ntiles + tile + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > P.cap ? P.cap : e1;
    const float *cam = P.cam + 4 * (long long)k * P.nv;
    for (long long b0 = e0; b0 < e1; b0 += kRasterThreads) {
        block_sync();                                             // the previous batch is no longer read
        int nrows = 0;
        const long long f = b0 + t < e1 ? P.bins[b0 + t] : -1;
        const int i0 = f >= 0 && f < P.nf ? P.faces[3 * f] : -1, i1 = f >= 0 && f < P.nf ? P.faces[3 * f + 1] : -1,
                  i2 = f >= 0 && f < P.nf ? P.faces[3 * f + 2] : -1;
        if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < P.nv && i1 < P.nv && i2 < P.nv) {
            const int *r = P.rect + 2 * ((long long)k * P.nf + f);
            int x0 = (r[0] & 0xffff) - gx0, x1 = ((r[0] >> 16) & 0xffff) - gx0, y0 = (r[1] & 0xffff) - gy0, y1 = ((r[1] >> 16) & 0xffff) - gy0;
            x0 = x0 < 0 ? 0 : x0; y0 = y0 < 0 ? 0 : y0;
            x1 = x1 > kRasterTile - 1 ? kRasterTile - 1 : x1; y1 = y1 > kRasterTile - 1 ? kRasterTile - 1 : y1;
            nrows = y1 >= y0 && x1 >= x0 ? y1 - y0 + 1 : 0;
            sBox[t] = y0 | (x0 << 8) | (x1 << 16);
            const int idx[3] = {i0, i1, i2};
            const float *V[3] = {cam + 4ll * idx[0], cam + 4ll * idx[1], cam + 4ll * idx[2]};
            for (int e = 0; e < 3; ++e) {
                const int a = e, c = (e + 1) % 3;
                double N[3];
                const bool canon = idx[a] <= idx[c];
                raster_edge(canon ? V[a] : V[c], canon ? V[c] : V[a], N);
                for (int q = 0; q < 3; ++q) sN[(3 * e + q) * kRasterThreads + t] = canon ? N[q] : -N[q];
            }
            const double v0x = V[0][0], v0y = V[0][1], v0z = V[0][2];
            const double ux = (double)V[1][0] - v0x, uy = (double)V[1][1] - v0y, uz = (double)V[1][2] - v0z;
            const double wx = (double)V[2][0] - v0x, wy = (double)V[2][1] - v0y, wz = (double)V[2][2] - v0z;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            const double num = (nx * v0x + ny * v0y) + nz * v0z;
            sP[t] = nx; sP[kRasterThreads + t] = ny; sP[2 * kRasterThreads + t] = nz;
            sP[3 * kRasterThreads + t] = num;
            if (!sink.keeps(num)) nrows = 0;
        }
        // exclusive scan of the row counts: item r of the batch is row r - rows[j] of triangle j, rows[j] <= r < rows[j + 1]
        int cur = 0;
        sRows[t] = nrows;
        block_sync();
        for (int d = 1; d < kRasterThreads; d <<= 1) {
            const int x = sRows[cur * (kRasterThreads + 1) + t] + (t >= d ? sRows[cur * (kRasterThreads + 1) + t - d] : 0);
            sRows[(1 - cur) * (kRasterThreads + 1) + t] = x;
            cur = 1 - cur;
            block_sync();
        }
        const int *incl = sRows + cur * (kRasterThreads + 1);
        const int total = incl[kRasterThreads - 1];
        for (int item = t; item < total; item += kRasterThreads) {
            int lo = 0, hi = kRasterThreads - 1;                     // first j with incl[j] > item
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (incl[mid] > item) hi = mid; else lo = mid + 1;
            }
            const int j = lo;
            const int bx = sBox[j];
            const int row = (bx & 0xff) + item - (j > 0 ? incl[j - 1] : 0);
            const int x0 = (bx >> 8) & 0xff, x1 = (bx >> 16) & 0xff;
            const double dy = sD[kRasterTile + row];
            double N[9];
            for (int q = 0; q < 9; ++q) N[q] = sN[q * kRasterThreads + j];
            const double nx = sP[j], ny = sP[kRasterThreads + j], nz = sP[2 * kRasterThreads + j], num = sP[3 * kRasterThreads + j];
            const unsigned fid = Sink::kFaceId ? (unsigned)P.bins[b0 + j] : 0u;
            for (int x = x0; x <= x1; ++x) {
                const double dx = sD[x];
                const double a = (dx * N[0] + dy * N[1]) + N[2];
                const double b = (dx * N[3] + dy * N[4]) + N[5];
                const double c = (dx * N[6] + dy * N[7]) + N[8];
                const bool pos = a >= 0.0 && b >= 0.0 && c >= 0.0, neg = a <= 0.0 && b <= 0.0 && c <= 0.0;
                if (!(pos || neg) || (a == 0.0 && b == 0.0 && c == 0.0)) continue;
                const double Z = num / ((nx * dx + ny * dy) + nz);
                if (!(Z >= P.near && Z <= P.far)) continue;
                raster_lds_min(zb + row * kRasterTile + x, sink.cell((float)Z, fid));
            }
        }
    }
    block_sync();
    return zb;
}

NSR_KERNEL void raster_resolve_kernel(const RasterParams P) {
    const unsigned *zb = raster_tile_pass(P, RasterDepthSink());
    const int t = tid(), k = bid_y(), tile = bid_x();
    const int gx0 = (tile % P.tx) * kRasterTile, gy0 = (tile / P.tx) * kRasterTile;
    for (int e = t; e < kRasterTile * kRasterTile; e += kRasterThreads) {
        const int x = gx0 + (e % kRasterTile), y = gy0 + (e / kRasterTile);
        if (x >= P.W || y >= P.H) continue;
        const unsigned z = zb[e];
        P.depth[((long long)k * P.H + y) * P.W + x] = z == kRasterEmpty ? 0.f : __builtin_bit_cast(float, z);
    }
}

// ------------------------------------------------------------------------------------------------
// Depth L1: per view, |a - b| in fp64 over H W pixels, trees of 256 (reduce_kernel's pairing), partials summed in block order
// ------------------------------------------------------------------------------------------------
struct L1Params {
    const float *a, *b;              // [K][n]
    long long n, nblocks;
    int K;
    double *partial;                 // [K][nblocks]
    double *out;                     // [K] per-view means
};

NSR_KERNEL void raster_l1_kernel(const L1Params P) {
    double *red = reinterpret_cast<double *>(lds_base());
    const int t = tid(), k = bid_y();
    const long long i = (long long)bid_x() * kRasterThreads + t;
    red[t] = i < P.n ? fabs((double)P.a[(long long)k * P.n + i] - (double)P.b[(long long)k * P.n + i]) : 0.0;
    block_sync();
    for (int w = kRasterThreads / 2; w >= 1; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        block_sync();
    }
    if (t == 0) P.partial[(long long)k * P.nblocks + bid_x()] = red[0];
}

NSR_KERNEL void raster_l1_final_kernel(const L1Params P) {
    const int k = bid_x() * kRasterThreads + tid();
    if (k >= P.K) return;
    double acc = 0.0;
    for (long long b = 0; b < P.nblocks; ++b) acc += P.partial[(long long)k * P.nblocks + b];
    P.out[k] = acc / (double)P.n;
}

// ------------------------------------------------------------------------------------------------
// View acceptance (check_proj): one thread per point, the candidates through LDS in chunks; a candidate's flag is set (a plain
// store of 1 by one lane of each wave that has a point it sees) iff some point projects into its image.  The caller zeroes it.
// ------------------------------------------------------------------------------------------------
struct ViewParams {
    CullParams C;                    // C.verts: the cloud (fp32 / fp64), C.n, C.fp64, C.w2c [K][12], C.kf, C.W, C.H
    unsigned char *sees;             // [K]
};

NSR_KERNEL void raster_view_clear_kernel(const ViewParams V) {
    const int k = bid_x() * kRasterThreads + tid();
    if (k < V.C.K) V.sees[k] = 0;
}

NSR_KERNEL void raster_view_kernel(const ViewParams V) {
    const CullParams &P = V.C;
    float *pose = reinterpret_cast<float *>(lds_base());           // [kRasterViewChunk][12]
    const long long i = (long long)bid_x() * kRasterThreads + tid();
    const bool live = i < P.n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) {
        double x, y, z;
        nn_load(P.verts, P.fp64, i, x, y, z);
        px = (float)x; py = (float)y; pz = (float)z;
    }
    for (int k0 = 0; k0 < P.K; k0 += kRasterViewChunk) {
        const int nk = P.K - k0 < kRasterViewChunk ? P.K - k0 : kRasterViewChunk;
        block_sync();
        for (int e = tid(); e < 12 * nk; e += kRasterThreads) pose[e] = P.w2c[12ll * k0 + e];
        block_sync();
        for (int k = 0; k < nk; ++k) {
            const bool s = live && cull_sees(P, pose + 12 * k, px, py, pz);
            if (ballot64(s) && (tid() & 63) == 0) V.sees[k0 + k] = 1;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Point visibility against the z-buffers of a batch of views (occlusion-aware culling, unseen-region clouds): one thread owns
// a point, the poses travel through LDS in chunks as in cull_vertex_kernel, the thread loops over the views and finishes with
// one plain read-modify-write of its own counter.  No atomics: counts are bit-identical run to run; successive batches of a
// trajectory are successive launches on one stream.  Contract (tests/occlusion_reference.py restates it in numpy):
//   Camera     the point rounded to fp32, then c_r = ((w_r0 x + w_r1 y) + w_r2 z) + w_r3 in fp32: raster_vertex_kernel's
//              expression, so a mesh's own vertices get the numbers its z-buffer was drawn from.
//   Range      in range iff near <= (double)c_z <= far.
//   Pixel      fp64: u = ((double)c_x / (double)c_z) fx + cx, v = ((double)c_y / (double)c_z) fy + cy; i = floor(u + 0.5),
//              j = floor(v + 0.5); inside iff 0 <= i < W and 0 <= j < H (a NaN is outside).
//   Occlusion  d = depth[k][j][i]; visible iff d == 0 (nothing drawn there) or (double)c_z <= (double)d + eps.
//   Count      count[p] += the number of the K views in which p is in range, inside and visible.
// ------------------------------------------------------------------------------------------------
struct VisParams {
    const void *pts;                 // [n][3] fp32 or fp64
    long long n;
    int fp64, K, H, W;
    const float *w2c;                // [K][12]
    const float *depth;              // [K][H][W]
    double fx, fy, cx, cy, near, far, eps;
    int *count;                      // [n], accumulated
};

NSR_KERNEL void points_visible_kernel(const VisParams P) {
    float *pose = reinterpret_cast<float *>(lds_base());           // [kRasterViewChunk][12]
    const long long i = (long long)bid_x() * kRasterThreads + tid();
    const bool live = i < P.n;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (live) {
        double x, y, z;
        nn_load(P.pts, P.fp64, i, x, y, z);
        px = (float)x; py = (float)y; pz = (float)z;
    }
    int c = 0;
    for (int k0 = 0; k0 < P.K; k0 += kRasterViewChunk) {
        const int nk = P.K - k0 < kRasterViewChunk ? P.K - k0 : kRasterViewChunk;
        block_sync();                                               // the previous chunk is no longer read
        for (int e = tid(); e < 12 * nk; e += kRasterThreads) pose[e] = P.w2c[12ll * k0 + e];
        block_sync();
        if (!live) continue;
        for (int k = 0; k < nk; ++k) {
            const float *w = pose + 12 * k;
            const float cz = ((w[8] * px + w[9] * py) + w[10] * pz) + w[11];
            const double z = (double)cz;
            if (!(z >= P.near && z <= P.far)) continue;
            const float xc = ((w[0] * px + w[1] * py) + w[2] * pz) + w[3];
            const float yc = ((w[4] * px + w[5] * py) + w[6] * pz) + w[7];
            const double u = floor((((double)xc / z) * P.fx + P.cx) + 0.5), v = floor((((double)yc / z) * P.fy + P.cy) + 0.5);
            if (!(u >= 0.0 && u < (double)P.W && v >= 0.0 && v < (double)P.H)) continue;
            const float d = P.depth[((long long)(k0 + k) * P.H + (long long)v) * P.W + (long long)u];
            if (d == 0.f || z <= (double)d + P.eps) ++c;
        }
    }
    if (live) P.count[i] = P.count[i] + c;
}

}  // namespace nsr
