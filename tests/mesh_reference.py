"""TEST INFRASTRUCTURE: numpy restatements of the mesh-extraction kernels (nice_slam_amd/csrc/nsr_kernels.h, "mesh
extraction" section), written from the contract in include/nsr.h and from the reference's Mesher (src/utils/Mesher.py),
never from the kernel sources.  Citations are to the reference tree.

    mc_table()          the 256-case triangulation, built from a per-face rule (crack-free by construction)
    marching_cubes()    welded marching cubes over a [nx][ny][nz] fp32 lattice
    point_masks()       Mesher.point_masks (:53-212), the three branches, per-chunk max_depth
    grid_uniform()      Mesher.get_grid_uniform (:322-347)
"""
import numpy as np

# --------------------------------------------------------------------------------------------------------------------
# marching cubes
#   corner c of a cell sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) along (x, y, z); bit c of the case is set iff
#   that corner is "above" (f > level).  Edge e = 4 * axis + (o1 + 2 * o2): the cell edge along `axis` whose offsets along
#   the two other axes (in increasing axis order) are o1, o2.
# --------------------------------------------------------------------------------------------------------------------


def _others(a):
    return [b for b in range(3) if b != a]


def edge_origin(e):
    """(offset of the edge's lower end inside the cell, axis)"""
    a = e // 4
    b1, b2 = _others(a)
    off = [0, 0, 0]
    off[b1] = e & 1
    off[b2] = (e >> 1) & 1
    return tuple(off), a


def mc_table():
    """Per case: list of triangles (edge triples).  On each of the cube's six faces, walked counter-clockwise as seen from
    outside the cube, every run of above corners is cut off by one segment from the edge where the run ends to the edge where
    it starts.  The segments depend only on the face's four signs (an ambiguous face always separates its two above corners),
    so two cells sharing a face cut it the same way: no cracks.  Each straddling cube edge ends one segment and starts another,
    so the segments close into loops (in order of their smallest edge), each triangulated by _triangulate."""
    def corner(o):
        return o[0] + 2 * o[1] + 4 * o[2]

    tables = []
    for case in range(256):
        above = [(case >> c) & 1 for c in range(8)]
        nxt = {}
        for a in range(3):
            b1, b2 = _others(a)
            right_handed = -1 if a == 1 else 1          # (e_b1, e_b2, e_a) is a right-handed frame for a = 0, 2
            for s in (0, 1):
                uv = [(0, 0), (1, 0), (1, 1), (0, 1)]
                if right_handed * (1 if s else -1) < 0:
                    uv = uv[::-1]
                cs = []
                for u, v in uv:
                    o = [0, 0, 0]
                    o[a], o[b1], o[b2] = s, u, v
                    cs.append(o)

                def face_edge(i):
                    p, q = cs[i], cs[(i + 1) % 4]
                    ax = [k for k in range(3) if p[k] != q[k]][0]
                    lo = [min(p[k], q[k]) for k in range(3)]
                    c1, c2 = _others(ax)
                    return 4 * ax + lo[c1] + 2 * lo[c2]

                entries = [i for i in range(4) if not above[corner(cs[i])] and above[corner(cs[(i + 1) % 4])]]
                exits = [i for i in range(4) if above[corner(cs[i])] and not above[corner(cs[(i + 1) % 4])]]
                for i in exits:
                    j = max([k for k in entries if k < i], default=max(entries))
                    nxt[face_edge(i)] = face_edge(j)
        loops, seen = [], set()
        for e0 in sorted(nxt):
            if e0 in seen:
                continue
            loop, e = [], e0
            while e not in seen:
                seen.add(e)
                loop.append(e)
                e = nxt[e]
            loops.append(loop)
        tris = []
        for lp in loops:
            tris += [(lp[a], lp[c], lp[b]) for a, b, c in _triangulate(lp)]
        tables.append(tris)
    return tables


def _edge_faces(e):
    off, a = edge_origin(e)
    return {(b, off[b]) for b in _others(a)}


def _triangulate(loop):
    """Triangles (i, j, k) of positions in the loop, i < j < k, first found in a fixed search order such that no inner
    diagonal joins two vertices on a common cube face: such a diagonal would lie in the face, where the neighbouring cell
    may draw the same segment, and the mesh edge would then be used by four faces.  Emitted as (i, k, j): the polygon is
    walked with the above corners on its left, and the face normal points toward decreasing field."""
    n = len(loop)

    def ok(i, j):
        return (j - i) % n in (1, n - 1) or not (_edge_faces(loop[i]) & _edge_faces(loop[j]))

    def rec(idx):
        if len(idx) < 3:
            return []
        a, b = idx[0], idx[-1]
        for k in range(1, len(idx) - 1):
            c = idx[k]
            if not (ok(a, c) and ok(c, b)):
                continue
            left, right = rec(idx[:k + 1]), rec(idx[k:])
            if left is not None and right is not None:
                return left + [(a, c, b)] + right
        return None

    tris = rec(list(range(n)))
    assert tris is not None, loop
    return tris


def marching_cubes(vol, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """-> (verts float64 [V,3], faces int32 [F,3]); vertex i = the i-th straddling lattice edge in edge-id order
    3 * (linear index of the lower end) + axis; faces by cell linear index, then table order."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    lvl = np.float32(level)
    above = vol > lvl
    n = vol.size
    flags = np.zeros((nx, ny, nz, 3), dtype=bool)
    flags[:-1, :, :, 0] = above[:-1] != above[1:]
    flags[:, :-1, :, 1] = above[:, :-1] != above[:, 1:]
    flags[:, :, :-1, 2] = above[:, :, :-1] != above[:, :, 1:]
    ff = flags.reshape(-1)
    vid = (np.cumsum(ff, dtype=np.int64) - 1).astype(np.int64)
    eid = np.nonzero(ff)[0]
    lin, ax = eid // 3, eid % 3
    ix, iy, iz = lin // (ny * nz), (lin // nz) % ny, lin % nz
    idx = np.stack([ix, iy, iz], 1)
    step = np.array([ny * nz, nz, 1])
    fa = vol.reshape(-1)[lin]
    fb = vol.reshape(-1)[lin + step[ax]]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (lvl - fa) / (fb - fa)
    sp = np.asarray(spacing, dtype=np.float64)
    org = np.asarray(origin, dtype=np.float64)
    pos = idx.astype(np.float64)
    pos[np.arange(len(eid)), ax] += t.astype(np.float64)
    verts = org[None, :] + pos * sp[None, :]

    tab = mc_table()
    if nx < 2 or ny < 2 or nz < 2:
        return verts, np.zeros((0, 3), np.int32)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= above[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntri = np.array([len(x) for x in tab])
    T = np.full((256, 5, 3), -1, dtype=np.int64)
    for k, tl in enumerate(tab):
        for j, tri in enumerate(tl):
            T[k, j] = tri
    cx, cy, cz = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    clin = ((cx * ny + cy) * nz + cz).reshape(-1)
    case = case.reshape(-1)
    live = ntri[case] > 0
    clin, case = clin[live], case[live]
    rep = ntri[case]
    cell_of = np.repeat(np.arange(len(clin)), rep)
    slot = np.arange(len(cell_of)) - np.repeat(np.cumsum(rep) - rep, rep)
    tri_e = T[case[cell_of], slot]                       # [F,3] cell edges
    eoff = np.array([edge_origin(e)[0] for e in range(12)])
    eax = np.array([edge_origin(e)[1] for e in range(12)])
    plin = clin[cell_of][:, None] + (eoff[tri_e] * step[None, None, :]).sum(-1)
    faces = vid[3 * plin + eax[tri_e]]
    return verts, faces.astype(np.int32)


# --------------------------------------------------------------------------------------------------------------------
# Mesher.point_masks (:53-212) and get_grid_uniform (:322-347)
# --------------------------------------------------------------------------------------------------------------------


def grid_uniform(bound, resolution, padding=0.05):
    """(points fp32 [R^3,3] in np.meshgrid order, [x, y, z] fp64 axes)"""
    b = np.asarray(bound, dtype=np.float64)
    xs = [np.linspace(b[i][0] - padding, b[i][1] + padding, resolution) for i in range(3)]
    xx, yy, zz = np.meshgrid(*xs)
    return np.vstack([xx.ravel(), yy.ravel(), zz.ravel()]).T.astype(np.float32), xs


def _grid_sample_zeros_ac(depth, gx, gy):
    """F.grid_sample(bilinear, zeros, align_corners=True) of one [H,W] image at normalised fp32 coordinates"""
    H, W = depth.shape
    f32 = np.float32
    x = ((gx + f32(1)) / f32(2)) * f32(W - 1)
    y = ((gy + f32(1)) / f32(2)) * f32(H - 1)
    xw, yn = np.floor(x), np.floor(y)
    w = x - xw
    e = f32(1) - w
    nn = y - yn
    s = f32(1) - nn
    out = np.zeros_like(x)
    for cy, cx, wt in ((yn, xw, s * e), (yn, xw + 1, s * w), (yn + 1, xw, nn * e), (yn + 1, xw + 1, nn * w)):
        with np.errstate(invalid="ignore"):
            ok = (cx > -1) & (cx < W) & (cy > -1) & (cy < H)
        xi = np.where(ok, cx, 0).astype(np.int64)
        yi = np.where(ok, cy, 0).astype(np.int64)
        out = out + np.where(ok, depth[yi, xi], f32(0)) * wt
    return out.astype(np.float32)


def point_masks(points, c2ws, depths, H, W, fx, fy, cx, cy, mode, chunk):
    """mode 0: get_mask_use_all_frames (:88-125); 1: keyframes, depth_test=False (:178-191); 2: keyframes, depth_test=True
    (:156-177).  -> uint8 [N]: 0 unseen, 1 seen, 2 forecast."""
    f32 = np.float32
    pts = np.asarray(points, dtype=np.float32)
    N = pts.shape[0]
    out = np.zeros(N, np.uint8)
    Kf = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64).astype(np.float32)
    for c0 in range(0, N, chunk):
        p = pts[c0:c0 + chunk]
        seen = np.zeros(len(p), bool)
        fore = np.zeros(len(p), bool)
        for k in range(len(c2ws)):
            w2c = np.linalg.inv(np.asarray(c2ws[k])).astype(np.float32)      # in the pose's own dtype, as :130-132
            cam = [((w2c[r, 0] * p[:, 0] + w2c[r, 1] * p[:, 1]) + w2c[r, 2] * p[:, 2]) + w2c[r, 3] for r in range(3)]
            cam[0] = cam[0] * f32(-1)
            uvz = [((Kf[r, 0] * cam[0] + Kf[r, 1] * cam[1]) + Kf[r, 2] * cam[2]) for r in range(3)]
            z = uvz[2] + f32(1e-8)
            with np.errstate(divide="ignore", invalid="ignore"):
                u, v = uvz[0] / z, uvz[1] / z
            s_in = (u < f32(W)) & (u > f32(0)) & (v < f32(H)) & (v > f32(0)) & (z < 0)
            f_in = (u < f32(W + 1000)) & (u > f32(-1000)) & (v < f32(H + 1000)) & (v > f32(-1000)) & (z < 0)
            pd = -cam[2]
            if mode == 2:
                d = np.asarray(depths[k], dtype=np.float32)
                gx = (u / f32(W - 1)) * f32(2.0) - f32(1.0)
                gy = (v / f32(H - 1)) * f32(2.0) - f32(1.0)
                ds = _grid_sample_zeros_ac(d, gx, gy)
                mx = ds.max()
                f_in &= pd < mx
                s_in &= (pd < ds + f32(2.4)) & (ds - f32(2.4) < pd)
            elif mode == 1:
                mx = np.asarray(depths[k], dtype=np.float32).max() * f32(1.1)
                f_in &= pd < mx
                s_in &= pd < mx
            seen |= s_in
            fore |= f_in
        fore &= ~seen
        out[c0:c0 + chunk] = np.where(seen, 1, np.where(fore, 2, 0))
    return out


# --------------------------------------------------------------------------------------------------------------------
# mesh properties used by the tests
# --------------------------------------------------------------------------------------------------------------------


def edge_use_counts(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e = np.sort(e, axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return cnt


def euler_characteristic(verts, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    n_e = len(np.unique(e, axis=0))
    n_v = len(np.unique(faces))
    return n_v - n_e + len(faces)


def signed_volume(verts, faces):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float(np.einsum("ij,ij->i", v0, np.cross(v1, v2)).sum() / 6.0)


def face_adjacency_components(faces):
    """connected components of faces that share an edge (scipy.sparse.csgraph on the face graph)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    F = len(faces)
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    fid = np.tile(np.arange(F), 3)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e, fid = e[order], fid[order]
    same = np.all(e[1:] == e[:-1], axis=1)
    a, b = fid[:-1][same], fid[1:][same]
    g = coo_matrix((np.ones(len(a)), (a, b)), shape=(F, F))
    return connected_components(g, directed=False)[1]


def face_areas(verts, faces):
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(v1 - v0, v2 - v0), axis=1)
