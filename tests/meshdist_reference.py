"""TEST INFRASTRUCTURE: references for the point-to-mesh distance (nice_slam_amd/csrc/nsr_meshdist.h).

(a) ``pair_eval`` / ``brute``: the kernel's per-face expression restated in vectorised numpy, operation by operation in the
    documented order, and the brute force over ALL faces built on it (the first face of the smallest squared distance);
(b) ``independent``: another formulation altogether -- project the point onto the face's plane, test inside-ness with the three
    signed areas, else (or for a degenerate face) the nearest of the three edges as segments;
and the small meshes the CPU and the GPU tests share."""
import numpy as np

EPS = 2.0 ** -52


def gate(coord_scale, dist):
    """the bound between the product and (b): 16 ulp of the larger of the coordinate scale and the distance"""
    return 16.0 * EPS * np.maximum(coord_scale, dist)


class _Numpy:
    where = staticmethod(np.where)

    @staticmethod
    def full_like(a, v):
        return np.full(a.shape, v)


class _Torch:
    """the same elementwise fp64 operations on torch CPU tensors (IEEE, one operation per call, never fused): the brute force
    over tens of thousands of faces runs on all cores instead of one"""
    @staticmethod
    def where(c, a, b):
        import torch
        return torch.where(c, a, b)

    @staticmethod
    def full_like(a, v):
        import torch
        return torch.full_like(a, v)


def _dot3(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _sub3(u, v):
    return (u[0] - v[0], u[1] - v[1], u[2] - v[2])


def _segment3(xp, p, s, e):
    d = _sub3(e, s)
    l = _dot3(d, d)
    t = _dot3(_sub3(p, s), d) / l
    first = (l == 0.0) | ~(t > 0.0)
    last = ~first & (t >= 1.0)
    x = tuple(xp.where(first, s[k] + 0.0 * l, xp.where(last, e[k] + 0.0 * l, s[k] + d[k] * t)) for k in range(3))
    r = _sub3(p, x)
    return _dot3(r, r), x


def _pair3(xp, p, a, b, c):
    """the kernel's md_face on component tuples (x, y, z) of arrays that broadcast against each other"""
    ab, ac = _sub3(b, a), _sub3(c, a)
    n = (ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0])
    ap, bp, cp = _sub3(p, a), _sub3(p, b), _sub3(p, c)
    d1, d2, d3, d4, d5, d6 = _dot3(ab, ap), _dot3(ac, ap), _dot3(ab, bp), _dot3(ac, bp), _dot3(ab, cp), _dot3(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    degen = ((n[0] == 0.0) & (n[1] == 0.0) & (n[2] == 0.0)) | (d1 != d1)          # (broadcast to the pair shape)
    r1 = (d1 <= 0.0) & (d2 <= 0.0)
    r2 = (d3 >= 0.0) & (d4 <= d3)
    r3 = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0)
    den3 = d1 - d3
    t3 = d1 / den3
    r4 = (d6 >= 0.0) & (d5 <= d6)
    r5 = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0)
    den5 = d2 - d6
    t5 = d2 / den5
    r6 = (va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0)
    den6 = (d4 - d3) + (d5 - d6)
    t6 = (d4 - d3) / den6
    den7 = (va + vb) + vc
    v7, w7 = vb / den7, vc / den7
    full = lambda v: xp.full_like(d1, float(v))
    region = xp.where(r1, full(1), xp.where(r2, full(2), xp.where(r3, full(3), xp.where(r4, full(4), xp.where(r5, full(5), xp.where(r6, full(6), full(7)))))))
    den = xp.where(region == 3, den3, xp.where(region == 5, den5, xp.where(region == 6, den6, xp.where(region == 7, den7, full(1)))))
    degen = degen | ~((den > 0.0) | (den < 0.0)) | ((region == 7) & ~((va > 0.0) & (vb > 0.0) & (vc > 0.0)))
    zero = 0.0 * d1 * 0.0
    zero = xp.where(zero == zero, zero, full(0))                   # a broadcast zero, whatever d1 holds
    x = tuple(xp.where(r1, a[k] + zero, xp.where(r2, b[k] + zero, xp.where(r3, a[k] + ab[k] * t3, xp.where(r4, c[k] + zero, xp.where(
        r5, a[k] + ac[k] * t5, xp.where(r6, b[k] + (c[k] - b[k]) * t6, (a[k] + ab[k] * v7) + ac[k] * w7)))))) for k in range(3))
    r = _sub3(p, x)
    dd = _dot3(r, r)
    sd, sx = _segment3(xp, p, a, b)
    for s, e in ((b, c), (c, a)):
        d, xx = _segment3(xp, p, s, e)
        closer = d < sd
        sd = xp.where(closer, d, sd)
        sx = tuple(xp.where(closer, xx[k], sx[k]) for k in range(3))
    return xp.where(degen, sd, dd), tuple(xp.where(degen, sx[k], x[k]) for k in range(3)), xp.where(degen, full(0), region)


def pair_eval(p, a, b, c):
    """(squared distance, closest point, region 1..7 of the walk or 0 for the degenerate route) of p [..., 3] to the triangles
    (a, b, c) [..., 3], broadcast against each other"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    comp = lambda u: (u[..., 0], u[..., 1], u[..., 2])
    with np.errstate(all="ignore"):
        d2, x, region = _pair3(_Numpy, comp(p), comp(a), comp(b), comp(c))
    return d2, np.stack(x, -1), region.astype(np.int64)


def brute(points, verts, faces, chunk=64, return_d2=False):
    """(dist [N], face [N] = argmin: the smallest index of the minimum, closest [N, 3][, d2 [N, F]]) over ALL faces, on torch's
    CPU tensors (tests/test_meshdist_emu.py holds them to the numpy path)"""
    import torch
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3)))
    tri = torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]))
    N = len(p)
    dist, face, closest = np.empty(N), np.empty(N, np.int64), np.empty((N, 3))
    full = np.empty((N, len(tri))) if return_d2 else None
    corner = lambda j: tuple(tri[None, :, j, k] for k in range(3))
    for s in range(0, N, chunk):
        q = tuple(p[s:s + chunk, None, k] for k in range(3))
        d2, x, _ = _pair3(_Torch, q, corner(0), corner(1), corner(2))
        i = (d2 == d2.min(1, keepdim=True)[0]).to(torch.uint8).argmax(1)          # the FIRST face of the minimum
        k = torch.arange(len(i))
        dist[s:s + chunk], face[s:s + chunk] = np.sqrt(d2[k, i].numpy()), i.numpy()      # (numpy's square root: correctly rounded)
        closest[s:s + chunk] = torch.stack([x[0][k, i], x[1][k, i], x[2][k, i]], 1).numpy()
        if return_d2:
            full[s:s + chunk] = d2.numpy()
    return (dist, face, closest, full) if return_d2 else (dist, face, closest)


def at_face(points, verts, faces, face):
    """(dist, closest) of (a) evaluated at one given face per point"""
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    d2, x, _ = pair_eval(np.asarray(points, np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    return np.sqrt(d2), x


def independent(p, a, b, c):
    """distance of p to the triangles by formulation (b)"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    with np.errstate(all="ignore"):
        h = ((p - a) * n).sum(-1) / nn
        q = p - n * h[..., None]
        s0 = (np.cross(b - a, q - a) * n).sum(-1)
        s1 = (np.cross(c - b, q - b) * n).sum(-1)
        s2 = (np.cross(a - c, q - c) * n).sum(-1)
        inside = (nn > 0.0) & (s0 >= 0.0) & (s1 >= 0.0) & (s2 >= 0.0)
        d_plane = np.abs(((p - a) * n).sum(-1)) / np.sqrt(nn)
    d_seg = np.full(p.shape[:-1], np.inf)
    for s, e in ((a, b), (b, c), (c, a)):
        d = e - s
        ll = (d * d).sum(-1)
        with np.errstate(all="ignore"):
            t = np.where(ll > 0.0, ((p - s) * d).sum(-1) / ll, 0.0)
        t = np.clip(np.nan_to_num(t), 0.0, 1.0)
        r = p - (s + d * t[..., None])
        d_seg = np.minimum(d_seg, np.sqrt((r * r).sum(-1)))
    return np.where(inside, d_plane, d_seg)


def independent_mesh(points, verts, faces, chunk=64):
    """distance [N] to the mesh by (b): the minimum over all faces"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    out = np.empty(len(p))
    for s in range(0, len(p), chunk):
        out[s:s + chunk] = independent(p[s:s + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).min(1)
    return out


# ---- meshes ---------------------------------------------------------------------------------------------------------
def rectangle(lo, hi, z=0.0, nx=1, ny=1):
    """the rectangle [lo, hi] (2-vectors) at height z as an nx x ny grid of quads, two triangles each, normals +z"""
    xs, ys = np.linspace(lo[0], hi[0], nx + 1), np.linspace(lo[1], hi[1], ny + 1)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, float(z))], 1)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    k = (i * (ny + 1) + j).ravel()
    f = np.concatenate([np.stack([k, k + ny + 1, k + ny + 2], 1), np.stack([k, k + ny + 2, k + 1], 1)])
    return v, f.astype(np.int32)


def box(lo, hi, n=1):
    """the closed box [lo, hi] with every side an n x n grid of quads"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    vs, fs, off = [], [], 0
    for d in range(3):
        e1, e2 = (d + 1) % 3, (d + 2) % 3
        for side in (lo[d], hi[d]):
            v2, f = rectangle((lo[e1], lo[e2]), (hi[e1], hi[e2]), side, n, n)
            v = np.empty_like(v2)
            v[:, e1], v[:, e2], v[:, d] = v2[:, 0], v2[:, 1], v2[:, 2]
            vs.append(v)
            fs.append(f + off)
            off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def oversize_scene(seed=0, small=1500):
    """two room-sized triangles among `small` millimetre-sized ones scattered through a 5 x 4 x 3 m room"""
    rng = np.random.default_rng(seed)
    c = rng.uniform([0.2, 0.2, 0.2], [4.8, 3.8, 2.8], (small, 3))
    v = (c[:, None, :] + rng.uniform(-1e-3, 1e-3, (small, 3, 3))).reshape(-1, 3)
    big = np.array([[0, 0, 0], [5, 0, 0], [0, 4, 3], [5, 4, 0], [0, 4, 0.5], [5, 0, 3]], np.float64)
    v = np.concatenate([v, big])
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    return v, f


def rotation_x(theta):
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
