"""TEST INFRASTRUCTURE: a numpy restatement of the depth-rasterization contract written out in
nice_slam_amd/csrc/nsr_raster.h, in the kernels' operation order (vertex pass in fp32, edge values and depth in fp64, near /
far, z-min, the per-view depth L1 and the check_proj view test), closed tessellated boxes, and an fp64 ray cast of them."""
import warnings

import numpy as np

F32 = np.float32


# ---- meshes -------------------------------------------------------------------------------------------------------------
def box_mesh(lo, hi, n):
    """(vertices fp64 [V, 3], faces int32 [F, 3]) of the closed surface of the box lo..hi, every face an n[a] x n[b] grid of
    quads split into two triangles; vertices on shared box edges are shared (one lattice)"""
    lo, hi, n = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(n, np.int64)
    keys, faces = {}, []
    verts = []

    def vid(ijk):
        k = tuple(int(x) for x in ijk)
        if k not in keys:
            keys[k] = len(verts)
            verts.append(lo + (hi - lo) * np.array(k, np.float64) / n)
        return keys[k]

    for d in range(3):
        a, b = (d + 1) % 3, (d + 2) % 3
        for side in (0, n[d]):
            for i in range(n[a]):
                for j in range(n[b]):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        ijk = [0, 0, 0]
                        ijk[d], ijk[a], ijk[b] = side, i + di, j + dj
                        q.append(vid(ijk))
                    faces.append((q[0], q[1], q[2]))
                    faces.append((q[0], q[2], q[3]))
    return np.array(verts), np.array(faces, np.int32)


def ray_cast_box_inside(c2w, lo, hi, H, W, fx, fy, cx, cy):
    """fp64 camera-space depth of the box's inner surface from a camera inside it (OpenCV c2w)"""
    j, i = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.stack([np.where(d[..., a] > 0, (hi[a] - o[a]) / d[..., a], np.where(d[..., a] < 0, (lo[a] - o[a]) / d[..., a], np.inf))
                      for a in range(3)], -1)
    return t.min(-1)                                  # t along d, whose camera z is 1: the depth


# ---- the contract -------------------------------------------------------------------------------------------------------
def w2c_rows(c2w):
    """[K, 12] fp32 rows 0..2 of inv(c2w) in fp64"""
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4, 4)
    return np.linalg.inv(c2w)[:, :3].reshape(len(c2w), 12).astype(F32)


def vertex_pass(verts, w):
    """camera-space vertices [V, 3] fp32: ((w0 x + w1 y) + w2 z) + w3 per row"""
    v = np.asarray(verts).astype(F32)
    w = np.asarray(w, F32).reshape(3, 4)
    return np.stack([((w[r, 0] * v[:, 0] + w[r, 1] * v[:, 1]) + w[r, 2] * v[:, 2]) + w[r, 3] for r in range(3)], 1).astype(F32)


def _boxes(cam, faces, near, H, W, fx, fy, cx, cy):
    """a generous pixel box per face (fp64 clip at 0.99 near, one pixel of margin), or x0 > x1"""
    V = cam.astype(np.float64)[faces]                # [F, 3, 3]
    zc = 0.99 * near
    us, vs = [], []
    for e in range(3):
        a, b = V[:, e], V[:, (e + 1) % 3]
        ina, inb = a[:, 2] >= zc, b[:, 2] >= zc
        with np.errstate(divide="ignore", invalid="ignore"):
            us.append(np.where(ina, fx * a[:, 0] / a[:, 2] + cx, np.nan))
            vs.append(np.where(ina, fy * a[:, 1] / a[:, 2] + cy, np.nan))
            t = (zc - a[:, 2]) / (b[:, 2] - a[:, 2])
            cr = ina != inb
            px, py = a[:, 0] + t * (b[:, 0] - a[:, 0]), a[:, 1] + t * (b[:, 1] - a[:, 1])
            us.append(np.where(cr, fx * px / zc + cx, np.nan))
            vs.append(np.where(cr, fy * py / zc + cy, np.nan))
    U, Vv = np.stack(us, 1), np.stack(vs, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)            # all-NaN rows: faces wholly behind the clip plane
        u0, u1, v0, v1 = np.nanmin(U, 1), np.nanmax(U, 1), np.nanmin(Vv, 1), np.nanmax(Vv, 1)
    empty = np.isnan(u0)
    u0, u1, v0, v1 = (np.nan_to_num(x, nan=0.0, posinf=1e9, neginf=-1e9) for x in (u0, u1, v0, v1))
    x0 = np.clip(np.floor(np.clip(u0, -1e7, 1e7)) - 1, 0, W - 1).astype(np.int64)
    x1 = np.clip(np.ceil(np.clip(u1, -1e7, 1e7)) + 1, -1, W - 1).astype(np.int64)
    y0 = np.clip(np.floor(np.clip(v0, -1e7, 1e7)) - 1, 0, H - 1).astype(np.int64)
    y1 = np.clip(np.ceil(np.clip(v1, -1e7, 1e7)) + 1, -1, H - 1).astype(np.int64)
    x1 = np.where(empty | (u1 < -3) | (u0 > W + 2), -1, x1)
    y1 = np.where(empty | (v1 < -3) | (v0 > H + 2), -1, y1)
    return x0, x1, y0, y1


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def render(verts, faces, w2c12, H, W, fx, fy, cx, cy, near, far, chunk=4_000_000):
    """[H, W] fp32 depth of one view (0: no fragment), the contract of nsr_raster.h"""
    faces = np.asarray(faces, np.int64)
    cam = vertex_pass(verts, w2c12)
    Vd = cam.astype(np.float64)
    dxs = (np.arange(W, dtype=np.float64) - cx) / fx
    dys = (np.arange(H, dtype=np.float64) - cy) / fy
    # per face: sign-corrected edge normals in canonical orientation, the plane
    N = []
    for e in range(3):
        ia, ib = faces[:, e], faces[:, (e + 1) % 3]
        canon = ia <= ib
        lo_i, hi_i = np.where(canon, ia, ib), np.where(canon, ib, ia)
        n = _cross(Vd[lo_i], Vd[hi_i])
        N.append(np.where(canon[:, None], n, -n))
    N = np.stack(N, 1)                                 # [F, 3, 3]
    V0, V1, V2 = Vd[faces[:, 0]], Vd[faces[:, 1]], Vd[faces[:, 2]]
    n = _cross(V1 - V0, V2 - V0)
    num = (n[:, 0] * V0[:, 0] + n[:, 1] * V0[:, 1]) + n[:, 2] * V0[:, 2]
    x0, x1, y0, y1 = _boxes(cam, faces, near, H, W, fx, fy, cx, cy)
    w = np.maximum(x1 - x0 + 1, 0)
    h = np.maximum(y1 - y0 + 1, 0)
    cnt = w * h
    zb = np.full(H * W, np.inf, F32)
    f_all = np.nonzero(cnt)[0]
    start = 0
    while start < len(f_all):
        csum = np.cumsum(cnt[f_all[start:]])
        stop = start + max(1, int(np.searchsorted(csum, chunk, side="right")))
        fs = f_all[start:stop]
        start = stop
        c = cnt[fs]
        fi = np.repeat(fs, c)
        off = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        px = x0[fi] + off % w[fi]
        py = y0[fi] + off // w[fi]
        dx, dy = dxs[px], dys[py]
        e = [(dx * N[fi, k, 0] + dy * N[fi, k, 1]) + N[fi, k, 2] for k in range(3)]
        pos = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
        neg = (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)
        zero = (e[0] == 0) & (e[1] == 0) & (e[2] == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            Z = num[fi] / ((n[fi, 0] * dx + n[fi, 1] * dy) + n[fi, 2])
        keep = (pos | neg) & ~zero & (Z >= near) & (Z <= far)
        np.minimum.at(zb, (py * W + px)[keep], Z[keep].astype(F32))
    return np.where(np.isinf(zb), F32(0), zb).reshape(H, W)


def render_views(verts, faces, c2w, H, W, fx, fy, cx, cy, near, far):
    w = w2c_rows(c2w)
    return np.stack([render(verts, faces, w[k], H, W, fx, fy, cx, cy, near, far) for k in range(len(w))])


def bin_entries(verts, faces, w2c12, H, W, fx, fy, cx, cy, near, tile=32):
    """the (face, tile) pairs of one view by this file's pixel boxes: the size of the view's bins up to the boxes' margins"""
    x0, x1, y0, y1 = _boxes(vertex_pass(verts, w2c12), np.asarray(faces, np.int64), near, H, W, fx, fy, cx, cy)
    live = (x1 >= x0) & (y1 >= y0)
    return int(((x1 // tile - x0 // tile + 1) * (y1 // tile - y0 // tile + 1))[live].sum())


def depth_l1(a, b):
    """[K] fp64 per-view means: |a - b| in fp64, trees of 256 (pairs t, t + w), block partials summed in order"""
    a = np.asarray(a, F32).reshape(len(a), -1).astype(np.float64)
    b = np.asarray(b, F32).reshape(len(b), -1).astype(np.float64)
    K, n = a.shape
    nb = (n + 255) // 256
    v = np.zeros((K, nb * 256))
    v[:, :n] = np.abs(a - b)
    v = v.reshape(K, nb, 256)
    w = 128
    while w >= 1:
        v[:, :, :w] = v[:, :, :w] + v[:, :, w:2 * w]
        w //= 2
    out = np.zeros(K)
    for k in range(K):
        acc = 0.0
        for p in v[k, :, 0]:
            acc += p
        out[k] = acc / n
    return out


def check_proj_sees(points, c2w, H, W, fx, fy, cx, cy):
    """check_proj restated in fp32 (cull_sees' order): True iff some point projects into the candidate's image"""
    c = np.asarray(c2w, np.float64).copy()
    c[:3, 1] *= -1.0
    c[:3, 2] *= -1.0
    w = np.linalg.inv(c)[:3].astype(F32)
    p = np.asarray(points).astype(F32)
    cam = [((w[r, 0] * p[:, 0] + w[r, 1] * p[:, 1]) + w[r, 2] * p[:, 2]) + w[r, 3] * F32(1) for r in range(3)]
    X, Y, Z = cam[0] * F32(-1), cam[1], cam[2]
    kf = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float64).astype(F32)
    uh = (kf[0] * X + kf[1] * Y) + kf[2] * Z
    vh = (kf[3] * X + kf[4] * Y) + kf[5] * Z
    z = ((kf[6] * X + kf[7] * Y) + kf[8] * Z) + F32(1e-5)
    u, v = uh / z, vh / z
    return bool(np.any((F32(0) <= -z) & (u < F32(W)) & (u > 0) & (v < F32(H)) & (v > 0)))


def look_from(eye, target, up=(0.0, 0.0, 1.0)):
    """OpenCV c2w (x right, y down, z forward) at eye looking at target"""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    M = np.eye(4)
    M[:3, 0], M[:3, 1], M[:3, 2], M[:3, 3] = x, y, z, eye
    return M
