"""TEST INFRASTRUCTURE: a numpy restatement of the point-visibility contract written out in nice_slam_amd/csrc/nsr_raster.h
(points_visible_kernel) and of the scaled-image rule of nice_slam_amd/raster.py (visibility_counts), on top of
raster_reference.render_views: the same scaled intrinsics and the same operation order, and the room-and-pillar scene the
occlusion tests share."""
import numpy as np

import raster_reference as R

F32 = np.float32
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([5.0, 4.0, 3.0])
PILLAR_LO, PILLAR_HI = np.array([2.2, 1.7, 0.0]), np.array([2.8, 2.3, 3.0])


def room_and_pillar(n_room=(10, 8, 6), n_pillar=(3, 3, 8)):
    """(vertices fp64, faces int32, number of room vertices): the closed room and a box pillar from floor to ceiling in it"""
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, n_room)
    pv, pf = R.box_mesh(PILLAR_LO, PILLAR_HI, n_pillar)
    return np.concatenate([v, pv]), np.concatenate([f, pf + len(v)]).astype(np.int32), len(v)


def raster_divisor(H, W, limit=1024):
    m = 1
    while -(-H // m) > limit or -(-W // m) > limit:
        m += 1
    return m


def scaled_camera(H, W, fx, fy, cx, cy, m):
    return -(-H // m), -(-W // m), float(fx) / m, float(fy) / m, (float(cx) + 0.5) / m - 0.5, (float(cy) + 0.5) / m - 0.5


def project(points, w2c12, H, W, fx, fy, cx, cy, near, far):
    """(z fp64 [N], i, j int64 [N], ok bool [N]): camera depth, nearest pixel centre and (in range and inside the image)"""
    cam = R.vertex_pass(points, w2c12)                               # points -> fp32, ((w0 x + w1 y) + w2 z) + w3 in fp32
    x, y, z = (cam[:, c].astype(np.float64) for c in range(3))
    in_range = (z >= near) & (z <= far)
    with np.errstate(divide="ignore", invalid="ignore"):
        i = np.floor(((x / z) * fx + cx) + 0.5)
        j = np.floor(((y / z) * fy + cy) + 0.5)
        inside = (i >= 0) & (i < W) & (j >= 0) & (j < H)
    ok = in_range & inside
    return z, np.where(ok, i, 0).astype(np.int64), np.where(ok, j, 0).astype(np.int64), ok


def visible(points, w2c12, depth, fx, fy, cx, cy, near, far, eps):
    """bool [N]: the points one view (depth [H, W] fp32) sees"""
    H, W = depth.shape
    z, i, j, ok = project(points, w2c12, H, W, fx, fy, cx, cy, near, far)
    d = depth[j, i]
    return ok & ((d == 0) | (z <= d.astype(np.float64) + eps))


def visibility_counts(points, verts, faces, c2w, H, W, fx, fy, cx, cy, eps, near, far=1e3, raster_div=None, per_view=False):
    """int32 [N] (per_view: bool [K, N]): the views of c2w (OpenCV) that see each point against the mesh's z-buffers"""
    m = raster_divisor(H, W) if raster_div is None else raster_div
    Hs, Ws, fxs, fys, cxs, cys = scaled_camera(H, W, fx, fy, cx, cy, m)
    c2w = np.asarray(c2w, np.float64).reshape(-1, 4, 4)
    depth = R.render_views(verts, faces, c2w, Hs, Ws, fxs, fys, cxs, cys, near, far)
    w = R.w2c_rows(c2w)
    vis = np.stack([visible(points, w[k], depth[k], fxs, fys, cxs, cys, near, far, eps) for k in range(len(w))])
    return vis if per_view else vis.sum(0).astype(np.int32)


def frustum_counts(points, c2w, H, W, fx, fy, cx, cy, near, far=1e3, raster_div=None):
    """int32 [N]: the views in which a point is in range and inside the image, whatever is in front of it"""
    m = raster_divisor(H, W) if raster_div is None else raster_div
    Hs, Ws, fxs, fys, cxs, cys = scaled_camera(H, W, fx, fy, cx, cy, m)
    w = R.w2c_rows(c2w)
    return np.stack([project(points, w[k], Hs, Ws, fxs, fys, cxs, cys, near, far)[3] for k in range(len(w))]).sum(0).astype(np.int32)


def as_loaded(c2w):
    """the OpenCV poses (what a trajectory file stores) as load_poses returns them, y and z axes flipped: [K, 4, 4] fp64"""
    t = np.asarray(c2w, np.float64).reshape(-1, 4, 4).copy()
    t[:, :3, 1] *= -1.0
    t[:, :3, 2] *= -1.0
    return t
