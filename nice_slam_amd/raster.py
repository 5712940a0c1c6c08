"""Depth rendering of triangle meshes on the GPU and the 2-D depth metric of the reference's ``src/tools/eval_recon.py``
(``calc_2d_metric``, :131-211, with ``get_cam_position``, ``viewmatrix`` and ``check_proj``).  Re-exported by
``nice_slam_amd.recon``.

    from nice_slam_amd import recon
    depth = recon.render_depth(vertices, faces, c2w)              # [K, 500, 500] fp32 device tensor, 0 = background
    recon.calc_2d_metric("rec.ply", "gt.ply")                      # {"depth_l1_cm": ..., "per_view": ...}

    count = recon.visibility_counts(points, vertices, faces, c2w, 680, 1200, 600., 600., 599.5, 339.5)   # int32 [N]
    np.save("gt_pc_unseen.npy", recon.unseen_points("gt.ply", recon.load_poses("traj.txt")))

    python -m nice_slam_amd.recon depth --rec_mesh R --gt_mesh G
    python -m nice_slam_amd.recon unseen --gt_mesh G --traj traj.txt --output G_pc_unseen.npy

Every per-pixel and per-point loop runs in libnsr.so (include/nsr.h, "Depth rasterization"; the rules are written out in
csrc/nsr_raster.h): a tiled z-buffer rasterizer (nsr_raster_bin, nsr_raster_depth), the per-view depth L1 (nsr_depth_error),
the candidate-view test (nsr_view_unseen) and the visibility of points against the z-buffers of a trajectory
(nsr_points_visible).  The oriented box of the camera positions is the library's fp64 convex hull plus
a minimum-area rectangle per hull-face normal on the host.

Deviations from the reference (also in INTEGRATION.md):
  * not Open3D's OpenGL depth buffer: depth is the exact ray-plane depth rounded once to fp32 (no 24-bit depth quantization),
    coverage is a ray-triangle test that counts boundary pixels as covered (no GL fill rule);
  * near plane 0.01 x the largest axis-aligned extent of the mesh being rendered (Open3D's ViewControl rule for a camera
    inside the bounding box, recalled from its source), far plane 20;
  * the view stream is a seeded numpy Generator (the reference draws from the unseeded ``random`` / numpy streams);
  * the oriented box orders its axes by ascending extent (trimesh's ``oriented_bounds(ordered=True)`` as recalled; trimesh
    is not used) with each of the two shorter axes pointing to the positive side of its largest component;
  * ``visibility_counts`` and ``unseen_points`` have no counterpart in the reference: its cull is frustum-only and its unseen
    clouds ship as files for the authors' scenes.
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import _capi
from .bound import convex_hull, prefilter
from .engine import Engine, gpu, pose_stack, w2c_rows
from .recon import align_icp, sample_surface

__all__ = ["render_depth", "depth_l1", "oriented_bounds", "cam_position", "viewmatrix", "view_draws", "views_from_draws",
           "views_unseen", "sample_views", "calc_2d_metric", "raster_divisor", "scaled_camera", "visibility_counts", "unseen_points"]

H_REF, W_REF, FOCAL_REF = 500, 500, 300.0          # eval_recon.py:135-142
FAR_REF = 20.0                                     # ctr.set_constant_z_far(20)
NEAR_REL = 0.01                                    # near = 0.01 x the mesh's largest extent
MAX_VIEWS_PER_LAUNCH = 64
MAX_IMAGE = 1024                                   # the rasterizer's limit per image side (kRasterMaxTiles)
H_CULL, W_CULL, F_CULL, CX_CULL, CY_CULL = 680, 1200, 600.0, 599.5, 339.5      # cull_mesh.py's camera (Replica)
EPS_VISIBLE = 0.03                                 # a point this far (m) behind the rendered depth still counts as seen


def max_extent(vertices) -> float:
    """the largest axis-aligned extent of a vertex set (fp64)"""
    v = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.asarray(vertices))
    v = v.detach().to(torch.float64)
    if v.numel() == 0:
        return 0.0
    return float((v.amax(0) - v.amin(0)).max())


def launch_views(E: Engine, scene, H: int, W: int, requested, what: str) -> int:
    """views drawn per launch of ``scene`` (what ``checked_scene`` returns) at H x W: ``requested``, or what a quarter of the free
    memory allows, at most 64; never more than the scene has"""
    nv, nf, K = scene[0].shape[0], scene[1].shape[0], len(scene[2])
    if requested is not None:
        step = int(requested)
    elif E.device.type != "cuda":
        step = 8
    else:
        ntiles = ((W + 31) // 32) * ((H + 31) // 32)
        per_view = 16 * nv + 8 * nf + 4 * ntiles * ((nf + 255) // 256) + 8 * ntiles + 16 * nf + 4 * H * W
        step = int(max(1, min(MAX_VIEWS_PER_LAUNCH, torch.cuda.mem_get_info(E.device)[0] // 4 // per_view)))
    step = min(K, step)
    if step < 1:
        raise ValueError(f"{what}: views_per_launch must be positive (got {requested})")
    return step


def checked_scene(E: Engine, vertices, faces, c2w, near, what: str):
    """(vertices fp32, faces int32, w2c [K, 12] fp32, near) on the engine's device, checked: what a batch of views is drawn from"""
    v = E.tensor(vertices, torch.float32, what + ": vertices")
    f = E.faces(faces)
    c2w = pose_stack(c2w)
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise _capi.NsrError(what + ": empty mesh")
    if len(c2w) == 0:
        raise _capi.NsrError(what + ": no views")
    lo, hi = int(f.min()), int(f.max())
    if lo < 0 or hi >= v.shape[0]:
        raise _capi.NsrError(f"{what}: face indices out of range [0, {v.shape[0]}) (found {lo}..{hi})")
    if near is None:
        near = NEAR_REL * max_extent(vertices)
    if not near > 0.0:
        raise _capi.NsrError(f"{what}: near must be positive (got {near})")
    return v, f, torch.from_numpy(w2c_rows(c2w, np.float64)).to(E.device), near


def binned_batches(E: Engine, scene, camera, step: int, what: str):
    """The views of ``scene`` (what ``checked_scene`` returns) binned ``step`` at a time for ``camera`` = (H, W, fx, fy, cx, cy,
    near, far): yields (k0, kb, w2c[k0:k0 + kb], workspace, bins, n) per batch, ready for nsr_raster_depth or nsr_view_mesh.  One
    workspace sized for a full step and one entry counter serve every batch; the bins grow (to n + n // 4) only when a batch
    needs more, so memory is bounded by one batch whatever K is.  Call it under ``E.guard()``."""
    v, f, w2c, _ = scene
    nv, nf = v.shape[0], f.shape[0]
    nbytes = int(E.lib.nsr_raster_workspace_bytes(nv, nf, step, camera[0], camera[1]))
    if nbytes < 0:
        raise _capi.NsrError(f"{what}: unsupported sizes ({nv} vertices, {nf} faces, {camera[0]} x {camera[1]})")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=E.device)
    n_ent = torch.zeros(1, dtype=torch.int64, device=E.device)
    bins = torch.empty(1, dtype=torch.int32, device=E.device)
    for k0 in range(0, len(w2c), step):
        wk = w2c[k0:k0 + step]
        E.call("nsr_raster_bin", v.data_ptr(), nv, f.data_ptr(), nf, wk.data_ptr(), len(wk), *camera, ws.data_ptr(), n_ent.data_ptr())
        n = int(n_ent.item())
        if n > bins.numel():
            del bins
            bins = torch.empty(n + n // 4, dtype=torch.int32, device=E.device)
        yield k0, len(wk), wk, ws, bins, n


def render_depth(vertices, faces, c2w, H=H_REF, W=W_REF, fx=FOCAL_REF, fy=FOCAL_REF, cx=249.5, cy=249.5, near=None, far=FAR_REF,
                 engine: Optional[Engine] = None, views_per_launch=None) -> torch.Tensor:
    """Depth images [K, H, W] fp32 on the engine's device of the mesh (vertices [V, 3], faces [F, 3]) seen from each c2w
    ([4, 4] or [K, 4, 4], OpenCV convention: x right, y down, z forward).  Depth is camera-space z, 0 where nothing is drawn;
    fragments outside [near, far] are discarded; near defaults to 0.01 x the mesh's largest axis-aligned extent.
    ``views_per_launch``: as in ``visibility_counts``."""
    E = engine or gpu()
    scene = checked_scene(E, vertices, faces, c2w, near, "render_depth")
    v, f, w2c, near = scene
    out = torch.empty((len(w2c), int(H), int(W)), dtype=torch.float32, device=E.device)
    step = launch_views(E, scene, int(H), int(W), views_per_launch, "render_depth")
    camera = (int(H), int(W), float(fx), float(fy), float(cx), float(cy), float(near), float(far))
    with torch.no_grad(), E.guard():
        for k0, kb, wk, ws, bins, n in binned_batches(E, scene, camera, step, "render_depth"):
            E.call("nsr_raster_depth", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], wk.data_ptr(), kb, *camera, ws.data_ptr(),
                   bins.data_ptr(), n, out[k0:k0 + kb].data_ptr())
    return out


def depth_l1(a: torch.Tensor, b: torch.Tensor, engine: Optional[Engine] = None) -> torch.Tensor:
    """per-view mean |a - b| [K] fp64 of two depth stacks [K, H, W] fp32 (fixed-order fp64 sums: bit-identical run to run)"""
    E = engine or gpu()
    lib = E.lib
    a = a.detach().to(E.device, torch.float32).contiguous()
    b = b.detach().to(E.device, torch.float32).contiguous()
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"depth_l1: two stacks [K, H, W] of one shape (got {tuple(a.shape)}, {tuple(b.shape)})")
    K, n = a.shape[0], a.shape[1] * a.shape[2]
    if K == 0 or n == 0:
        raise _capi.NsrError("depth_l1: no views or empty images")
    out = torch.empty(K, dtype=torch.float64, device=E.device)
    partial = torch.empty(int(lib.nsr_depth_error_partial_doubles(K, n)), dtype=torch.float64, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_depth_error", a.data_ptr(), b.data_ptr(), K, n, partial.data_ptr(), out.data_ptr())
    return out


# --------------------------------------------------------------------------------------------------
# the box the cameras are drawn in (get_cam_position, eval_recon.py:120-128)
# --------------------------------------------------------------------------------------------------
def _hull2d(p: np.ndarray) -> np.ndarray:
    """indices of the 2-D convex hull of p [n, 2], counter-clockwise (monotone chain, collinear points dropped)"""
    order = np.lexsort((p[:, 1], p[:, 0]))

    def half(idx):
        h = []
        for i in idx:
            while len(h) >= 2:
                a, b = p[h[-2]], p[h[-1]]
                if (b[0] - a[0]) * (p[i][1] - a[1]) - (b[1] - a[1]) * (p[i][0] - a[0]) <= 0:
                    h.pop()
                else:
                    break
            h.append(i)
        return h

    lower, upper = half(order), half(order[::-1])
    return np.array(lower[:-1] + upper[:-1], dtype=np.int64)


def _min_rect(q: np.ndarray):
    """(area, (e, e_perp) unit directions, (lo, hi) along them) of the minimum-area rectangle around the 2-D points q:
    rotating calipers' candidates, one rectangle side on each hull edge"""
    h = q[_hull2d(q)]
    if len(h) < 3:
        h = q
    e = np.roll(h, -1, axis=0) - h
    L = np.linalg.norm(e, axis=1)
    e, L = e[L > 0], L[L > 0]
    e = e / L[:, None]
    p = np.stack([-e[:, 1], e[:, 0]], 1)
    a = h @ e.T                                    # [n_pts, n_edges]
    b = h @ p.T
    wa, wb = a.max(0) - a.min(0), b.max(0) - b.min(0)
    area = wa * wb
    j = int(np.argmin(area))
    return area[j], (e[j], p[j]), ((a[:, j].min(), a[:, j].max()), (b[:, j].min(), b[:, j].max()))


def _hull_points(vertices, E: Engine) -> np.ndarray:
    pts = prefilter(E.tensor(vertices, torch.float64, "oriented_bounds: vertices"), E).cpu().numpy()
    hv = convex_hull(pts, 1.0, lib=E.lib)
    return hv[0], hv[3]


def oriented_bounds(vertices, engine: Optional[Engine] = None):
    """(to_origin 4x4 fp64, extents [3] ascending): the smallest-volume box with one face parallel to a face of the convex
    hull (trimesh.bounds.oriented_bounds).  Box axes in the order of their extents, right-handed; to_origin maps the box's
    centre to the origin and its axes onto x, y, z."""
    E = engine or gpu()
    hv, planes = _hull_points(vertices, E)
    normals = np.unique(np.round(planes[:, :3], 12), axis=0)
    best = None
    for n in normals:
        n = n / np.linalg.norm(n)
        t = np.eye(3)[int(np.argmin(np.abs(n)))]
        u = np.cross(n, t)
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        q = np.stack([hv @ u, hv @ w], 1)
        hn = hv @ n
        area, (e, p), ((a0, a1), (b0, b1)) = _min_rect(q)
        vol = area * (hn.max() - hn.min())
        if best is None or vol < best[0]:
            ax = [e[0] * u + e[1] * w, p[0] * u + p[1] * w, n]
            ext = [a1 - a0, b1 - b0, hn.max() - hn.min()]
            mid = [(a0 + a1) / 2, (b0 + b1) / 2, (hn.max() + hn.min()) / 2]
            best = (vol, ax, ext, mid)
    _, ax, ext, mid = best
    centre = sum(m * a for m, a in zip(mid, ax))
    order = np.argsort(ext, kind="stable")
    R = np.stack([ax[i] for i in order], 1)
    for c in range(2):
        if R[int(np.argmax(np.abs(R[:, c]))), c] < 0:
            R[:, c] = -R[:, c]
    R[:, 2] = np.cross(R[:, 0], R[:, 1])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, centre
    return np.linalg.inv(T), np.asarray(ext, np.float64)[order]


def cam_position(vertices, faces=None, engine: Optional[Engine] = None):
    """(extents [3], transform 4x4) of the box camera origins are drawn in, as get_cam_position: the oriented bounds of the
    ground-truth mesh, extents scaled by (0.3, 0.7, 0.7) (the shortest axis: the room's height), the centre raised by 0.4
    on world z.  ``faces`` is accepted for symmetry with the reference's mesh argument; the box reads only the vertices."""
    to_origin, extents = oriented_bounds(vertices, engine)
    extents = extents.copy()
    extents[2] *= 0.7
    extents[1] *= 0.7
    extents[0] *= 0.3
    transform = np.linalg.inv(to_origin)
    transform[2, 3] += 0.4
    return extents, transform


# --------------------------------------------------------------------------------------------------
# candidate views (calc_2d_metric's rejection loop, :162-180)
# --------------------------------------------------------------------------------------------------
def _normalize(x):
    return x / np.linalg.norm(x)


def viewmatrix(z, up, pos) -> np.ndarray:
    """3x4 [x | y | z | pos] of a camera at pos looking along z: x = normalize(up x z), y = normalize(z x x)"""
    v2 = _normalize(z)
    v0 = _normalize(np.cross(up, v2))
    v1 = _normalize(np.cross(v2, v0))
    return np.stack([v0, v1, v2, pos], 1)


def view_draws(n: int, rng: np.random.Generator) -> np.ndarray:
    """[n, 6] uniforms in [0, 1) per candidate: three for the origin in the box, three for the target"""
    return rng.random((n, 6))


def views_from_draws(extents, transform, draws) -> np.ndarray:
    """[M, 4, 4] fp64 candidate c2w from draws [M, 6]: origin = transform (u - 0.5) extents (trimesh's volume_rectangular),
    target = round(uniform(-1e4, 1e4), 2) - origin per axis, up = (0, 0, -1)"""
    draws = np.asarray(draws, np.float64).reshape(-1, 6)
    extents = np.asarray(extents, np.float64)
    transform = np.asarray(transform, np.float64)
    out = np.zeros((len(draws), 4, 4))
    for i, d in enumerate(draws):
        p = (d[:3] - 0.5) * extents
        origin = np.dot(transform, np.append(p, 1.0))[:3]
        tgt = np.array([round(-10000.0 + 20000.0 * float(x), 2) for x in d[3:]])
        m = np.eye(4)
        m[:3, :] = viewmatrix(tgt - origin, [0, 0, -1], origin)
        out[i] = m
    return out


def views_unseen(c2w, unseen, H=H_REF, W=W_REF, fx=FOCAL_REF, fy=FOCAL_REF, cx=249.5, cy=249.5,
                 engine: Optional[Engine] = None) -> np.ndarray:
    """bool [M]: check_proj of each candidate c2w against the unseen cloud: True iff the candidate sees some point of it"""
    E = engine or gpu()
    c2w = pose_stack(c2w, flip_yz=True)
    w2c = torch.from_numpy(w2c_rows(c2w, np.float64)).to(E.device)
    pts = E.tensor(unseen, what="unseen points")
    sees = torch.empty(len(c2w), dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_view_unseen", pts.data_ptr(), pts.shape[0], int(pts.dtype == torch.float64), w2c.data_ptr(), len(c2w), int(H), int(W),
               float(fx), float(fy), float(cx), float(cy), sees.data_ptr())
    return sees.cpu().numpy().astype(bool)


def sample_views(extents, transform, n, unseen=None, seed=0, draws=None, H=H_REF, W=W_REF, fx=FOCAL_REF, fy=FOCAL_REF, cx=249.5,
                 cy=249.5, engine: Optional[Engine] = None, max_candidates=10_000_000) -> np.ndarray:
    """[n, 4, 4] fp64 c2w: the first n candidates, in draw order, that see no point of ``unseen`` (None: every candidate is
    accepted) -- the reference's sequential rejection loop fed by numpy.random.default_rng(seed), or by ``draws`` [M, 6]."""
    E = engine or gpu()
    n = int(n)
    rng = np.random.default_rng(seed)
    out, used = [], 0
    while len(out) < n:
        if draws is not None:
            if used >= len(draws):
                raise ValueError(f"sample_views: the {len(draws)} draws give only {len(out)} accepted views of {n}")
            d = np.asarray(draws)[used:used + max(64, 2 * (n - len(out)))]
        else:
            if used >= max_candidates:
                raise RuntimeError(f"sample_views: {used} candidates drawn, {len(out)} of {n} accepted: the unseen cloud is in "
                                   "almost every view")
            d = view_draws(min(4096, max(64, 2 * (n - len(out)))), rng)
        used += len(d)
        c2w = views_from_draws(extents, transform, d)
        ok = np.ones(len(c2w), bool) if unseen is None else ~views_unseen(c2w, unseen, H, W, fx, fy, cx, cy, E)
        out.extend(c2w[ok][: n - len(out)])
    return np.asarray(out, np.float64).reshape(n, 4, 4)


# --------------------------------------------------------------------------------------------------
# the 2-D metric (calc_2d_metric, eval_recon.py:131-211)
# --------------------------------------------------------------------------------------------------
def calc_2d_metric(rec_mesh, gt_mesh, align=True, n_imgs=1000, unseen=None, seed=0, H=H_REF, W=W_REF, fx=FOCAL_REF, fy=FOCAL_REF,
                   cx=249.5, cy=249.5, views_per_batch=100, engine: Optional[Engine] = None):
    """Depth L1 [cm] of a reconstructed mesh against the ground truth, as calc_2d_metric: (optionally) ICP-align the
    reconstruction, draw ``n_imgs`` views in the box of cam_position that see no point of the unseen cloud, render both
    meshes at 500 x 500 (f = 300) and average the per-view mean |gt - rec|.  Meshes: PLY paths or (vertices, faces) pairs.
    ``unseen``: None = the ground truth's ``_pc_unseen.npy`` beside it (required), a path or [N, 3] array, or False (accept
    every candidate).  The intrinsics default to the reference's.  Returns {"depth_l1_cm": float, "per_view": fp64 [n_imgs]
    (m), "c2w": fp64 [n_imgs, 4, 4]}."""
    E = engine or gpu()
    if unseen is None:
        if not isinstance(gt_mesh, str):
            raise ValueError("calc_2d_metric: pass unseen= (a path, an array or False) with an in-memory ground truth")
        unseen = gt_mesh.replace(".ply", "_pc_unseen.npy")
        if not os.path.exists(unseen):
            raise FileNotFoundError(f"calc_2d_metric: the unseen point cloud {unseen} is missing (pass unseen=False to accept every view)")
    if isinstance(unseen, str):
        unseen = np.load(unseen)
    if unseen is False:
        unseen = None
    rv, rf = E.mesh(rec_mesh)
    gv, gf = E.mesh(gt_mesh)
    if align:
        T = align_icp(rv, gv, 0.1, engine=E)[0]
        rv = rv.clone()
        E.transform(rv, T)
    extents, transform = cam_position(gv, gf, E)
    poses = sample_views(extents, transform, n_imgs, unseen, seed, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, engine=E)
    near_gt, near_rec = NEAR_REL * max_extent(gv), NEAR_REL * max_extent(rv)
    per_view = []
    for k0 in range(0, len(poses), views_per_batch):
        c2w = poses[k0:k0 + views_per_batch]
        gt_d = render_depth(gv, gf, c2w, H, W, fx, fy, cx, cy, near=near_gt, engine=E)
        rec_d = render_depth(rv, rf, c2w, H, W, fx, fy, cx, cy, near=near_rec, engine=E)
        per_view.append(depth_l1(gt_d, rec_d, E).cpu().numpy())
        del gt_d, rec_d
    per_view = np.concatenate(per_view) if per_view else np.zeros(0)
    total = 0.0
    for x in per_view:                              # in view order
        total += float(x)
    return {"depth_l1_cm": total / max(len(per_view), 1) * 100, "per_view": per_view, "c2w": poses}


# --------------------------------------------------------------------------------------------------
# visibility of points over a trajectory: occlusion-aware culling and unseen-region clouds
# --------------------------------------------------------------------------------------------------
def raster_divisor(H: int, W: int) -> int:
    """the smallest integer m with ceil(H / m) <= 1024 and ceil(W / m) <= 1024: the scale the rasterizer renders H x W at"""
    m = 1
    while -(-int(H) // m) > MAX_IMAGE or -(-int(W) // m) > MAX_IMAGE:
        m += 1
    return m


def scaled_camera(H, W, fx, fy, cx, cy, m: int):
    """(Hs, Ws, fx, fy, cx, cy) of the image at 1 / m scale: pixel (i, j) of it covers the m x m block at (m i, m j), so a
    pixel centre u of the full image lies at (u + 0.5) / m - 0.5"""
    m = int(m)
    if m < 1:
        raise ValueError(f"raster_div must be a positive integer (got {m})")
    return -(-int(H) // m), -(-int(W) // m), float(fx) / m, float(fy) / m, (float(cx) + 0.5) / m - 0.5, (float(cy) + 0.5) / m - 0.5


def visibility_counts(points, vertices, faces, c2w, H, W, fx, fy, cx, cy, eps=EPS_VISIBLE, near=None, far=1e3, raster_div=None,
                      views_per_launch=None, engine: Optional[Engine] = None) -> torch.Tensor:
    """int32 [N] on the engine's device: for each of ``points`` [N, 3] (fp32 / fp64) the number of the poses ``c2w`` ([K, 4, 4],
    OpenCV convention) that see it: the point lies in [near, far], projects into the H x W image and is at most ``eps`` behind
    the depth of the mesh (vertices, faces) at the nearest pixel centre.  The depth images are rendered a batch of views at a
    time into one reused stack (``views_per_launch``: default what the free memory allows, at most 64) and the counts
    accumulate over the batches, so memory is bounded by one batch whatever K is.  Images larger than the rasterizer's 1024
    pixels a side are rendered at 1 / m scale (``raster_div``, default the smallest m that fits: 2 for 680 x 1200) with the
    intrinsics of ``scaled_camera``.  near defaults to 0.01 x the mesh's largest axis-aligned extent."""
    E = engine or gpu()
    pts = E.tensor(points, what="visibility_counts: points")
    scene = checked_scene(E, vertices, faces, c2w, near, "visibility_counts")
    v, f, w2c, near = scene
    N = pts.shape[0]
    m = raster_divisor(H, W) if raster_div is None else int(raster_div)
    Hs, Ws, fxs, fys, cxs, cys = scaled_camera(H, W, fx, fy, cx, cy, m)
    count = torch.zeros(N, dtype=torch.int32, device=E.device)
    if N == 0:
        return count
    step = launch_views(E, scene, Hs, Ws, views_per_launch, "visibility_counts")
    camera = (Hs, Ws, fxs, fys, cxs, cys, float(near), float(far))
    with torch.no_grad(), E.guard():
        depth = torch.empty((step, Hs, Ws), dtype=torch.float32, device=E.device)   # one batch's depth stack, reused by every batch
        for _, kb, wk, ws, bins, n in binned_batches(E, scene, camera, step, "visibility_counts"):
            E.call("nsr_raster_depth", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], wk.data_ptr(), kb, *camera, ws.data_ptr(),
                   bins.data_ptr(), n, depth.data_ptr())
            E.call("nsr_points_visible", pts.data_ptr(), N, int(pts.dtype == torch.float64), wk.data_ptr(), kb, depth.data_ptr(), Hs, Ws,
                   fxs, fys, cxs, cys, float(near), float(far), float(eps), count.data_ptr())
    return count


def unseen_points(gt_mesh, c2w_list, n_points=200000, seed=0, H=H_CULL, W=W_CULL, fx=F_CULL, fy=F_CULL, cx=CX_CULL, cy=CY_CULL,
                  eps=EPS_VISIBLE, stride=1, near=None, far=1e3, raster_div=None, views_per_launch=None,
                  engine: Optional[Engine] = None) -> np.ndarray:
    """fp64 [M, 3]: the points of ``n_points`` seeded surface samples of the ground-truth mesh (a PLY path or a (vertices,
    faces) pair) that no pose of the trajectory sees, tested against the mesh's own z-buffers: the ``<gt_mesh>_pc_unseen.npy``
    that calc_2d_metric rejects candidate views with.  ``c2w_list``: the poses as ``load_poses`` returns them (y and z axes
    flipped), every ``stride``-th one used; the camera defaults to cull_mesh.py's."""
    E = engine or gpu()
    gv, gf = E.mesh(gt_mesh)
    c2w = pose_stack(list(c2w_list)[::int(stride)], flip_yz=True)
    pts = sample_surface(gv, gf, n_points, seed=seed, engine=E)[0]
    count = visibility_counts(pts, gv, gf, c2w, H, W, fx, fy, cx, cy, eps=eps, near=near, far=far, raster_div=raster_div,
                              views_per_launch=views_per_launch, engine=E)
    return pts[count == 0].cpu().numpy()
