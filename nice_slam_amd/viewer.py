"""Headless replay of a SLAM run on the GPU: what the reference's ``visualizer.py`` shows in an Open3D window through
``src/tools/viz.py`` (``SLAMFrontend``) -- the newest mesh shaded with back faces hidden, the estimated and ground-truth camera as
point-sampled wireframes, both trajectories as point clouds, one JPEG per frame for ``vis.mp4`` -- without a window or a display.

    from nice_slam_amd import viewer
    rgb, depth, face = viewer.render_mesh(vertices, faces, c2w, 540, 960, 467.65, 467.65, 479.5, 269.5, colors=colors, cull="back")
    replay = viewer.Replay(init_pose=est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt)
    replay.update_mesh("output/mesh/00500_mesh.ply"); replay.update_pose(1, est[500]); replay.save("frame.jpg")

    python -m nice_slam_amd.viewer --output output/Replica/room0 --scale 1        # -> output/Replica/room0/tmp_rendering/*.jpg
    python -m nice_slam_amd.viewer --output output/Replica/room0 --video          # ... encoded on the GPU, and output/.../vis.avi

Every per-pixel and per-vertex loop runs in libnsr.so (include/nsr.h, "Replay view"; the rules are written out in
csrc/nsr_view.h): area-weighted vertex normals (nsr_view_normals), the mesh layer over the depth rasterizer's bins
(nsr_raster_bin, nsr_view_mesh: depth, owning face, headlight-shaded colour, a cull mode) and the point layer drawn over it with
a depth test (nsr_view_points).

Deviations from the reference (also in INTEGRATION.md):
  * not Open3D's renderer: headlight shading ``0.35 + 0.65 |n . d|`` of the interpolated vertex normal instead of its Phong
    lights, the rasterizer's inclusive ray-triangle coverage instead of the GL fill rule, points as axis-aligned squares with a
    per-pixel depth test instead of GL point sprites;
  * 960 x 540 by default, half the reference's 1920 x 1080 window: the rasterizer draws at most 1024 pixels a side;
  * the pinhole camera is Open3D's default as recalled (vertical field of view 60 degrees, principal point at the image centre);
  * near is 0.01 x the mesh's largest extent, as ``render_depth`` derives it (the reference passes 0);
  * no interactive window, no ``--vis_input_frame``; one image per replayed frame (the reference captures one per redraw of its
    window, however many frames were queued meanwhile).
"""
from __future__ import annotations

import argparse
import glob
import math
import os
from typing import Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, gpu, pose_stack, to_numpy, w2c_rows
from .ply import read_mesh
from .raster import binned_batches, checked_scene, launch_views, max_extent, NEAR_REL

__all__ = ["vertex_normals", "render_mesh", "draw_points", "camera_actor", "viewer_pose", "default_camera", "config_scale", "Replay",
           "replay_run", "save_image", "main"]

CULL = {None: 0, "none": 0, "back": 1, "front": 2}
WIDTH, HEIGHT = 960, 540                            # half of viz.py:158
POINT_SIZE = 4                                      # viz.py:159
FAR = 1000.0                                        # viz.py:164
FOV_DEG = 60.0                                      # Open3D's default vertical field of view, as recalled
FRAMES_PER_LAUNCH = 64
RED, BLACK = (255, 0, 0), (0, 0, 0)                 # viz.py:37: the estimate, the ground truth

# viz.py:14-26 restated: the apex, the image rectangle at depth 1.5 and the "up" marker above it; the rectangle, its diagonals, the
# four rays from the apex and the marker's two strokes
_CAM_POINTS = ((0, 0, 0), (-1, -1, 1.5), (1, -1, 1.5), (1, 1, 1.5), (-1, 1, 1.5), (-0.5, 1, 1.5), (0.5, 1, 1.5), (0, 1.2, 1.5))
_CAM_LINES = ((1, 2), (2, 3), (3, 4), (4, 1), (1, 3), (2, 4), (1, 0), (0, 2), (3, 0), (0, 4), (5, 7), (7, 6))
_POINTS_PER_LINE = 100


# --------------------------------------------------------------------------------------------------
# the three library pieces
# --------------------------------------------------------------------------------------------------
def vertex_normals(vertices, faces, return_sums: bool = False, engine: Optional[Engine] = None):
    """fp32 [V, 3] on the engine's device: per vertex the normalised sum of its faces' cross products (V1 - V0) x (V2 - V0),
    summed in fp64 in ascending face id -- area-weighted, Open3D's ``compute_vertex_normals`` as recalled.  A vertex of no face,
    or one whose faces cancel, gets (0, 0, 0).  ``return_sums``: also the fp64 sums [V, 3]."""
    E = engine or gpu()
    v = E.tensor(vertices, torch.float32, "vertex_normals: vertices")
    f = E.faces(faces)
    nv, nf = v.shape[0], f.shape[0]
    if nv == 0 or nf == 0:
        raise _capi.NsrError("vertex_normals: empty mesh")
    lo, hi = int(f.min()), int(f.max())
    if lo < 0 or hi >= nv:
        raise _capi.NsrError(f"vertex_normals: face indices out of range [0, {nv}) (found {lo}..{hi})")
    flat = f.reshape(-1).long()
    order = torch.sort(flat, stable=True)[1]                     # entry 3 f + c: a vertex's entries stay in ascending face id
    incident = torch.div(order, 3, rounding_mode="floor").to(torch.int32).contiguous()
    start = torch.zeros(nv + 1, dtype=torch.int64, device=E.device)
    start[1:] = torch.cumsum(torch.bincount(flat, minlength=nv), 0)
    sums = torch.empty((nv, 3), dtype=torch.float64, device=E.device)
    out = torch.empty((nv, 3), dtype=torch.float32, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_view_normals", v.data_ptr(), nv, f.data_ptr(), nf, start.data_ptr(), incident.data_ptr(), incident.numel(),
               sums.data_ptr(), out.data_ptr())
    return (out, sums) if return_sums else out


def _u8(E: Engine, a, n: int, what: str) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 2 or t.shape[0] != n or t.shape[1] < 3 or t.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8 [{n}, 3] (got {t.dtype} {tuple(t.shape)})")
    return t.detach()[:, :3].to(E.device).contiguous()


def render_mesh(vertices, faces, c2w, H=HEIGHT, W=WIDTH, fx=None, fy=None, cx=None, cy=None, colors=None, normals=None, cull=None,
                near=None, far=FAR, engine: Optional[Engine] = None, views_per_launch=None):
    """(rgb uint8 [K, H, W, 3], depth fp32 [K, H, W], face int32 [K, H, W]) on the engine's device: the mesh seen from each c2w
    ([4, 4] or [K, 4, 4], OpenCV convention), shaded by a headlight.  ``colors``: uint8 [V, 3] vertex colours (None: grey),
    ``normals``: fp32 [V, 3] (None: ``vertex_normals``), ``cull``: None / "none", "back" (hide the faces whose normal
    (V1 - V0) x (V2 - V0) points away from the camera) or "front".  Background: white, depth 0, face -1.  With no culling the
    depth is ``render_depth``'s bit for bit.  Intrinsics default to ``default_camera(H, W)``; near to 0.01 x the mesh's extent.
    ``views_per_launch``: as in ``raster.visibility_counts``."""
    E = engine or gpu()
    if cull not in CULL:
        raise _capi.NsrError(f"render_mesh: bad cull mode {cull!r} (None, 'none', 'back', 'front')")
    H, W = int(H), int(W)
    dfx, dfy, dcx, dcy = default_camera(H, W)
    fx, fy, cx, cy = (float(d if a is None else a) for a, d in ((fx, dfx), (fy, dfy), (cx, dcx), (cy, dcy)))
    scene = checked_scene(E, vertices, faces, c2w, near, "render_mesh")
    v, f, w2c, near = scene
    nv, nf, K = v.shape[0], f.shape[0], len(w2c)
    nrm = vertex_normals(v, f, engine=E) if normals is None else E.tensor(normals, torch.float32, "render_mesh: normals")
    if nrm.shape[0] != nv:
        raise ValueError(f"render_mesh: {nrm.shape[0]} normals for {nv} vertices")
    col = None if colors is None else _u8(E, colors, nv, "render_mesh: colors")
    rgb = torch.empty((K, H, W, 3), dtype=torch.uint8, device=E.device)
    depth = torch.empty((K, H, W), dtype=torch.float32, device=E.device)
    face = torch.empty((K, H, W), dtype=torch.int32, device=E.device)
    step = launch_views(E, scene, H, W, views_per_launch, "render_mesh")
    camera = (H, W, fx, fy, cx, cy, float(near), float(far))
    with torch.no_grad(), E.guard():
        for k0, kb, wk, ws, bins, n in binned_batches(E, scene, camera, step, "render_mesh"):
            E.call("nsr_view_mesh", v.data_ptr(), nv, f.data_ptr(), nf, wk.data_ptr(), kb, *camera, ws.data_ptr(), bins.data_ptr(), n,
                   nrm.data_ptr(), None if col is None else col.data_ptr(), CULL[cull], depth[k0:k0 + kb].data_ptr(),
                   face[k0:k0 + kb].data_ptr(), rgb[k0:k0 + kb].data_ptr())
    return rgb, depth, face


def draw_points(rgb, depth, points, colors, offsets, c2w, fx=None, fy=None, cx=None, cy=None, near=0.01, far=FAR, size=POINT_SIZE,
                return_owner: bool = False, engine: Optional[Engine] = None):
    """uint8 [B, H, W, 3] on the engine's device: B frames of points drawn as ``size`` x ``size`` squares over a base layer.
    ``rgb`` / ``depth``: the base, uint8 [H, W, 3] / fp32 [H, W] shared by every frame, or [B, H, W, 3] / [B, H, W] one per frame
    (``render_mesh``'s outputs; depth 0 hides nothing).  Frame b draws ``points[offsets[b]:offsets[b + 1]]`` ([N, 3], colours
    uint8 [N, 3], unshaded) from ``c2w[b]``.  A pixel of a point is drawn iff the point is not behind the base there; the nearest
    point wins, then the one listed first.  ``return_owner``: also int32 [B, H, W], the index in its frame of the point drawn
    (-1: the base shows)."""
    E = engine or gpu()
    base_rgb = (rgb if isinstance(rgb, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rgb))).detach().to(E.device).contiguous()
    base_d = (depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(depth))).detach()
    base_d = base_d.to(E.device, torch.float32).contiguous()
    if base_rgb.dtype != torch.uint8 or base_rgb.dim() not in (3, 4) or base_rgb.shape[-1] != 3 or base_d.shape != base_rgb.shape[:-1]:
        raise ValueError(f"draw_points: base uint8 [.., H, W, 3] with depth [.., H, W] (got {base_rgb.dtype} {tuple(base_rgb.shape)}, "
                         f"{tuple(base_d.shape)})")
    per_frame = base_rgb.dim() == 4
    H, W = int(base_rgb.shape[-3]), int(base_rgb.shape[-2])
    poses = pose_stack(c2w)
    B = len(poses)
    if B == 0:
        raise _capi.NsrError("draw_points: no views")
    if per_frame and base_rgb.shape[0] != B:
        raise ValueError(f"draw_points: {base_rgb.shape[0]} base layers for {B} frames")
    off = torch.as_tensor(np.asarray(to_numpy(offsets), np.int64).reshape(-1))
    pts = E.tensor(np.zeros((0, 3), np.float32) if len(points) == 0 else points, torch.float32, "draw_points: points")
    N = pts.shape[0]
    col = _u8(E, np.zeros((0, 3), np.uint8) if N == 0 else colors, N, "draw_points: colors")
    if off.numel() != B + 1 or int(off[0]) != 0 or int(off[-1]) != N or bool((off[1:] < off[:-1]).any()):
        raise ValueError(f"draw_points: offsets must rise from 0 to {N} in {B + 1} entries")
    off = off.to(E.device)
    dfx, dfy, dcx, dcy = default_camera(H, W)
    fx, fy, cx, cy = (float(d if a is None else a) for a, d in ((fx, dfx), (fy, dfy), (cx, dcx), (cy, dcy)))
    w2c = torch.from_numpy(w2c_rows(poses, np.float64)).to(E.device)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=E.device)
    owner = torch.empty((B, H, W), dtype=torch.int32, device=E.device) if return_owner else None
    with torch.no_grad(), E.guard():
        E.call("nsr_view_points", pts.data_ptr() if N else None, col.data_ptr() if N else None, N, off.data_ptr(), w2c.data_ptr(), B, H, W,
               fx, fy, cx, cy, float(near), float(far), int(size), base_rgb.data_ptr(), base_d.data_ptr(), int(per_frame), out.data_ptr(),
               None if owner is None else owner.data_ptr())
    return (out, owner) if return_owner else out


# --------------------------------------------------------------------------------------------------
# the scene around the mesh (viz.py)
# --------------------------------------------------------------------------------------------------
def default_camera(H: int, W: int, fov_deg: float = FOV_DEG):
    """(fx, fy, cx, cy) of the pinhole camera of an H x W window: vertical field of view ``fov_deg``, square pixels, the
    principal point at the image centre"""
    f = 0.5 * H / math.tan(math.radians(fov_deg) / 2.0)
    return f, f, (W - 1) / 2.0, (H - 1) / 2.0


def camera_actor(c2w, scale: float, is_gt: bool = False):
    """(points fp64 [1200, 3], colour uint8 [3]): the camera wireframe of viz.py:14-42 moved by the 4 x 4 ``c2w`` -- 8 corner
    points times ``scale``, 12 segments, 100 evenly spaced points on each (both ends included); red for the estimate, black for
    the ground truth"""
    corners = float(scale) * np.array(_CAM_POINTS, np.float64)
    t = np.linspace(0.0, 1.0, _POINTS_PER_LINE)
    pts = np.concatenate([corners[a][None, :] * (1.0 - t)[:, None] + corners[b][None, :] * t[:, None] for a, b in _CAM_LINES])
    m = np.asarray(to_numpy(c2w), np.float64)
    return pts @ m[:3, :3].T + m[:3, 3], np.array(BLACK if is_gt else RED, np.uint8)


def viewer_pose(first_c2w) -> np.ndarray:
    """The viewer's c2w (fp64 4 x 4, OpenCV convention: x right, y down, z forward) behind the run's first pose, viz.py:166-171:
    2 m along the pose's normalised z column (backwards for the run's OpenGL-style poses), then columns 1 and 2 negated"""
    m = np.array(to_numpy(first_c2w), np.float64)
    z = m[:3, 2]
    m[:3, 3] = m[:3, 3] + 2.0 * (z / np.linalg.norm(z))
    m[:3, 2] *= -1.0
    m[:3, 1] *= -1.0
    return m


class Replay:
    """``SLAMFrontend`` (viz.py:180-209) without a window or a process.  The update calls change the scene; ``frame()`` draws
    it.  ``view="first"``: one fixed viewer behind the first pose -- the mesh layer is rendered once per mesh and every frame
    is a point layer over it; ``view="follow"``: the viewer sits behind the newest estimated pose.  ``snapshot()`` queues the
    scene as it is and ``flush()`` draws the queue, up to 64 frames a launch."""

    def __init__(self, init_pose, cam_scale=1.0, estimate_c2w_list=None, gt_c2w_list=None, width=WIDTH, height=HEIGHT, cull="back",
                 view="first", near=None, far=FAR, point_size=POINT_SIZE, engine: Optional[Engine] = None):
        if view not in ("first", "follow"):
            raise ValueError(f"Replay: view must be 'first' or 'follow' (got {view!r})")
        if cull not in CULL:
            raise _capi.NsrError(f"Replay: bad cull mode {cull!r}")
        self.E = engine or gpu()
        self.W, self.H = int(width), int(height)
        self.camera = default_camera(self.H, self.W)
        self.cull, self.view, self.near, self.far, self.point_size = cull, view, near, float(far), int(point_size)
        self.cam_scale = float(cam_scale)
        self.first_view = viewer_pose(init_pose)
        self.lists = {False: None if estimate_c2w_list is None else np.asarray(to_numpy(estimate_c2w_list), np.float64),
                      True: None if gt_c2w_list is None else np.asarray(to_numpy(gt_c2w_list), np.float64)}
        self.mesh = None
        self._base = None
        self._pending, self._ready = [], []
        self.reset()
        self.traj = {}
        self.follow_pose = np.array(to_numpy(init_pose), np.float64)

    # ---- the scene ----
    def update_pose(self, index, pose, gt=False):
        """the camera actor ``index`` of the estimate / ground truth at ``pose`` (viz.py:188-193: its z column negated, so the
        wireframe opens along the viewing direction; the caller's array is left as it is)"""
        m = np.array(to_numpy(pose), np.float64)
        if not gt:
            self.follow_pose = m.copy()
        m[:3, 2] *= -1.0
        self.cameras[(int(index), bool(gt))] = m

    def update_mesh(self, mesh):
        """a PLY path or (vertices, faces[, colours uint8]); the face orientation is flipped as viz.py:95-101 does.  Frames queued
        so far are drawn with the mesh they were queued with."""
        self._render_pending()
        if isinstance(mesh, str):
            v, f, c = read_mesh(mesh, colors=True)
        else:
            v, f, c = mesh[0], mesh[1], (mesh[2] if len(mesh) > 2 else None)
        E = self.E
        v = E.tensor(v, torch.float32, "Replay: vertices")
        f = E.faces(f).flip(1).contiguous()
        self._base = None
        if v.shape[0] == 0 or f.shape[0] == 0:
            self.mesh = None
            return
        c = None if c is None else _u8(E, c, v.shape[0], "Replay: colours")
        self.mesh = {"v": v, "f": f, "c": c, "n": vertex_normals(v, f, engine=E), "near": NEAR_REL * max_extent(v)}

    def update_cam_trajectory(self, i, gt=False):
        """the trajectory cloud of the estimate / ground truth up to frame ``i``: ``c2w_list[1:i, :3, 3]`` (viz.py:104-125)"""
        lst = self.lists[bool(gt)]
        if lst is None:
            raise ValueError("Replay: no pose list for this trajectory")
        self.traj[bool(gt)] = lst[1:int(i), :3, 3].copy()

    def reset(self):
        """drop the camera actors (viz.py:127-137)"""
        self.cameras = {}

    # ---- drawing ----
    def scene_points(self):
        """(points fp32 [N, 3], colours uint8 [N, 3]) of the scene as it is: camera actors, then trajectories"""
        pts, cols = [np.zeros((0, 3))], [np.zeros((0, 3), np.uint8)]
        for (_, gt), m in sorted(self.cameras.items()):
            p, c = camera_actor(m, self.cam_scale, gt)
            pts.append(p)
            cols.append(np.broadcast_to(c, p.shape))
        for gt in sorted(self.traj):
            p = self.traj[gt]
            pts.append(p)
            cols.append(np.broadcast_to(np.array(BLACK if gt else RED, np.uint8), p.shape))
        return np.concatenate(pts).astype(np.float32), np.ascontiguousarray(np.concatenate(cols))

    def current_view(self) -> np.ndarray:
        return self.first_view if self.view == "first" else viewer_pose(self.follow_pose)

    def _near(self):
        if self.near is not None:
            return float(self.near)
        return self.mesh["near"] if self.mesh is not None else 0.01

    def _mesh_layer(self, c2w):
        K = len(c2w)
        if self.mesh is None:
            return (torch.full((K, self.H, self.W, 3), 255, dtype=torch.uint8, device=self.E.device),
                    torch.zeros((K, self.H, self.W), dtype=torch.float32, device=self.E.device))
        m = self.mesh
        rgb, depth, _ = render_mesh(m["v"], m["f"], c2w, self.H, self.W, *self.camera, colors=m["c"], normals=m["n"], cull=self.cull,
                                    near=self._near(), far=self.far, engine=self.E)
        return rgb, depth

    def snapshot(self):
        """queue the scene as it is for ``flush()``"""
        p, c = self.scene_points()
        self._pending.append((p, c, self.current_view().copy()))

    def _render_pending(self):
        while self._pending:
            batch, self._pending = self._pending[:FRAMES_PER_LAUNCH], self._pending[FRAMES_PER_LAUNCH:]
            views = np.stack([b[2] for b in batch])
            if self.view == "first":
                if self._base is None:
                    rgb, depth = self._mesh_layer(views[:1])
                    self._base = (rgb[0], depth[0])
                base = self._base
            else:
                base = self._mesh_layer(views)
            offsets = np.concatenate([[0], np.cumsum([len(b[0]) for b in batch])])
            self._ready.append(draw_points(base[0], base[1], np.concatenate([b[0] for b in batch]), np.concatenate([b[1] for b in batch]),
                                           offsets, views, *self.camera, near=self._near(), far=self.far, size=self.point_size,
                                           engine=self.E))

    def flush(self) -> torch.Tensor:
        """uint8 [n, H, W, 3] on the device: the queued frames, in order"""
        self._render_pending()
        out, self._ready = self._ready, []
        if not out:
            return torch.empty((0, self.H, self.W, 3), dtype=torch.uint8, device=self.E.device)
        return out[0] if len(out) == 1 else torch.cat(out)

    def frame(self) -> torch.Tensor:
        """uint8 [H, W, 3] on the device: the scene as it is (frames queued before are drawn and dropped)"""
        self.snapshot()
        return self.flush()[-1]

    def save(self, path: str, quality: int = 90, encoder: str = "pil"):
        save_image(self.frame(), path, quality, encoder=encoder, engine=self.E)


ENCODERS = ("pil", "gpu")


def save_image(img: torch.Tensor, path: str, quality: int = 90, encoder: str = "pil", engine: Optional[Engine] = None):
    """one uint8 [H, W, 3] image as a file.  ``encoder="pil"``: PIL on the host, whatever format the path names;
    ``"gpu"``: a JPEG encoded where the pixels are (``jpeg.save_jpeg``, on ``engine`` or the product's)"""
    if encoder not in ENCODERS:
        raise ValueError(f"save_image: encoder must be 'pil' or 'gpu' (got {encoder!r})")
    if encoder == "gpu":
        from .jpeg import save_jpeg
        save_jpeg(img, path, quality=quality, engine=engine)
        return
    from PIL import Image
    Image.fromarray(img.cpu().numpy()).save(path, quality=quality)


# --------------------------------------------------------------------------------------------------
# the command (visualizer.py)
# --------------------------------------------------------------------------------------------------
def config_scale(path: str) -> float:
    """``scale`` of a run's YAML config, looked up along its ``inherit_from`` chain (src/config.py:10-41); 1 when no file of the
    chain sets it, the default of configs/nice_slam.yaml"""
    import yaml
    seen = set()
    while path is not None and path not in seen:
        seen.add(path)
        with open(path) as fh:
            cfg = yaml.full_load(fh) or {}
        if "scale" in cfg:
            return float(cfg["scale"])
        nxt = cfg.get("inherit_from")
        if nxt is not None and not os.path.exists(nxt):             # the chain names paths relative to the reference's root
            d = os.path.dirname(os.path.abspath(path))
            while d != os.path.dirname(d) and not os.path.exists(os.path.join(d, nxt)):
                d = os.path.dirname(d)
            nxt = os.path.join(d, nxt)
        path = nxt
    return 1.0


def load_run(output: str, scale: float):
    """(estimate_c2w_list, gt_c2w_list fp64 [n, 4, 4], idx) of the newest checkpoint of a run directory, translations divided by
    ``scale`` (visualizer.py:44-58)"""
    ckpts = sorted(glob.glob(os.path.join(output, "ckpts", "*.tar")))
    if not ckpts:
        raise FileNotFoundError(f"no checkpoint under {os.path.join(output, 'ckpts')}")
    print("Get ckpt :", ckpts[-1])
    try:
        ckpt = torch.load(ckpts[-1], map_location="cpu", weights_only=True)
    except Exception:                                                # checkpoints of the reference hold more than tensors
        ckpt = torch.load(ckpts[-1], map_location="cpu", weights_only=False)
    est = np.array(to_numpy(ckpt["estimate_c2w_list"]), np.float64)
    gt = np.array(to_numpy(ckpt["gt_c2w_list"]), np.float64)
    est[:, :3, 3] /= scale
    gt[:, :3, 3] /= scale
    return est, gt, int(ckpt["idx"])


def replay_run(output: str, scale: float = 1.0, no_gt_traj: bool = False, width=WIDTH, height=HEIGHT, view="first", every=1,
               engine: Optional[Engine] = None, encoder: str = "pil", video: Optional[str] = None) -> int:
    """Replay the run in ``output`` as visualizer.py:60-91 walks it -- the newest mesh when ``mesh/{i:05d}_mesh.ply`` exists, both
    poses every frame, the trajectories every 10th -- and write every ``every``-th frame to ``tmp_rendering/{n:06d}.jpg`` (n from
    1).  ``encoder="gpu"``: every flushed batch is encoded by one ``jpeg.encode_jpeg`` call and the files are its streams;
    ``video``: a file name under ``output`` (``vis.avi``) that receives the same streams as a Motion-JPEG video at 30 frames/s
    (it implies the GPU encoder).  Returns the number of images written."""
    if encoder not in ENCODERS:
        raise ValueError(f"replay_run: encoder must be 'pil' or 'gpu' (got {encoder!r})")
    if video is not None:
        encoder = "gpu"
    est, gt, N = load_run(output, scale)
    replay = Replay(est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, width=width, height=height, view=view, engine=engine)
    out_dir = os.path.join(output, "tmp_rendering")
    os.makedirs(out_dir, exist_ok=True)
    for old in glob.glob(os.path.join(out_dir, "*.jpg")):
        os.remove(old)
    written = 0
    writer = None
    if video is not None:
        from .jpeg import MjpegWriter
        writer = MjpegWriter(os.path.join(output, video), width, height, fps=30)

    def write():
        nonlocal written
        if encoder == "gpu":
            from .jpeg import encode_jpeg
            frames = replay.flush()
            for data in (encode_jpeg(frames, quality=90, engine=replay.E) if len(frames) else []):
                written += 1
                with open(os.path.join(out_dir, f"{written:06d}.jpg"), "wb") as fh:
                    fh.write(data)
                if writer is not None:
                    writer.write(data)
            return
        for img in replay.flush().cpu().numpy():
            written += 1
            from PIL import Image
            Image.fromarray(img).save(os.path.join(out_dir, f"{written:06d}.jpg"), quality=90)

    queued = 0
    for i in range(0, N + 1):
        meshfile = os.path.join(output, "mesh", f"{i:05d}_mesh.ply")
        if os.path.isfile(meshfile):
            replay.update_mesh(meshfile)
        replay.update_pose(1, est[i], gt=False)
        if not no_gt_traj:
            replay.update_pose(1, gt[i], gt=True)
        if i % 10 == 0:
            replay.update_cam_trajectory(i, gt=False)
            if not no_gt_traj:
                replay.update_cam_trajectory(i, gt=True)
        if i % int(every) == 0:
            replay.snapshot()
            queued += 1
            if queued % FRAMES_PER_LAUNCH == 0:
                write()
    try:
        write()
    finally:
        if writer is not None:
            writer.close()
    return written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nice_slam_amd.viewer",
                                 description="Replay a finished SLAM run headless: shaded mesh, cameras and trajectories as numbered JPEGs.")
    ap.add_argument("--output", required=True, help="the run's output folder (ckpts/*.tar, mesh/*_mesh.ply)")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--scale", type=float, default=None, help="the run's scale (translations are divided by it); default 1")
    g.add_argument("--config", type=str, default=None, help="the run's YAML config: scale is read from it, following inherit_from")
    ap.add_argument("--no_gt_traj", action="store_true", help="do not draw the ground-truth camera and trajectory")
    ap.add_argument("--size", type=str, default=f"{WIDTH}x{HEIGHT}", help="image size WxH, at most 1024 a side")
    ap.add_argument("--view", choices=("first", "follow"), default="first", help="fixed viewer behind the first pose, or behind each pose")
    ap.add_argument("--every", type=int, default=1, help="write every N-th frame")
    ap.add_argument("--encoder", choices=ENCODERS, default="pil", help="who encodes the JPEGs: PIL on the host, or the GPU (a batch per call)")
    ap.add_argument("--video", nargs="?", const="vis.avi", default=None, metavar="NAME",
                    help="also write the frames as a Motion-JPEG video OUTPUT/NAME (default vis.avi) at 30 frames/s; implies --encoder gpu")
    args = ap.parse_args(argv)
    try:
        width, height = (int(x) for x in args.size.lower().split("x"))
    except ValueError:
        ap.error(f"--size must be WxH (got {args.size!r})")
    if args.every < 1:
        ap.error("--every must be positive")
    scale = config_scale(args.config) if args.config else (1.0 if args.scale is None else args.scale)
    n = replay_run(args.output, scale, args.no_gt_traj, width, height, args.view, args.every, encoder=args.encoder, video=args.video)
    print(f"wrote {n} images to {os.path.join(args.output, 'tmp_rendering')}")
    if args.video is not None:
        print(f"wrote {n} frames to {os.path.join(args.output, args.video)}")
        return 0
    print(f"ffmpeg -f image2 -r 30 -pattern_type glob -i '{args.output}/tmp_rendering/*.jpg' -y {args.output}/vis.mp4")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
