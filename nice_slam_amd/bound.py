"""The mesh bound from keyframes on the GPU: the reference's ``Mesher.get_bound_from_frames`` (src/utils/Mesher.py:214-279).

    from nice_slam_amd import bound_from_frames
    hull = bound_from_frames(keyframe_dict, H, W, fx, fy, cx, cy, scale=cfg["scale"], bound_scale=1.02)
    inside = hull.contains(points)          # numpy in -> numpy out, device tensor in -> device tensor out

Every per-voxel and per-point loop runs in libnsr.so (include/nsr.h, "Mesh bound from keyframes"; the rules are written out
in csrc/nsr_bound.h): TSDF fusion of the keyframes' depth as Open3D's ScalableTSDFVolume does it (nsr_tsdf_*), the vertex
set of that volume's mesh (nsr_tsdf_surface_*), a pre-filter that drops every point strictly inside the hull of 26 extreme
points (nsr_hull_extremes, nsr_hull_prefilter), and the point-in-hull test (nsr_hull_contains).  The exact hull of the
survivors is an fp64 quickhull run on the host inside the library (nsr_convex_hull).  torch does the plumbing.

Deviations from the reference (also in INTEGRATION.md):
  * no colour is fused: the hull reads nothing but positions;
  * the hull is this library's quickhull, not Qhull; a point on the boundary counts as inside (trimesh's ray-parity
    ``contains`` leaves that case undefined).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, c_doubles, c_int32s, gpu, on, pose_stack, w2c_rows
from .ply import write_ply

UNIT = 16                        # voxels per unit edge (Open3D's volume_unit_resolution)
HULL_TOL_REL = 1e-14             # quickhull distance tolerance, relative to the sum over axes of the largest |coordinate|
PREFILTER_MARGIN_REL = 1e-9      # a point is dropped only if it lies this far inside every plane of the extremes' hull


def frame_poses(c2ws):
    """(c2w fp64 [K,12], w2c fp32 [K,12], camera centres fp64 [K,3]) from the keyframes' est_c2w, flipped to Open3D's
    convention as Mesher.py:240-243 does; w2c = inv(c2w) in fp64, then rounded to fp32."""
    c2w = pose_stack(c2ws, flip_yz=True)
    return np.ascontiguousarray(c2w[:, :3]).reshape(len(c2w), 12), w2c_rows(c2w, np.float64), c2w[:, :3, 3].copy()


class TSDFVolume:
    """The fused volume on the device: ``units`` int32 [U,3] (unit indices, linear-index order), ``touch`` uint32
    [U,(K+31)//32] (bit k: frame k touched the unit), ``tsdf`` / ``weight`` fp32 [U,16,16,16] (x slowest); ``box`` the
    host copy of the unit box, ``workspace`` the unit bitmap and its rank (read by surface_points)."""

    def __init__(self, engine, box, workspace, units, touch, tsdf, weight, voxel_length, sdf_trunc, cams):
        self.engine, self.box, self.workspace = engine, box, workspace
        self.units, self.touch, self.tsdf, self.weight = units, touch, tsdf, weight
        self.voxel_length, self.sdf_trunc, self.cams = voxel_length, sdf_trunc, cams


def tsdf_fuse(keyframes, H, W, fx, fy, cx, cy, scale=1.0, engine: Optional[Engine] = None, timer=None) -> TSDFVolume:
    """Fuse every keyframe's depth (``keyframe['depth']`` [H,W], ``keyframe['est_c2w']`` 4x4) into a sparse TSDF volume with
    voxel_length 4 scale / 512 and sdf_trunc 0.04 scale (Mesher.py:227-236).  ``timer``: optional callable(phase)."""
    E = engine or gpu()
    lib, dev = E.lib, E.device
    tick = timer or (lambda name: None)
    K = len(keyframes)
    if K == 0:
        raise ValueError("tsdf_fuse: no keyframes")
    vl, trunc = 4.0 * scale / 512.0, 0.04 * scale
    c2w, w2c, cams = frame_poses([kf["est_c2w"] for kf in keyframes])
    with torch.no_grad(), E.guard():
        depth = torch.stack([torch.as_tensor(kf["depth"]).detach().to(dev, torch.float32).reshape(H, W) for kf in keyframes]).contiguous()
        c2w_d = torch.from_numpy(c2w).to(dev)
        w2c_d = torch.from_numpy(w2c).to(dev)
        args = (depth.data_ptr(), K, int(H), int(W), c2w_d.data_ptr(), float(fx), float(fy), float(cx), float(cy), vl, trunc)
        box_d = torch.empty(6, dtype=torch.int32, device=dev)
        E.call("nsr_tsdf_unit_box", *args, box_d.data_ptr())
        box = box_d.cpu().numpy()
        tw = (K + 31) // 32
        if box[3] < box[0]:                                           # no valid depth in any keyframe
            z = torch.zeros((0, UNIT, UNIT, UNIT), dtype=torch.float32, device=dev)
            return TSDFVolume(E, box, None, torch.zeros((0, 3), dtype=torch.int32, device=dev),
                              torch.zeros((0, tw), dtype=torch.int32, device=dev), z, z.clone(), vl, trunc, cams)
        nbytes = lib.nsr_tsdf_workspace_bytes(c_int32s(box))
        if nbytes < 0:
            raise _capi.NsrError(f"tsdf_fuse: the touched units span {box[3:] - box[:3] + 1} units: more than 2^31")
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        nu_d = torch.empty(1, dtype=torch.int64, device=dev)
        E.call("nsr_tsdf_touch_count", *args, c_int32s(box), ws.data_ptr(), nu_d.data_ptr())
        nu = int(nu_d.cpu()[0])
        units = torch.empty((nu, 3), dtype=torch.int32, device=dev)
        touch = torch.empty((nu, tw), dtype=torch.int32, device=dev)     # uint32 bits (torch has no uint32 arithmetic)
        E.call("nsr_tsdf_touch_emit", *args, c_int32s(box), ws.data_ptr(), nu, units.data_ptr(), touch.data_ptr())
        tick("touch")
        tsdf = torch.empty((nu, UNIT, UNIT, UNIT), dtype=torch.float32, device=dev)
        weight = torch.empty_like(tsdf)
        E.call("nsr_tsdf_integrate", depth.data_ptr(), K, int(H), int(W), w2c_d.data_ptr(), float(fx), float(fy), float(cx), float(cy), vl,
               trunc, units.data_ptr(), touch.data_ptr(), nu, tsdf.data_ptr(), weight.data_ptr())
        tick("integrate")
    return TSDFVolume(E, box, ws, units, touch, tsdf, weight, vl, trunc, cams)


def surface_points(vol: TSDFVolume) -> torch.Tensor:
    """fp64 [N,3] on the volume's device: the vertex set of the volume's extract_triangle_mesh (csrc/nsr_bound.h: a point on
    every sign-changing voxel edge of a cube whose 8 corners have weight > 0), units in list order, voxels x-slowest, axes
    x, y, z."""
    E = vol.engine
    dev = E.device
    nu = vol.units.shape[0]
    if nu == 0:
        return torch.zeros((0, 3), dtype=torch.float64, device=dev)
    with torch.no_grad(), E.guard():
        counts = torch.empty(nu + 1, dtype=torch.int64, device=dev)
        E.call("nsr_tsdf_surface_count", c_int32s(vol.box), vol.workspace.data_ptr(), vol.units.data_ptr(), nu, vol.tsdf.data_ptr(),
               vol.weight.data_ptr(), counts.data_ptr())
        n = int(counts[nu].cpu())
        pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
        E.call("nsr_tsdf_surface_emit", c_int32s(vol.box), vol.workspace.data_ptr(), vol.units.data_ptr(), nu, vol.tsdf.data_ptr(),
               vol.weight.data_ptr(), float(vol.voxel_length), counts.data_ptr(), n, pts.data_ptr())
    return pts


def _tol_scale(p: np.ndarray) -> float:
    return float(np.abs(p).max(0).sum()) if len(p) else 0.0


def convex_hull(points, bound_scale=1.0, tol=None, lib=None):
    """Exact fp64 quickhull of host points [N,3] (nsr_convex_hull), scaled by ``bound_scale`` about the mean of its vertices
    -> (vertices fp64 [V,3], vertex_index int64 [V] into points (ascending), faces int32 [F,3] outward, planes fp64 [F,4]
    (unit normal, offset) of the scaled faces)."""
    lib = lib or gpu().lib
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    n = len(p)
    if tol is None:
        tol = HULL_TOL_REL * _tol_scale(p)
    counts = np.zeros(2, np.int64)
    verts = np.zeros((max(n, 1), 3), np.float64)
    vidx = np.zeros(max(n, 1), np.int64)
    faces = np.zeros((max(2 * n, 1), 3), np.int32)
    planes = np.zeros((max(2 * n, 1), 4), np.float64)
    lib.call("nsr_convex_hull", p.ctypes, n, float(tol), float(bound_scale), counts.ctypes, verts.ctypes, vidx.ctypes, faces.ctypes,
             planes.ctypes)
    nv, nf = int(counts[0]), int(counts[1])
    return verts[:nv].copy(), vidx[:nv].copy(), faces[:nf].copy(), planes[:nf].copy()


def prefilter(points: torch.Tensor, engine: Optional[Engine] = None) -> torch.Tensor:
    """The points that may be vertices of the convex hull of ``points`` (fp64 [N,3] on the engine's device), in their
    order: every point strictly inside the hull of the 26 extremes (csrc/nsr_bound.h) is dropped."""
    E = engine or gpu()
    lib, dev = E.lib, E.device
    pts = points.detach().to(dev, torch.float64).contiguous()
    n = pts.shape[0]
    if n < 5:
        return pts
    with torch.no_grad(), E.guard():
        partial = torch.empty(int(lib.nsr_hull_partial_doubles()), dtype=torch.float64, device=dev)
        ext = torch.empty(26, dtype=torch.int64, device=dev)
        E.call("nsr_hull_extremes", pts.data_ptr(), n, partial.data_ptr(), ext.data_ptr())
        idx = np.unique(ext.cpu().numpy())
        ep = pts[torch.from_numpy(idx).to(dev)].cpu().numpy()
        try:
            _, _, _, planes = convex_hull(ep, 1.0, HULL_TOL_REL * _tol_scale(ep), lib=lib)
        except _capi.NsrError:                                        # the extremes span no volume: nothing is strictly inside
            return pts
        margin = PREFILTER_MARGIN_REL * _tol_scale(ep)
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        E.call("nsr_hull_prefilter", pts.data_ptr(), n, c_doubles(planes), planes.shape[0], margin, keep.data_ptr())
    return pts[keep.bool()]


class ConvexBound:
    """The scaled convex hull: ``vertices`` fp64 [V,3], ``faces`` int32 [F,3] (outward), ``planes`` fp64 [F,4].  ``contains``
    (alias ``__call__``, so it fits ``Mesher.get_mesh(mesh_bound=...)``) runs on the device: a point is inside iff
    ((nx x + ny y) + nz z) + off <= 0 for every plane, in fp64 -- points on the boundary count as inside."""

    def __init__(self, vertices, faces, planes, engine: Optional[Engine] = None, stats=None):
        self.vertices = np.asarray(vertices, np.float64)
        self.faces = np.asarray(faces, np.int32)
        self.planes = np.asarray(planes, np.float64)
        self.engine = engine
        self.stats = dict(stats or {})
        self._dplanes = {}

    def _planes_on(self, dev):
        key = str(dev)
        if key not in self._dplanes:
            self._dplanes[key] = torch.from_numpy(np.ascontiguousarray(self.planes)).to(dev)
        return self._dplanes[key]

    def contains(self, points):
        """bool [N]: numpy in -> numpy out; a tensor in -> a tensor on its device out (fp32 or fp64 points, [N,3])."""
        as_np = not isinstance(points, torch.Tensor)
        E = self.engine or gpu()
        if not as_np and points.device.type == E.device.type and points.device != E.device:
            E = on(points.device)                                     # a tensor on another GPU is tested there
        t = E.tensor(np.reshape(points, (-1, 3)) if as_np else points.reshape(-1, 3), what="contains: points")
        n = t.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=E.device)
        if n:
            pl = self._planes_on(E.device)
            with torch.no_grad(), E.guard():
                E.call("nsr_hull_contains", t.data_ptr(), n, int(t.dtype == torch.float64), pl.data_ptr(), pl.shape[0], out.data_ptr())
        res = out.bool()
        return res.cpu().numpy() if as_np else res

    __call__ = contains

    def to_ply(self, path: str):
        write_ply(path, self.vertices, self.faces)


def bound_from_frames(keyframe_dict, H, W, fx, fy, cx, cy, scale=1.0, bound_scale=1.02, engine: Optional[Engine] = None,
                      timer=None) -> ConvexBound:
    """Mesher.get_bound_from_frames: the convex hull of the camera centres and the TSDF mesh vertices of the keyframes,
    scaled by ``bound_scale`` about the mean of its vertices.  ``stats`` of the result: the point counts of each stage."""
    E = engine or gpu()
    tick = timer or (lambda name: None)
    vol = tsdf_fuse(keyframe_dict, H, W, fx, fy, cx, cy, scale, engine=E, timer=tick)
    surf = surface_points(vol)
    tick("extract")
    cams = torch.from_numpy(vol.cams).to(E.device)
    pts = torch.cat([cams, surf], 0).contiguous()                      # Mesher.py:269: camera centres first
    cand = prefilter(pts, E)
    host = cand.cpu().numpy()
    tick("prefilter")
    verts, _, faces, planes = convex_hull(host, bound_scale, lib=E.lib)
    tick("hull")
    stats = {"units": int(vol.units.shape[0]), "surface_points": int(surf.shape[0]), "points": int(pts.shape[0]),
             "prefiltered": int(cand.shape[0]), "hull_vertices": int(len(verts)), "hull_faces": int(len(faces))}
    return ConvexBound(verts, faces, planes, engine=E, stats=stats)
