"""Mesh extraction on the GPU: a drop-in for the reference's ``src.utils.Mesher.Mesher`` (src/utils/Mesher.py).

    from nice_slam_amd import Mesher, marching_cubes

Every per-point and per-cell loop runs in libnsr.so (include/nsr.h, "Mesh extraction"): the lattice query
(nsr_eval_points_fwd), the seen / forecast / unseen classification (nsr_point_masks), marching cubes (nsr_mc_count /
nsr_mc_emit), face areas and the union-find over faces that share an edge (nsr_face_areas, nsr_cc_*, nsr_segment_sums).
torch does the plumbing: lattice coordinates, boolean indexing, sorting edge keys, compaction.

Deviations from the reference (also in INTEGRATION.md):
  * ``get_bound_from_frames`` (:214-279) raises NotImplementedError; ``bound_from_frames`` (nice_slam_amd/bound.py) builds the
    same hull on the GPU and returns a ``ConvexBound``.  ``get_mesh(..., mesh_bound=...)`` takes: None (everything is
    inside), "frames" (the bound of ``keyframe_dict``, built on the GPU: the reference's default), a ``ConvexBound`` (tested on
    the device), or a callable ``contains(np.ndarray [N,3]) -> bool [N]``, e.g. the ``contains`` of a user's trimesh hull.
  * ``color_mesh_extraction_method == 'render_ray_along_normal'`` is iMAP* only and raises NotImplementedError.
  * The marching-cubes table is this project's own (crack-free, tests/mesh_reference.py); vertex and face order follow the
    lattice, not skimage's, and the kept faces keep their order (trimesh regroups them by component).  No vertices are
    merged before export: coincident vertices arise only where a lattice value equals the level exactly.
  * ``get_mesh`` also returns the device tensors (vertices / scale fp64, faces int32, colours uint8 or None).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import _capi
from .bound import ConvexBound, bound_from_frames
from .common import _require_cuda
from .engine import Engine, c_doubles, compact, on, w2c_rows
from .ply import read_mesh, write_ply
from .renderer import eval_points_raw


def _engine(engine: Optional[Engine], t: torch.Tensor, what: str) -> Engine:
    """the caller's engine, else the product library on the GPU ``t`` lives on"""
    if engine is not None:
        return engine
    _require_cuda(t, what)
    return on(t.device)


def marching_cubes(volume: torch.Tensor, level: float = 0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0),
                   engine: Optional[Engine] = None):
    """Welded marching cubes of a device fp32 lattice ``volume[nx, ny, nz]`` (x slowest) -> (verts fp64 [V,3], faces int32
    [F,3]) on the device.  Vertex = origin + (i + t) * spacing; face normals point toward decreasing field (skimage's
    ``gradient_direction='descent'``).  One host read (the two counts) sizes the outputs."""
    E = _engine(engine, volume, "marching_cubes: volume")
    if volume.dim() != 3:
        raise ValueError("marching_cubes: volume must be [nx, ny, nz]")
    lib, dev = E.lib, E.device
    vol = volume.detach().to(dev, torch.float32).contiguous()
    nx, ny, nz = (int(s) for s in vol.shape)
    with torch.no_grad(), E.guard():
        nbytes = lib.nsr_mc_workspace_bytes(nx, ny, nz)
        if nbytes < 0:
            raise _capi.NsrError(f"marching_cubes: lattice {tuple(vol.shape)} not supported (every dimension >= 2, <= 2^31 points)")
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        E.call("nsr_mc_count", vol.data_ptr(), nx, ny, nz, float(level), ws.data_ptr(), counts.data_ptr())
        n_v, n_f = (int(x) for x in counts.cpu())
        verts = torch.empty((n_v, 3), dtype=torch.float64, device=dev)
        faces = torch.empty((n_f, 3), dtype=torch.int32, device=dev)
        E.call("nsr_mc_emit", vol.data_ptr(), nx, ny, nz, float(level), c_doubles(origin, 3), c_doubles(spacing, 3), ws.data_ptr(), n_v,
               n_f, verts.data_ptr(), faces.data_ptr())
    return verts, faces


def point_masks_raw(points: torch.Tensor, c2ws, depths, H, W, fx, fy, cx, cy, mode: int, chunk: int,
                    engine: Optional[Engine] = None) -> torch.Tensor:
    """uint8 [N] on the device: 0 unseen, 1 seen, 2 forecast (nsr_point_masks).  ``c2ws``: list of 4x4 poses (tensors or
    arrays); ``depths``: list of [H,W] depth tensors (modes 1, 2)."""
    E = _engine(engine, points, "point_masks: points")
    lib, dev = E.lib, E.device
    pts = points.detach().to(dev, torch.float32).contiguous()
    n = pts.shape[0]
    K = len(c2ws)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    if n == 0:
        return out
    w2c_d = torch.from_numpy(w2c_rows(c2ws, None)).to(dev)
    depth = limit = ws = None
    if mode == 2 and K:
        depth = torch.stack([d.detach().to(dev, torch.float32).reshape(H, W) for d in depths]).contiguous()
        ws = torch.empty(int(lib.nsr_point_masks_workspace_floats(n, chunk, K)), dtype=torch.float32, device=dev)
    elif mode == 1 and K:
        limit = torch.stack([torch.max(d.detach().to(dev, torch.float32)) * 1.1 for d in depths]).contiguous()   # :179
    with E.guard():
        E.call("nsr_point_masks", pts.data_ptr(), n, int(chunk), int(mode), K, w2c_d.data_ptr(),
               None if depth is None else depth.data_ptr(), None if limit is None else limit.data_ptr(), int(H), int(W), float(fx),
               float(fy), float(cx), float(cy), None if ws is None else ws.data_ptr(), out.data_ptr())
    return out


def face_adjacency(faces: torch.Tensor, n_verts: int) -> torch.Tensor:
    """int32 [P,2] pairs of faces that share an edge (trimesh's face_adjacency; a shared vertex alone does not count):
    edge keys sorted stably, neighbours with equal keys paired."""
    F = faces.shape[0]
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = torch.minimum(e[:, 0], e[:, 1]) * max(int(n_verts), 1) + torch.maximum(e[:, 0], e[:, 1])
    fid = torch.arange(F, device=faces.device).repeat(3)
    ks, order = torch.sort(key, stable=True)
    fs = fid[order]
    same = ks[1:] == ks[:-1]
    return torch.stack([fs[:-1][same], fs[1:][same]], 1).to(torch.int32).contiguous()


def face_components(verts: torch.Tensor, faces: torch.Tensor, engine: Optional[Engine] = None):
    """(label int64 [F] = the largest face index of the face's component, component areas fp64 [C], first (smallest) face of
    each component int64 [C], component index of each face int64 [F]); components in order of their label."""
    F = faces.shape[0]
    if F == 0:
        z = torch.zeros(0, dtype=torch.int64, device=faces.device)
        return z, torch.zeros(0, dtype=torch.float64, device=faces.device), z, z
    E = _engine(engine, faces, "face_components: faces")
    dev = E.device
    vv = verts.detach().to(dev, torch.float64).contiguous()
    ff = faces.to(dev, torch.int32).contiguous()
    pairs = face_adjacency(ff, vv.shape[0])
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    with E.guard():
        E.call("nsr_cc_init", F, parent.data_ptr(), changed.data_ptr())
        r = 0
        while True:
            E.call("nsr_cc_round", pairs.data_ptr(), pairs.shape[0], F, parent.data_ptr(), changed.data_ptr(), r)
            if int(changed.item()) != r + 1:
                break
            r += 1
        area = torch.empty(F, dtype=torch.float64, device=dev)
        E.call("nsr_face_areas", vv.data_ptr(), ff.data_ptr(), F, area.data_ptr())
        label = parent.long()
        ls, order = torch.sort(label, stable=True)
        start = torch.ones(F, dtype=torch.bool, device=dev)
        start[1:] = ls[1:] != ls[:-1]
        seg = torch.cat([torch.nonzero(start).reshape(-1), torch.tensor([F], device=dev)]).contiguous()
        n_seg = seg.shape[0] - 1
        comp_area = torch.empty(n_seg, dtype=torch.float64, device=dev)
        order, ls = order.contiguous(), ls.contiguous()
        partial = torch.empty(F, dtype=torch.float64, device=dev)
        E.call("nsr_segment_sums", area.data_ptr(), order.data_ptr(), ls.data_ptr(), F, seg.data_ptr(), n_seg, partial.data_ptr(),
               comp_area.data_ptr())
    comp_of = torch.empty(F, dtype=torch.int64, device=dev)
    comp_of[order] = torch.cumsum(start.long(), 0) - 1
    first = order[seg[:-1]]
    return label, comp_area, first, comp_of


def keep_components(verts: torch.Tensor, faces: torch.Tensor, largest: bool, min_area: float, engine: Optional[Engine] = None):
    """Mesher.py:487-498: keep the component of largest area (ties: the one whose first face comes first), or every component
    of area > min_area; then drop unreferenced vertices.  Faces and vertices keep their order."""
    _, comp_area, first, comp_of = face_components(verts, faces, engine)
    if faces.shape[0] == 0:
        return verts[:0], faces
    if largest:
        best = comp_area == comp_area.max()
        cand = torch.where(best, first, torch.full_like(first, faces.shape[0]))
        keep_comp = torch.zeros_like(best)
        keep_comp[torch.argmin(cand)] = True
    else:
        keep_comp = comp_area > min_area
    return compact(verts, faces[keep_comp[comp_of]])


def read_ply(path: str):
    """What write_ply writes -> (verts float32 [V,3], faces int32 [F,3], colors uint8 [V,4] or None): read_mesh with the
    colours, in write_ply's dtypes."""
    v, f, c = read_mesh(path, colors=True)
    return v.astype(np.float32), f.astype(np.int32), c


class Mesher:
    """src/utils/Mesher.py:11-574 with the same constructor and get_mesh call.  ``args`` is not used (the reference reads the
    dataset only for its length); ``slam`` provides renderer, bound, nice, verbose, H, W, fx, fy, cx, cy."""

    def __init__(self, cfg, args, slam, points_batch_size=500000, ray_batch_size=100000):
        self.points_batch_size = points_batch_size
        self.ray_batch_size = ray_batch_size
        self.renderer = slam.renderer
        self.coarse = cfg["coarse"]
        self.scale = cfg["scale"]
        self.occupancy = cfg["occupancy"]
        m = cfg["meshing"]
        self.resolution = m["resolution"]
        self.level_set = m["level_set"]
        self.clean_mesh_bound_scale = m["clean_mesh_bound_scale"]
        self.remove_small_geometry_threshold = m["remove_small_geometry_threshold"]
        self.color_mesh_extraction_method = m["color_mesh_extraction_method"]
        self.get_largest_components = m["get_largest_components"]
        self.depth_test = m["depth_test"]
        self.bound = slam.bound
        self.nice = slam.nice
        self.verbose = slam.verbose
        self.marching_cubes_bound = torch.from_numpy(np.array(cfg["mapping"]["marching_cubes_bound"]) * self.scale)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy

    # ---- the reference's methods ----
    def get_bound_from_frames(self, keyframe_dict, scale=1):
        raise NotImplementedError("Mesher.get_bound_from_frames needs Open3D's TSDF fusion and convex hull; use "
                                  "Mesher.bound_from_frames (the same bound, built on the GPU) or get_mesh(..., mesh_bound=\"frames\")")

    def bound_from_frames(self, keyframe_dict, scale=1):
        """Mesher.py:214-279 on the GPU (nice_slam_amd/bound.py) -> ConvexBound: the hull of the camera centres and the TSDF mesh
        vertices of the keyframes, scaled by meshing.clean_mesh_bound_scale about the mean of its vertices."""
        return bound_from_frames(keyframe_dict, self.H, self.W, self.fx, self.fy, self.cx, self.cy, scale, self.clean_mesh_bound_scale)

    @staticmethod
    def _inside(mesh_bound, points: torch.Tensor) -> torch.Tensor:
        """bool [N] on points' device: a ConvexBound runs on the device, a plain callable gets numpy slabs"""
        if isinstance(mesh_bound, ConvexBound):
            return mesh_bound.contains(points)
        return torch.from_numpy(np.asarray(mesh_bound(points.cpu().numpy()), dtype=bool)).to(points.device)

    def get_grid_uniform(self, resolution, device="cpu"):
        """Mesher.py:322-347: {"grid_points": fp32 [R^3,3] in np.meshgrid order (y slowest, then x, then z), "xyz": [x, y, z]}"""
        bound = self.marching_cubes_bound
        padding = 0.05
        xyz = [np.linspace(float(bound[i][0]) - padding, float(bound[i][1]) + padding, resolution) for i in range(3)]
        ax = [torch.from_numpy(a).to(device) for a in xyz]
        yy, xx, zz = torch.meshgrid(ax[1], ax[0], ax[2], indexing="ij")
        pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1).to(torch.float32)
        return {"grid_points": pts, "xyz": xyz}

    def eval_points(self, p, decoders, c=None, stage="color", device="cuda:0"):
        """Mesher.py:280-320 (occupancy := 100 outside self.bound), slab by slab of points_batch_size: the fp64 copy the
        library reads never exceeds one slab."""
        if not self.nice:
            raise NotImplementedError("Mesher.eval_points: iMAP* decoders are not supported")
        p = p.to(device)
        outs = [eval_points_raw(pi, decoders, c, stage, self.bound) for pi in torch.split(p, self.points_batch_size)]
        return torch.cat(outs, 0) if outs else torch.zeros((0, 4), dtype=torch.float32, device=device)

    def _mask_codes(self, points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames):
        pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.asarray(points))
        pts = pts.to(device).float()
        if get_mask_use_all_frames:
            c2ws, depths, mode = [estimate_c2w_list[i] for i in range(idx + 1)], [], 0
        else:
            c2ws = [kf["est_c2w"] for kf in keyframe_dict]
            depths = [kf["depth"] for kf in keyframe_dict]
            mode = 2 if self.depth_test else 1
        return point_masks_raw(pts, c2ws, depths, self.H, self.W, self.fx, self.fy, self.cx, self.cy, mode, self.points_batch_size)

    def point_masks(self, input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames=False):
        """Mesher.py:53-212 -> (seen, forecast, unseen) numpy bool arrays."""
        code = self._mask_codes(input_points, keyframe_dict, estimate_c2w_list, idx, device, get_mask_use_all_frames).cpu().numpy()
        return code == 1, code == 2, code == 0

    # ---- get_mesh ----
    def get_mesh(self, mesh_out_file, c, decoders, keyframe_dict, estimate_c2w_list, idx, device="cuda:0", show_forecast=False,
                 color=True, clean_mesh=True, get_mask_use_all_frames=False, mesh_bound: Optional[Callable] = None,
                 timer=None):
        """Mesher.py:349-574.  Writes a binary PLY and returns (vertices / scale fp64 [V,3], faces int32 [F,3], colours uint8
        [V,3] or None) on the device; None (and no file) when the level set has no surface.  ``mesh_bound`` replaces
        get_bound_from_frames (see the module docstring; "frames" builds it from keyframe_dict when a branch needs it).
        ``timer``: optional callable(phase_name) invoked after each phase (tools/mesh_timing.py)."""
        tick = timer or (lambda name: None)
        dev = torch.device(device)
        if isinstance(mesh_bound, str):
            if mesh_bound != "frames":
                raise ValueError(f"get_mesh: mesh_bound must be None, \"frames\", a ConvexBound or a callable (got {mesh_bound!r})")
            if show_forecast and not clean_mesh:
                mesh_bound = None                                          # no branch reads it
            else:
                mesh_bound = self.bound_from_frames(keyframe_dict, self.scale)
                tick("bound")
        with torch.no_grad():
            grid = self.get_grid_uniform(self.resolution, device=dev)
            points = grid["grid_points"]
            R = [len(a) for a in grid["xyz"]]
            if show_forecast:
                code = self._mask_codes(points, keyframe_dict, estimate_c2w_list, idx, dev, get_mask_use_all_frames)
                tick("masks")
                seen, fore = code == 1, code == 2
                z = torch.full((points.shape[0],), -100.0, dtype=torch.float32, device=dev)
                z[fore] = self.eval_points(points[fore], decoders, c, "coarse", dev)[:, -1] + 0.2
                z[seen] = self.eval_points(points[seen], decoders, c, "fine", dev)[:, -1]
            else:
                z = torch.cat([self.eval_points(pi, decoders, c, "fine", dev)[:, -1] for pi in torch.split(points, self.points_batch_size)])
                if mesh_bound is not None:
                    inside = torch.cat([self._inside(mesh_bound, pi) for pi in torch.split(points, self.points_batch_size)])
                    z[~inside] = 100.0
            tick("query")
            vol = z.reshape(R[1], R[0], R[2]).permute(1, 0, 2).contiguous()          # :440-441
            spacing = [a[2] - a[1] for a in grid["xyz"]]
            origin = [a[0] for a in grid["xyz"]]
            verts, faces = marching_cubes(vol, self.level_set, spacing, origin)
            tick("marching_cubes")
            if faces.shape[0] == 0:
                print("marching_cubes error. Possibly no surface extracted from the level set.")
                return None
            if clean_mesh:
                if show_forecast:
                    if mesh_bound is not None:
                        inside = self._inside(mesh_bound, verts)
                        faces = faces[~(~inside)[faces.long()].all(1)]
                else:
                    code = self._mask_codes(verts, keyframe_dict, estimate_c2w_list, idx, dev, get_mask_use_all_frames)
                    faces = faces[~(code != 1)[faces.long()].all(1)]
                verts, faces = keep_components(verts, faces, self.get_largest_components,
                                               self.remove_small_geometry_threshold * self.scale * self.scale)
            tick("clean")
            colors = None
            if color:
                if self.color_mesh_extraction_method != "direct_point_query":
                    raise NotImplementedError(f"Mesher: color_mesh_extraction_method '{self.color_mesh_extraction_method}' "
                                              "(iMAP* only) is not supported")
                rgb = self.eval_points(verts.float(), decoders, c, "color", dev)[:, :3]
                colors = (rgb.clamp(0, 1) * 255).to(torch.uint8)
                if show_forecast:
                    code = self._mask_codes(verts, keyframe_dict, estimate_c2w_list, idx, dev, get_mask_use_all_frames)
                    colors[code == 2] = torch.tensor([0, 255, 255], dtype=torch.uint8, device=dev)
            tick("colors")
            verts = verts / self.scale
            write_ply(mesh_out_file, verts.cpu().numpy(), faces.cpu().numpy(), None if colors is None else colors.cpu().numpy())
            tick("export")
            if self.verbose:
                print("Saved mesh at", mesh_out_file)
        return verts, faces, colors
