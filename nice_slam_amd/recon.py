"""Reconstruction evaluation on the GPU: a drop-in for the reference's ``src/tools/eval_recon.py`` (3-D metrics) and
``src/tools/cull_mesh.py``.

    from nice_slam_amd import recon
    recon.calc_3d_metric("rec.ply", "gt.ply")      # {accuracy_cm, completion_cm, completion_ratio_pct}
    recon.calc_2d_metric("rec.ply", "gt.ply")      # {depth_l1_cm, per_view}  (nice_slam_amd/raster.py)
    recon.calc_3d_metric("rec.ply", "gt.ply", surface="mesh")   # point-to-MESH distances: + precision / recall / F-score,
                                                                # normal consistency (surface_metrics; not the reference's metric)

    python -m nice_slam_amd.recon eval --rec_mesh R --gt_mesh G -3d [--surface mesh [--thresholds T ...] [--error_mesh OUT.ply]]
    python -m nice_slam_amd.recon depth --rec_mesh R --gt_mesh G
    python -m nice_slam_amd.recon cull --input_mesh M --traj traj.txt --output_mesh OUT [--occlusion]
    python -m nice_slam_amd.recon unseen --gt_mesh G --traj traj.txt --output G_pc_unseen.npy

Every per-point loop runs in libnsr.so (include/nsr.h, "Reconstruction evaluation"): exact nearest neighbour over a cell grid
(nsr_nn_*: the cKDTree queries), area-weighted surface sampling (nsr_sample_surface: trimesh.sample.sample_surface),
fixed-order fp64 reductions (nsr_dist_stats, nsr_icp_stats), the ICP point update (nsr_transform_points) and frustum culling
over a whole trajectory (nsr_cull_vertices).  torch does the plumbing: sorting cell keys, indexing, compaction; the host
does the 3x3 SVD of each ICP step and the 4x4 pose inverses.

Deviations from the reference (also in INTEGRATION.md):
  * the surface sampler is seeded (``seed``; the reference draws unseeded from numpy), so a metric is reproducible; trimesh's
    own random stream cannot be matched, only its algorithm;
  * ICP is Open3D's point-to-point ``registration_icp`` loop restated (the same correspondences, update and stopping rule),
    not Open3D itself: the transform agrees to rounding;
  * the 2-D depth metric (``calc_2d_metric``, ``render_depth``: nice_slam_amd/raster.py) renders with this library's tiled
    rasterizer, not Open3D's OpenGL depth buffer; its own deviations are listed in raster.py;
  * ``cull_mesh(occlusion=True)`` (``cull --occlusion``) also drops what the mesh itself hides from every camera, a test
    cull_mesh.py does not have; off by default.  ``unseen_points`` (``unseen``) makes the ``_pc_unseen.npy`` cloud of a ground
    truth, which the reference ships only for its own scenes;
  * ``surface="mesh"`` (``eval -3d --surface mesh``, ``surface_metrics``, ``MeshIndex``, ``error_mesh``) measures from each sample
    to the other MESH (nsr_meshdist_*: the exact point-to-triangle distance) instead of to the other sample cloud.  This is
    NOT the reference's metric: it has no sampling floor, so its accuracy and completion are smaller.  Opt-in; the default
    is the reference's estimator, unchanged.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from typing import Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, c_doubles, gpu, pose_stack, w2c_rows
from .engine import compact as compact_mesh
from .ply import read_mesh, write_ply

__all__ = ["nearest", "accuracy", "completion", "completion_ratio", "recon_metrics", "sample_surface", "align_icp",
           "calc_3d_metric", "cull_mesh", "load_poses", "read_mesh", "NNIndex",
           "render_depth", "depth_l1", "cam_position", "sample_views", "calc_2d_metric", "cull_masks", "visibility_counts",
           "unseen_points", "MeshIndex", "mesh_distance", "face_normals", "surface_metrics", "error_mesh"]


# --------------------------------------------------------------------------------------------------
# nearest neighbour
# --------------------------------------------------------------------------------------------------
def _grid_plan(E: Engine, pts: torch.Tensor, plan_entry: str, count: int):
    """the host's grid plan (``plan_entry``: nsr_nn_plan or nsr_meshdist_plan, for ``count`` entries) over the box of ``pts``"""
    bounds = torch.empty(6 * 257, dtype=torch.float64, device=E.device)
    E.call("nsr_nn_bounds", pts.data_ptr(), pts.shape[0], int(pts.dtype == torch.float64), bounds.data_ptr())
    plan = (C.c_double * 16)()
    E.lib.call(plan_entry, c_doubles(bounds[:6].cpu().numpy()), count, plan)
    return plan


def _query_tensor(E: Engine, q, who: str):
    """(``q`` as a finite [N, 3] tensor on the device, N, its fp64 flag)"""
    qt = E.tensor(q, what=f"{who}: query")
    if qt.shape[0] and not bool(torch.isfinite(qt).all()):
        raise ValueError(f"{who}: query coordinates must be finite")
    return qt, qt.shape[0], int(qt.dtype == torch.float64)


def _key_order(E: Engine, plan, qt: torch.Tensor, fp64: int) -> torch.Tensor:
    """the order that sorts the queries by their cell key, so that a wave's lanes walk neighbouring cells"""
    keys = torch.empty(qt.shape[0], dtype=torch.int64, device=E.device)
    E.call("nsr_nn_keys", qt.data_ptr(), qt.shape[0], fp64, plan, keys.data_ptr())
    return torch.sort(keys, stable=True)[1].contiguous()


class NNIndex:
    """Exact nearest-neighbour index over ``ref`` [M, 3] (fp32 or fp64): a uniform cell grid built on the device.
    ``query(q)`` -> (dist fp64 [N], idx int64 [N]) as ``scipy.spatial.cKDTree(ref).query(q)``; distances in fp64,
    ties to the smallest reference index."""

    def __init__(self, ref, engine: Optional[Engine] = None):
        E = self.engine = engine or gpu()
        lib = E.lib
        r = self.ref = E.tensor(ref, what="nearest: ref")
        M = self.m = r.shape[0]
        if M == 0:
            raise ValueError("nearest: the reference set is empty")
        self.fp64 = int(r.dtype == torch.float64)
        with torch.no_grad(), E.guard():
            self.plan = _grid_plan(E, r, "nsr_nn_plan", M)
            nbytes = lib.nsr_nn_workspace_bytes(self.plan, M)
            if nbytes < 0:
                raise _capi.NsrError("nearest: invalid grid plan")
            self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=E.device)
            keys = torch.empty(M, dtype=torch.int64, device=E.device)
            E.call("nsr_nn_keys", r.data_ptr(), M, self.fp64, self.plan, keys.data_ptr())
            sk, order = torch.sort(keys, stable=True)
            E.call("nsr_nn_build", r.data_ptr(), M, self.fp64, self.plan, sk.data_ptr(), order.contiguous().data_ptr(), self.ws.data_ptr())

    def query(self, q, with_candidates: bool = False):
        E = self.engine
        qt, N, fp64 = _query_tensor(E, q, "nearest")
        dist = torch.empty(N, dtype=torch.float64, device=E.device)
        idx = torch.empty(N, dtype=torch.int64, device=E.device)
        ncand = torch.empty(N, dtype=torch.int32, device=E.device) if with_candidates else None
        if N:
            with torch.no_grad(), E.guard():
                qorder = _key_order(E, self.plan, qt, fp64)
                E.call("nsr_nn_query", qt.data_ptr(), N, fp64, qorder.data_ptr(), self.plan, self.ws.data_ptr(), self.m, dist.data_ptr(),
                       idx.data_ptr(), None if ncand is None else ncand.data_ptr())
        return (dist, idx, ncand) if with_candidates else (dist, idx)


def nearest(query, ref, engine: Optional[Engine] = None):
    """(dist fp64 [N], idx int64 [N]): for every query point its nearest point of ``ref`` (cKDTree(ref).query(query))."""
    return NNIndex(ref, engine).query(query)


# --------------------------------------------------------------------------------------------------
# metrics (eval_recon.py:24-43, :91-117)
# --------------------------------------------------------------------------------------------------
def _dist_stats(E: Engine, dist: torch.Tensor, th: float):
    lib = E.lib
    n = dist.shape[0]
    partial = torch.empty(int(lib.nsr_recon_partial_doubles(n)), dtype=torch.float64, device=E.device)
    out = torch.empty(2, dtype=torch.float64, device=E.device)
    with E.guard():
        E.call("nsr_dist_stats", dist.data_ptr(), n, float(th), partial.data_ptr(), out.data_ptr())
    s, c = (float(x) for x in out.cpu())
    return s, c


def _mean(E, dist):
    n = dist.shape[0]
    return _dist_stats(E, dist, 0.0)[0] / n if n else float("nan")


def accuracy(gt_points, rec_points, engine: Optional[Engine] = None) -> float:
    """Mean distance from each reconstructed point to the ground truth (eval_recon.py:32-36)."""
    E = engine or gpu()
    return _mean(E, nearest(rec_points, gt_points, E)[0])


def completion(gt_points, rec_points, engine: Optional[Engine] = None) -> float:
    """Mean distance from each ground-truth point to the reconstruction (eval_recon.py:39-43)."""
    E = engine or gpu()
    return _mean(E, nearest(gt_points, rec_points, E)[0])


def completion_ratio(gt_points, rec_points, dist_th=0.05, engine: Optional[Engine] = None) -> float:
    """Fraction of ground-truth points within ``dist_th`` of the reconstruction (eval_recon.py:24-29)."""
    E = engine or gpu()
    d = nearest(gt_points, rec_points, E)[0]
    return _dist_stats(E, d, dist_th)[1] / d.shape[0] if d.shape[0] else float("nan")


def recon_metrics(gt_points, rec_points, dist_th=0.05, engine: Optional[Engine] = None):
    """(accuracy, completion, completion_ratio) from two nearest-neighbour passes (the reference makes three)."""
    E = engine or gpu()
    d_acc = nearest(rec_points, gt_points, E)[0]
    d_comp = nearest(gt_points, rec_points, E)[0]
    n = d_comp.shape[0]
    s_comp, c_comp = _dist_stats(E, d_comp, dist_th)
    return _mean(E, d_acc), (s_comp / n if n else float("nan")), (c_comp / n if n else float("nan"))


# --------------------------------------------------------------------------------------------------
# surface sampling (trimesh.sample.sample_surface, eval_recon.py:103,106)
# --------------------------------------------------------------------------------------------------
def sample_surface(vertices, faces, count: int, seed: int = 0, uniforms=None, engine: Optional[Engine] = None):
    """(points fp64 [count, 3], face_index int64 [count]): ``count`` points on the mesh, faces picked in proportion to their
    area.  ``uniforms`` [count, 3] fp64 (u0, a, b) replaces the in-kernel philox draws keyed by ``seed``."""
    E = engine or gpu()
    lib = E.lib
    v = E.tensor(vertices, torch.float64, "sample_surface: vertices")
    f = E.faces(faces)
    n = int(count)
    pts = torch.empty((n, 3), dtype=torch.float64, device=E.device)
    fi = torch.empty(n, dtype=torch.int64, device=E.device)
    u = None
    if uniforms is not None:
        u = E.tensor(uniforms, torch.float64, "sample_surface: uniforms")
        if u.shape[0] != n:
            raise ValueError("sample_surface: uniforms must be [count, 3]")
    ws = torch.empty(int(lib.nsr_sample_workspace_bytes(f.shape[0])), dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_sample_surface", v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], n, None if u is None else u.data_ptr(),
               int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), pts.data_ptr(), fi.data_ptr())
    return pts, fi


# --------------------------------------------------------------------------------------------------
# ICP (eval_recon.py:45-59: Open3D registration_icp, point to point)
# --------------------------------------------------------------------------------------------------
def _umeyama(stats: np.ndarray) -> np.ndarray:
    """The rigid update of Open3D's TransformationEstimationPointToPoint (Eigen::umeyama without scaling) from the
    correspondence statistics of nsr_icp_stats; identity without correspondences."""
    T = np.eye(4)
    cnt = stats[0]
    if cnt <= 0:
        return T
    mu_s, mu_t = stats[2:5], stats[5:8]
    sigma = stats[8:17].reshape(3, 3) / cnt
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    T[:3, :3] = R
    T[:3, 3] = mu_t - R @ mu_s
    return T


def _icp(E: Engine, source, target, threshold=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    lib = E.lib
    index = NNIndex(target, E)
    tgt = index.ref if index.ref.dtype == torch.float64 else index.ref.double().contiguous()
    pcd = E.tensor(source, torch.float64, "align_icp: source").clone()
    n = pcd.shape[0]
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    if not np.array_equal(T, np.eye(4)):
        E.transform(pcd, T)
    partial = torch.empty(int(lib.nsr_recon_partial_doubles(n)), dtype=torch.float64, device=E.device)
    out = torch.empty(17, dtype=torch.float64, device=E.device)

    def evaluate():
        d, idx = index.query(pcd)
        with E.guard():
            E.call("nsr_icp_stats", pcd.data_ptr(), tgt.data_ptr(), idx.data_ptr(), d.data_ptr(), n, tgt.shape[0], float(threshold),
                   partial.data_ptr(), out.data_ptr())
        s = out.cpu().numpy().copy()
        fitness = s[0] / n if n else 0.0
        rmse = float(np.sqrt(s[1] / s[0])) if s[0] > 0 else 0.0
        return s, fitness, rmse

    stats, fitness, rmse = evaluate()
    it = 0
    while it < max_iteration:
        it += 1
        update = _umeyama(stats)
        T = update @ T
        E.transform(pcd, update)
        prev_f, prev_r = fitness, rmse
        stats, fitness, rmse = evaluate()
        if abs(prev_f - fitness) < relative_fitness and abs(prev_r - rmse) < relative_rmse:
            break
    return T, fitness, rmse, it


def align_icp(source, target, threshold=0.1, init=None, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
              engine: Optional[Engine] = None):
    """(T 4x4 fp64, fitness, inlier_rmse): point-to-point ICP of ``source`` onto ``target`` as Open3D's registration_icp
    (correspondences closer than ``threshold``, a rigid Umeyama update left-multiplied into T, stop when fitness and inlier
    RMSE both change by less than their tolerances, at most ``max_iteration`` updates)."""
    T, fitness, rmse, _ = _icp(engine or gpu(), source, target, threshold, init, max_iteration, relative_fitness, relative_rmse)
    return T, fitness, rmse


# --------------------------------------------------------------------------------------------------
# point-to-mesh distance (no counterpart in the reference: opt-in)
# --------------------------------------------------------------------------------------------------
class MeshIndex:
    """Exact point-to-triangle-mesh distance: a uniform cell grid over the box of ``vertices`` [V, 3] (fp32 or fp64) with every
    face of ``faces`` [F, 3] registered in the cells its box overlaps, built on the device without atomics.
    ``query(points)`` -> (dist fp64 [N], face int64 [N], closest fp64 [N, 3]): the minimum over ALL faces of the per-face
    distance (csrc/nsr_meshdist.h), in fp64, ties to the smallest face index; a degenerate face counts as its edges."""

    def __init__(self, vertices, faces, engine: Optional[Engine] = None):
        E = self.engine = engine or gpu()
        lib = E.lib
        v = self.vertices = E.tensor(vertices, what="mesh_distance: vertices")
        f = self.faces = E.faces(faces)
        V, F = v.shape[0], f.shape[0]
        if F == 0 or V == 0:
            raise ValueError("mesh_distance: the mesh has no faces")
        if not bool(torch.isfinite(v).all()):
            raise ValueError("mesh_distance: vertex coordinates must be finite")
        if int(f.min()) < 0 or int(f.max()) >= V:
            raise ValueError("mesh_distance: face index outside the vertex array")
        self.nf = F
        self.fp64 = int(v.dtype == torch.float64)
        mesh = (v.data_ptr(), V, self.fp64, f.data_ptr(), F)
        with torch.no_grad(), E.guard():
            self.plan = _grid_plan(E, v, "nsr_meshdist_plan", F)
            count = torch.empty(F, dtype=torch.int64, device=E.device)
            over = torch.empty(F, dtype=torch.int64, device=E.device)
            E.call("nsr_meshdist_count", *mesh, self.plan, count.data_ptr(), over.data_ptr())
            cum, ocum = torch.cumsum(count, 0), torch.cumsum(over, 0)
            self.npairs, self.nover = int(cum[-1]), int(ocum[-1])
            nbytes = lib.nsr_meshdist_workspace_bytes(self.plan, F, self.npairs, self.nover)
            if nbytes < 0:
                raise _capi.NsrError(f"mesh_distance: {self.npairs} (cell, face) pairs overflow the index's int32 tables")
            keys = torch.empty(self.npairs, dtype=torch.int64, device=E.device)
            pair_face = torch.empty(self.npairs, dtype=torch.int64, device=E.device)
            E.call("nsr_meshdist_fill", *mesh, self.plan, cum.data_ptr(), self.npairs, keys.data_ptr(), pair_face.data_ptr())
            sk, order = torch.sort(keys, stable=True)
            self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=E.device)
            E.call("nsr_meshdist_build", *mesh, self.plan, sk.data_ptr(), order.contiguous().data_ptr(), pair_face.data_ptr(), self.npairs,
                   over.data_ptr(), ocum.data_ptr(), self.nover, self.ws.data_ptr())

    def query(self, points, with_candidates: bool = False):
        """(dist, face, closest[, ncand int32 [N]: faces examined, repeats counted])"""
        E = self.engine
        qt, N, fp64 = _query_tensor(E, points, "mesh_distance")
        dist = torch.empty(N, dtype=torch.float64, device=E.device)
        face = torch.empty(N, dtype=torch.int64, device=E.device)
        closest = torch.empty((N, 3), dtype=torch.float64, device=E.device)
        ncand = torch.empty(N, dtype=torch.int32, device=E.device) if with_candidates else None
        if N:
            with torch.no_grad(), E.guard():
                qorder = _key_order(E, self.plan, qt, fp64)
                E.call("nsr_meshdist_query", qt.data_ptr(), N, fp64, qorder.data_ptr(), self.plan, self.ws.data_ptr(), self.nf, self.npairs,
                       self.nover, dist.data_ptr(), face.data_ptr(), closest.data_ptr(), None if ncand is None else ncand.data_ptr())
        return (dist, face, closest, ncand) if with_candidates else (dist, face, closest)


def mesh_distance(points, vertices, faces, engine: Optional[Engine] = None):
    """(dist fp64 [N], face int64 [N], closest fp64 [N, 3]): for every point the nearest point of the triangle mesh."""
    return MeshIndex(vertices, faces, engine).query(points)


def face_normals(vertices, faces, engine: Optional[Engine] = None) -> torch.Tensor:
    """Unit normals fp64 [F, 3] of the faces, (v1 - v0) x (v2 - v0) normalised; the zero vector for a degenerate face."""
    E = engine or gpu()
    v = E.tensor(vertices, what="face_normals: vertices")
    f = E.faces(faces)
    n = torch.empty((f.shape[0], 3), dtype=torch.float64, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_face_normals", v.data_ptr(), v.shape[0], int(v.dtype == torch.float64), f.data_ptr(), f.shape[0], n.data_ptr())
    return n


def _normal_stats(E: Engine, sample_normals: torch.Tensor, fnormals: torch.Tensor, face: torch.Tensor):
    """(sum of |n . m|, valid pairs) of the samples' normals against the normals of the faces the search returned"""
    n = face.shape[0]
    qn = sample_normals.contiguous()
    partial = torch.empty(int(E.lib.nsr_recon_partial_doubles(n)), dtype=torch.float64, device=E.device)
    out = torch.empty(2, dtype=torch.float64, device=E.device)
    with E.guard():
        E.call("nsr_normal_stats", qn.data_ptr(), fnormals.data_ptr(), face.data_ptr(), n, fnormals.shape[0], partial.data_ptr(), out.data_ptr())
    s, c = (float(x) for x in out.cpu())
    return s, c


def _aligned_meshes(E: Engine, rec_mesh, gt_mesh, align: bool):
    rv, rf = E.mesh(rec_mesh)
    gv, gf = E.mesh(gt_mesh)
    if align:
        T = align_icp(rv, gv, 0.1, engine=E)[0]
        rv = rv.clone()
        E.transform(rv, T)
    return rv, rf, gv, gf


def surface_metrics(rec_mesh, gt_mesh, align=True, n_points=200000, seed=0, thresholds=(0.05,), engine: Optional[Engine] = None):
    """The 3-D metrics with point-to-MESH distances: the ICP alignment and the seeded samples of ``calc_3d_metric``, but accuracy
    measures from each reconstruction sample to the ground-truth mesh and completion from each ground-truth sample to the
    reconstructed mesh, so the sampling spacing of the other surface does not enter.  NOT the reference's estimator.
    Returns accuracy_cm, completion_cm, chamfer_cm (their mean), completion_ratio_pct (at 0.05 m); per threshold t of
    ``thresholds`` [m] the dicts precision_pct[t] (reconstruction samples closer than t), recall_pct[t] (ground-truth samples
    closer than t) and fscore_pct[t] = 2PR / (P + R) (0 when P + R = 0); normal_consistency: the mean over the two directions of
    the mean |n . m| of a sample's face normal against the normal of its nearest face, and normal_pairs: the pairs that
    entered it (a pair with a degenerate face on either side does not)."""
    E = engine or gpu()
    rv, rf, gv, gf = _aligned_meshes(E, rec_mesh, gt_mesh, align)
    rec_pts, rec_fi = sample_surface(rv, rf, n_points, seed=seed, engine=E)
    gt_pts, gt_fi = sample_surface(gv, gf, n_points, seed=seed + 1, engine=E)
    d_acc, f_acc, _ = MeshIndex(gv, gf, E).query(rec_pts)
    d_comp, f_comp, _ = MeshIndex(rv, rf, E).query(gt_pts)
    n = int(n_points)
    acc, comp = _mean(E, d_acc), _mean(E, d_comp)
    out = {"accuracy_cm": acc * 100, "completion_cm": comp * 100, "chamfer_cm": (acc * 100 + comp * 100) / 2,
           "completion_ratio_pct": (_dist_stats(E, d_comp, 0.05)[1] / n if n else float("nan")) * 100,
           "precision_pct": {}, "recall_pct": {}, "fscore_pct": {}}
    for t in thresholds:
        t = float(t)
        p = (_dist_stats(E, d_acc, t)[1] / n if n else float("nan")) * 100
        r = (_dist_stats(E, d_comp, t)[1] / n if n else float("nan")) * 100
        out["precision_pct"][t], out["recall_pct"][t] = p, r
        out["fscore_pct"][t] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    rn, gn = face_normals(rv, rf, E), face_normals(gv, gf, E)
    s_a, c_a = _normal_stats(E, rn[rec_fi], gn, f_acc)
    s_c, c_c = _normal_stats(E, gn[gt_fi], rn, f_comp)
    means = [s / c for s, c in ((s_a, c_a), (s_c, c_c)) if c > 0]
    out["normal_consistency"] = sum(means) / len(means) if means else float("nan")
    out["normal_pairs"] = int(c_a + c_c)
    return out


def error_mesh(rec_mesh, gt_mesh, path: Optional[str] = None, vmax=0.05, align=False, engine: Optional[Engine] = None):
    """Distance fp64 [V] of every vertex of the reconstruction to the ground-truth MESH; with ``path`` the reconstruction is
    written there as a PLY whose vertices carry the distance through the figures' plasma map (0 -> its first entry, ``vmax``
    [m] and beyond -> its last).  ``align``: ICP-align the reconstruction first, as the metrics do."""
    from .imgeval import colorize_depth
    E = engine or gpu()
    rv, rf, gv, gf = _aligned_meshes(E, rec_mesh, gt_mesh, align)
    d = MeshIndex(gv, gf, E).query(rv)[0]
    if path is not None:
        rgb = colorize_depth(d.float().reshape(1, -1), vmax=float(vmax), engine=E)[0] if d.shape[0] else torch.empty((0, 3), dtype=torch.uint8)
        write_ply(path, rv.cpu().numpy(), rf.cpu().numpy(), colors=rgb.cpu().numpy())
    return d


# --------------------------------------------------------------------------------------------------
# the 3-D metric (eval_recon.py:91-117)
# --------------------------------------------------------------------------------------------------
def calc_3d_metric(rec_mesh, gt_mesh, align=True, n_points=200000, seed=0, engine: Optional[Engine] = None, surface="points",
                   thresholds=(0.05,)):
    """Accuracy [cm], completion [cm] and completion ratio [%] of a reconstructed mesh against the ground truth, as
    eval_recon.py's calc_3d_metric: (optionally) ICP-align the reconstruction's vertices to the ground truth's, sample
    ``n_points`` on each surface, then two nearest-neighbour passes.  Meshes: PLY paths or (vertices, faces) pairs (e.g. the
    device tensors ``Mesher.get_mesh`` returns).  The samplers are seeded (``seed`` for the reconstruction, ``seed + 1`` for
    the ground truth).  ``surface="mesh"``: the point-to-mesh estimator instead, ``surface_metrics``' dict (``thresholds`` goes
    there); not the reference's metric."""
    if surface == "mesh":
        return surface_metrics(rec_mesh, gt_mesh, align=align, n_points=n_points, seed=seed, thresholds=thresholds, engine=engine)
    if surface != "points":
        raise ValueError(f"calc_3d_metric: surface must be 'points' or 'mesh' (got {surface!r})")
    E = engine or gpu()
    rv, rf = E.mesh(rec_mesh)
    gv, gf = E.mesh(gt_mesh)
    if align:
        T = align_icp(rv, gv, 0.1, engine=E)[0]
        rv = rv.clone()
        E.transform(rv, T)
    rec_pts = sample_surface(rv, rf, n_points, seed=seed, engine=E)[0]
    gt_pts = sample_surface(gv, gf, n_points, seed=seed + 1, engine=E)[0]
    acc, comp, ratio = recon_metrics(gt_pts, rec_pts, 0.05, E)
    return {"accuracy_cm": acc * 100, "completion_cm": comp * 100, "completion_ratio_pct": ratio * 100}


# --------------------------------------------------------------------------------------------------
# culling (cull_mesh.py)
# --------------------------------------------------------------------------------------------------
def load_poses(path):
    """cull_mesh.py:9-19: one row-major 4x4 c2w per line, the y and z axes flipped, as float32 tensors."""
    poses = []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            c2w = np.array(list(map(float, line.split()))).reshape(4, 4)
            c2w[:3, 1] *= -1
            c2w[:3, 2] *= -1
            poses.append(torch.from_numpy(c2w).float())
    return poses


def _w2c_rows(c2w_list) -> np.ndarray:
    """[K, 12] fp32: rows 0..2 of np.linalg.inv of each pose AS FLOAT32, which is what cull_mesh.py:49 computes (its poses are
    float32 tensors, so numpy inverts in single precision)."""
    return w2c_rows(c2w_list, np.float32)


def cull_masks(vertices, faces, c2w_list, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, engine: Optional[Engine] = None, *,
               occlusion=False, eps=0.03, min_views=1, stride=1):
    """(seen bool [V], keep bool [F]): vertices some pose sees, faces with at least one seen vertex (cull_mesh.py:45-75).
    ``occlusion=True``: a vertex is seen by a pose only if it also is at most ``eps`` behind the depth of the mesh itself
    rendered from that pose (raster.visibility_counts), and seen at all if at least ``min_views`` of every ``stride``-th pose
    see it.  The poses are those ``load_poses`` returns (y and z axes flipped) either way."""
    E = engine or gpu()
    v = E.tensor(vertices, what="cull_mesh: vertices")
    f = E.faces(faces)
    if occlusion:
        c2w = pose_stack(list(c2w_list)[::int(stride)], flip_yz=True)       # back to the rasterizer's OpenCV convention
        count = visibility_counts(v, v, f, c2w, H, W, fx, fy, cx, cy, eps=eps, engine=E)
        seen = count >= int(min_views)
        return seen, seen[f.long()].any(1)
    K = len(c2w_list)
    w2c = torch.from_numpy(_w2c_rows(c2w_list)).to(E.device)
    seen = torch.empty(v.shape[0], dtype=torch.uint8, device=E.device)
    keep = torch.empty(f.shape[0], dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_cull_vertices", v.data_ptr(), v.shape[0], int(v.dtype == torch.float64), w2c.data_ptr(), K, int(H), int(W), float(fx),
               float(fy), float(cx), float(cy), f.data_ptr(), f.shape[0], seen.data_ptr(), keep.data_ptr())
    return seen.bool(), keep.bool()


def cull_mesh(vertices, faces, c2w_list, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, compact=False,
              engine: Optional[Engine] = None, *, occlusion=False, eps=0.03, min_views=1, stride=1):
    """(vertices, faces) with every face removed that no pose of ``c2w_list`` sees any vertex of (cull_mesh.py).  As the
    reference's ``mesh.update_faces`` the vertex array is returned unchanged; ``compact=True`` drops unreferenced vertices
    and renumbers the faces.  ``occlusion``, ``eps``, ``min_views``, ``stride``: as cull_masks."""
    E = engine or gpu()
    _, keep = cull_masks(vertices, faces, c2w_list, H, W, fx, fy, cx, cy, E, occlusion=occlusion, eps=eps, min_views=min_views,
                         stride=stride)
    v = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertices))
    v = v.to(E.device)
    f = E.faces(faces)[keep]
    return compact_mesh(v, f) if compact else (v, f)


# earlier names of the shared engine's pieces, still called by tools and tests written against them
_gpu = gpu


def _transform(E: Engine, pts: torch.Tensor, T):
    E.transform(pts, T)


# the 2-D metric and the rasterizer live in raster.py (which imports this module's ICP)
from .raster import (calc_2d_metric, cam_position, depth_l1, render_depth, sample_views, unseen_points,  # noqa: E402
                     visibility_counts)


# --------------------------------------------------------------------------------------------------
# command line: eval_recon.py -3d / calc_2d_metric, cull_mesh.py and the unseen cloud of a ground truth
# --------------------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nice_slam_amd.recon", description="Reconstruction evaluation on the GPU.")
    sub = ap.add_subparsers(dest="cmd", required=True)
    ev = sub.add_parser("eval", help="eval_recon.py: 3-D metrics of a reconstructed mesh")
    ev.add_argument("--rec_mesh", type=str, help="reconstructed mesh file path")
    ev.add_argument("--gt_mesh", type=str, help="ground truth mesh file path")
    ev.add_argument("-2d", "--metric_2d", action="store_true", help="enable 2D metric (not available)")
    ev.add_argument("-3d", "--metric_3d", action="store_true", help="enable 3D metric")
    ev.add_argument("--seed", type=int, default=0, help="seed of the surface samplers")
    ev.add_argument("--n_points", type=int, default=200000, help="surface samples per mesh")
    ev.add_argument("--surface", choices=("points", "mesh"), default=None,
                    help="mesh: point-to-mesh distances, with F-score and normal consistency (not the reference's metric)")
    ev.add_argument("--thresholds", type=float, nargs="+", default=[0.05], help="with --surface mesh: F-score thresholds (m)")
    ev.add_argument("--error_mesh", type=str, default=None,
                    help="with --surface mesh: write the aligned reconstruction coloured by its distance to the ground-truth mesh")
    de = sub.add_parser("depth", help="eval_recon.py calc_2d_metric: Depth L1 of a reconstructed mesh")
    de.add_argument("--rec_mesh", type=str, required=True, help="reconstructed mesh file path")
    de.add_argument("--gt_mesh", type=str, required=True, help="ground truth mesh file path")
    un = de.add_mutually_exclusive_group()
    un.add_argument("--unseen", type=str, default=None, help="unseen point cloud (.npy; default: <gt_mesh>_pc_unseen.npy)")
    un.add_argument("--no_unseen", action="store_true", help="accept every candidate view")
    de.add_argument("--n_imgs", type=int, default=1000, help="number of views")
    de.add_argument("--seed", type=int, default=0, help="seed of the view stream")
    de.add_argument("--no_align", action="store_true", help="skip the ICP alignment of the reconstruction")
    cu = sub.add_parser("cull", help="cull_mesh.py: remove faces no camera of a trajectory sees")
    cu.add_argument("--input_mesh", type=str, help="path to the mesh to be culled")
    cu.add_argument("--traj", type=str, help="path to the trajectory")
    cu.add_argument("--output_mesh", type=str, help="path to the output mesh")
    cu.add_argument("--occlusion", action="store_true", help="also drop what the mesh itself hides from every camera")
    cu.add_argument("--eps", type=float, default=0.03, help="with --occlusion: depth a vertex may lie behind the rendered surface (m)")
    cu.add_argument("--min_views", type=int, default=1, help="with --occlusion: cameras that must see a vertex")
    cu.add_argument("--stride", type=int, default=1, help="with --occlusion: use every stride-th pose")
    us = sub.add_parser("unseen", help="the ground-truth surface points no camera of a trajectory sees (<gt_mesh>_pc_unseen.npy)")
    us.add_argument("--gt_mesh", type=str, required=True, help="ground truth mesh file path")
    us.add_argument("--traj", type=str, required=True, help="path to the trajectory")
    us.add_argument("--output", type=str, required=True, help="path to the output point cloud (.npy)")
    us.add_argument("--n_points", type=int, default=200000, help="number of surface samples tested")
    us.add_argument("--seed", type=int, default=0, help="seed of the surface sampler")
    args = ap.parse_args(argv)
    if args.cmd == "eval":
        if args.metric_2d:
            raise NotImplementedError("eval -2d is not wired to the rasterizer: the 2-D depth metric (eval_recon.py calc_2d_metric) "
                                      "is `python -m nice_slam_amd.recon depth --rec_mesh R --gt_mesh G`")
        if args.surface != "mesh" and (args.error_mesh or args.thresholds != [0.05]):
            raise SystemExit("recon eval: --thresholds and --error_mesh need --surface mesh")
        if args.metric_3d:
            m = calc_3d_metric(args.rec_mesh, args.gt_mesh, n_points=args.n_points, seed=args.seed, surface=args.surface or "points",
                               thresholds=args.thresholds)
            print("accuracy: ", m["accuracy_cm"])
            print("completion: ", m["completion_cm"])
            print("completion ratio: ", m["completion_ratio_pct"])
            if args.surface == "mesh":
                print("chamfer: ", m["chamfer_cm"])
                for t in m["fscore_pct"]:
                    print(f"precision@{t}: ", m["precision_pct"][t])
                    print(f"recall@{t}: ", m["recall_pct"][t])
                    print(f"f-score@{t}: ", m["fscore_pct"][t])
                print("normal consistency: ", m["normal_consistency"])
                print("normal pairs: ", m["normal_pairs"])
            if args.error_mesh:
                d = error_mesh(args.rec_mesh, args.gt_mesh, args.error_mesh, align=True)
                print("error mesh: ", args.error_mesh, "max", float(d.max()) if d.shape[0] else 0.0)
    elif args.cmd == "depth":
        unseen = False if args.no_unseen else args.unseen
        m = calc_2d_metric(args.rec_mesh, args.gt_mesh, align=not args.no_align, n_imgs=args.n_imgs, unseen=unseen, seed=args.seed)
        print("Depth L1: ", m["depth_l1_cm"])
    elif args.cmd == "unseen":
        pts = unseen_points(args.gt_mesh, load_poses(args.traj), n_points=args.n_points, seed=args.seed)
        np.save(args.output, pts)
        print("unseen points: ", len(pts), "of", args.n_points)
    else:
        v, f = read_mesh(args.input_mesh)
        poses = load_poses(args.traj)
        _, keep = cull_masks(v, f, poses, occlusion=args.occlusion, eps=args.eps, min_views=args.min_views, stride=args.stride)
        write_ply(args.output_mesh, v, f[keep.cpu().numpy()])
    return 0


if __name__ == "__main__":
    sys.exit(main())
