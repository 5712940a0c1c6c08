"""Reconstruction evaluation on the GPU: a drop-in for the reference's ``src/tools/eval_recon.py`` (3-D metrics) and
``src/tools/cull_mesh.py``.

    from nice_slam_amd import recon
    recon.calc_3d_metric("rec.ply", "gt.ply")      # {accuracy_cm, completion_cm, completion_ratio_pct}
    recon.calc_2d_metric("rec.ply", "gt.ply")      # {depth_l1_cm, per_view}  (nice_slam_amd/raster.py)

    python -m nice_slam_amd.recon eval --rec_mesh R --gt_mesh G -3d
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
    truth, which the reference ships only for its own scenes.
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
           "unseen_points"]


# --------------------------------------------------------------------------------------------------
# nearest neighbour
# --------------------------------------------------------------------------------------------------
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
            bounds = torch.empty(6 * 257, dtype=torch.float64, device=E.device)
            E.call("nsr_nn_bounds", r.data_ptr(), M, self.fp64, bounds.data_ptr())
            b = bounds[:6].cpu().numpy()
            self.plan = (C.c_double * 16)()
            lib.call("nsr_nn_plan", c_doubles(b), M, self.plan)
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
        qt = E.tensor(q, what="nearest: query")
        N = qt.shape[0]
        dist = torch.empty(N, dtype=torch.float64, device=E.device)
        idx = torch.empty(N, dtype=torch.int64, device=E.device)
        ncand = torch.empty(N, dtype=torch.int32, device=E.device) if with_candidates else None
        if N:
            if not bool(torch.isfinite(qt).all()):
                raise ValueError("nearest: query coordinates must be finite")
            fp64 = int(qt.dtype == torch.float64)
            with torch.no_grad(), E.guard():
                keys = torch.empty(N, dtype=torch.int64, device=E.device)
                E.call("nsr_nn_keys", qt.data_ptr(), N, fp64, self.plan, keys.data_ptr())
                qorder = torch.sort(keys, stable=True)[1].contiguous()
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
# the 3-D metric (eval_recon.py:91-117)
# --------------------------------------------------------------------------------------------------
def calc_3d_metric(rec_mesh, gt_mesh, align=True, n_points=200000, seed=0, engine: Optional[Engine] = None):
    """Accuracy [cm], completion [cm] and completion ratio [%] of a reconstructed mesh against the ground truth, as
    eval_recon.py's calc_3d_metric: (optionally) ICP-align the reconstruction's vertices to the ground truth's, sample
    ``n_points`` on each surface, then two nearest-neighbour passes.  Meshes: PLY paths or (vertices, faces) pairs (e.g. the
    device tensors ``Mesher.get_mesh`` returns).  The samplers are seeded (``seed`` for the reconstruction, ``seed + 1`` for
    the ground truth)."""
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
        if args.metric_3d:
            m = calc_3d_metric(args.rec_mesh, args.gt_mesh, seed=args.seed)
            print("accuracy: ", m["accuracy_cm"])
            print("completion: ", m["completion_cm"])
            print("completion ratio: ", m["completion_ratio_pct"])
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
