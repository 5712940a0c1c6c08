"""Reconstruction evaluation on the GPU: a drop-in for the reference's ``src/tools/eval_recon.py`` (3-D metrics) and
``src/tools/cull_mesh.py``.

    from nice_slam_amd import recon
    recon.calc_3d_metric("rec.ply", "gt.ply")      # {accuracy_cm, completion_cm, completion_ratio_pct}
    recon.calc_2d_metric("rec.ply", "gt.ply")      # {depth_l1_cm, per_view}  (nice_slam_amd/raster.py)

    python -m nice_slam_amd.recon eval --rec_mesh R --gt_mesh G -3d
    python -m nice_slam_amd.recon depth --rec_mesh R --gt_mesh G
    python -m nice_slam_amd.recon cull --input_mesh M --traj traj.txt --output_mesh OUT

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
    rasterizer, not Open3D's OpenGL depth buffer; its own deviations are listed in raster.py.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from typing import Optional

import numpy as np
import torch

from . import _capi
from .common import _stream
from .mesher import write_ply

__all__ = ["nearest", "accuracy", "completion", "completion_ratio", "recon_metrics", "sample_surface", "align_icp",
           "calc_3d_metric", "cull_mesh", "load_poses", "read_mesh", "NNIndex",
           "render_depth", "depth_l1", "cam_position", "sample_views", "calc_2d_metric"]


# --------------------------------------------------------------------------------------------------
# the engine: one library (the product's libnsr.so on a GPU) and the device its tensors live on
# --------------------------------------------------------------------------------------------------
class Engine:
    """Drives the reconstruction entry points of a loaded library on tensors of one device.  The product uses the GPU
    engine (``_gpu()``); the CPU tests build one on the emulator library, which takes host pointers."""

    def __init__(self, lib, device):
        self.lib = lib
        self.device = torch.device(device)

    def stream(self):
        return _stream(self.device) if self.device.type == "cuda" else None

    def guard(self):
        return _capi.on_device(self.device if self.device.type == "cuda" else None)

    def tensor(self, a, dtype=None, what="points"):
        """[N, 3] contiguous tensor on this device (numpy and tensors of any device accepted; fp32 / fp64 kept)."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if dtype is None:
            dtype = t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float64
        t = t.detach().to(self.device, dtype).contiguous()
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what} must be [N, 3] (got {tuple(t.shape)})")
        return t


_gpu_engine = None


def _gpu() -> Engine:
    global _gpu_engine
    if _gpu_engine is None:
        if not torch.cuda.is_available():
            raise _capi.NsrError("nice_slam_amd.recon needs the AMD GPU; there is no CPU path")
        _gpu_engine = Engine(_capi.get_lib(), torch.device("cuda", torch.cuda.current_device()))
    return _gpu_engine


def _dbl(v):
    v = [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]
    return (C.c_double * len(v))(*v)


# --------------------------------------------------------------------------------------------------
# nearest neighbour
# --------------------------------------------------------------------------------------------------
class NNIndex:
    """Exact nearest-neighbour index over ``ref`` [M, 3] (fp32 or fp64): a uniform cell grid built on the device.
    ``query(q)`` -> (dist fp64 [N], idx int64 [N]) as ``scipy.spatial.cKDTree(ref).query(q)``; distances in fp64,
    ties to the smallest reference index."""

    def __init__(self, ref, engine: Optional[Engine] = None):
        E = self.engine = engine or _gpu()
        lib = E.lib
        r = self.ref = E.tensor(ref, what="nearest: ref")
        M = self.m = r.shape[0]
        if M == 0:
            raise ValueError("nearest: the reference set is empty")
        self.fp64 = int(r.dtype == torch.float64)
        with torch.no_grad(), E.guard():
            bounds = torch.empty(6 * 257, dtype=torch.float64, device=E.device)
            lib.check(lib.nsr_nn_bounds(r.data_ptr(), M, self.fp64, bounds.data_ptr(), E.stream()), "nsr_nn_bounds")
            b = bounds[:6].cpu().numpy()
            self.plan = (C.c_double * 16)()
            lib.check(lib.nsr_nn_plan(_dbl(b), M, self.plan), "nsr_nn_plan")
            nbytes = lib.nsr_nn_workspace_bytes(self.plan, M)
            if nbytes < 0:
                raise _capi.NsrError("nearest: invalid grid plan")
            self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=E.device)
            keys = torch.empty(M, dtype=torch.int64, device=E.device)
            lib.check(lib.nsr_nn_keys(r.data_ptr(), M, self.fp64, self.plan, keys.data_ptr(), E.stream()), "nsr_nn_keys")
            sk, order = torch.sort(keys, stable=True)
            lib.check(lib.nsr_nn_build(r.data_ptr(), M, self.fp64, self.plan, sk.data_ptr(), order.contiguous().data_ptr(),
                                       self.ws.data_ptr(), E.stream()), "nsr_nn_build")

    def query(self, q, with_candidates: bool = False):
        E, lib = self.engine, self.engine.lib
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
                lib.check(lib.nsr_nn_keys(qt.data_ptr(), N, fp64, self.plan, keys.data_ptr(), E.stream()), "nsr_nn_keys")
                qorder = torch.sort(keys, stable=True)[1].contiguous()
                lib.check(lib.nsr_nn_query(qt.data_ptr(), N, fp64, qorder.data_ptr(), self.plan, self.ws.data_ptr(), self.m,
                                           dist.data_ptr(), idx.data_ptr(), None if ncand is None else ncand.data_ptr(),
                                           E.stream()), "nsr_nn_query")
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
        lib.check(lib.nsr_dist_stats(dist.data_ptr(), n, float(th), partial.data_ptr(), out.data_ptr(), E.stream()), "nsr_dist_stats")
    s, c = (float(x) for x in out.cpu())
    return s, c


def _mean(E, dist):
    n = dist.shape[0]
    return _dist_stats(E, dist, 0.0)[0] / n if n else float("nan")


def accuracy(gt_points, rec_points, engine: Optional[Engine] = None) -> float:
    """Mean distance from each reconstructed point to the ground truth (eval_recon.py:32-36)."""
    E = engine or _gpu()
    return _mean(E, nearest(rec_points, gt_points, E)[0])


def completion(gt_points, rec_points, engine: Optional[Engine] = None) -> float:
    """Mean distance from each ground-truth point to the reconstruction (eval_recon.py:39-43)."""
    E = engine or _gpu()
    return _mean(E, nearest(gt_points, rec_points, E)[0])


def completion_ratio(gt_points, rec_points, dist_th=0.05, engine: Optional[Engine] = None) -> float:
    """Fraction of ground-truth points within ``dist_th`` of the reconstruction (eval_recon.py:24-29)."""
    E = engine or _gpu()
    d = nearest(gt_points, rec_points, E)[0]
    return _dist_stats(E, d, dist_th)[1] / d.shape[0] if d.shape[0] else float("nan")


def recon_metrics(gt_points, rec_points, dist_th=0.05, engine: Optional[Engine] = None):
    """(accuracy, completion, completion_ratio) from two nearest-neighbour passes (the reference makes three)."""
    E = engine or _gpu()
    d_acc = nearest(rec_points, gt_points, E)[0]
    d_comp = nearest(gt_points, rec_points, E)[0]
    n = d_comp.shape[0]
    s_comp, c_comp = _dist_stats(E, d_comp, dist_th)
    return _mean(E, d_acc), (s_comp / n if n else float("nan")), (c_comp / n if n else float("nan"))


# --------------------------------------------------------------------------------------------------
# surface sampling (trimesh.sample.sample_surface, eval_recon.py:103,106)
# --------------------------------------------------------------------------------------------------
def _faces(E: Engine, faces):
    f = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    f = f.detach().to(E.device)
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [F, 3] (got {tuple(f.shape)})")
    return f.to(torch.int32).contiguous()


def sample_surface(vertices, faces, count: int, seed: int = 0, uniforms=None, engine: Optional[Engine] = None):
    """(points fp64 [count, 3], face_index int64 [count]): ``count`` points on the mesh, faces picked in proportion to their
    area.  ``uniforms`` [count, 3] fp64 (u0, a, b) replaces the in-kernel philox draws keyed by ``seed``."""
    E = engine or _gpu()
    lib = E.lib
    v = E.tensor(vertices, torch.float64, "sample_surface: vertices")
    f = _faces(E, faces)
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
        lib.check(lib.nsr_sample_surface(v.data_ptr(), v.shape[0], f.data_ptr(), f.shape[0], n, None if u is None else u.data_ptr(),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), pts.data_ptr(), fi.data_ptr(), E.stream()),
                  "nsr_sample_surface")
    return pts, fi


# --------------------------------------------------------------------------------------------------
# ICP (eval_recon.py:45-59: Open3D registration_icp, point to point)
# --------------------------------------------------------------------------------------------------
def _transform(E: Engine, pts: torch.Tensor, T: np.ndarray):
    with E.guard():
        E.lib.check(E.lib.nsr_transform_points(pts.data_ptr(), pts.shape[0], _dbl(np.asarray(T, np.float64)[:3, :4]), E.stream()),
                    "nsr_transform_points")


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
        _transform(E, pcd, T)
    partial = torch.empty(int(lib.nsr_recon_partial_doubles(n)), dtype=torch.float64, device=E.device)
    out = torch.empty(17, dtype=torch.float64, device=E.device)

    def evaluate():
        d, idx = index.query(pcd)
        with E.guard():
            lib.check(lib.nsr_icp_stats(pcd.data_ptr(), tgt.data_ptr(), idx.data_ptr(), d.data_ptr(), n, tgt.shape[0], float(threshold),
                                        partial.data_ptr(), out.data_ptr(), E.stream()), "nsr_icp_stats")
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
        _transform(E, pcd, update)
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
    T, fitness, rmse, _ = _icp(engine or _gpu(), source, target, threshold, init, max_iteration, relative_fitness, relative_rmse)
    return T, fitness, rmse


# --------------------------------------------------------------------------------------------------
# the 3-D metric (eval_recon.py:91-117)
# --------------------------------------------------------------------------------------------------
def _mesh(E: Engine, mesh):
    if isinstance(mesh, str):
        v, f = read_mesh(mesh)
    else:
        v, f = mesh[0], mesh[1]
    return E.tensor(v, torch.float64, "mesh vertices"), _faces(E, f)


def calc_3d_metric(rec_mesh, gt_mesh, align=True, n_points=200000, seed=0, engine: Optional[Engine] = None):
    """Accuracy [cm], completion [cm] and completion ratio [%] of a reconstructed mesh against the ground truth, as
    eval_recon.py's calc_3d_metric: (optionally) ICP-align the reconstruction's vertices to the ground truth's, sample
    ``n_points`` on each surface, then two nearest-neighbour passes.  Meshes: PLY paths or (vertices, faces) pairs (e.g. the
    device tensors ``Mesher.get_mesh`` returns).  The samplers are seeded (``seed`` for the reconstruction, ``seed + 1`` for
    the ground truth)."""
    E = engine or _gpu()
    rv, rf = _mesh(E, rec_mesh)
    gv, gf = _mesh(E, gt_mesh)
    if align:
        T = align_icp(rv, gv, 0.1, engine=E)[0]
        rv = rv.clone()
        _transform(E, rv, T)
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
    out = np.zeros((max(len(c2w_list), 1), 12), dtype=np.float32)
    for k, c2w in enumerate(c2w_list):
        c = c2w.detach().cpu().numpy() if isinstance(c2w, torch.Tensor) else np.asarray(c2w)
        out[k] = np.linalg.inv(c.astype(np.float32)).astype(np.float32)[:3].reshape(-1)
    return out


def cull_masks(vertices, faces, c2w_list, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, engine: Optional[Engine] = None):
    """(seen bool [V], keep bool [F]): vertices some pose sees, faces with at least one seen vertex (cull_mesh.py:45-75)."""
    E = engine or _gpu()
    lib = E.lib
    v = E.tensor(vertices, what="cull_mesh: vertices")
    f = _faces(E, faces)
    K = len(c2w_list)
    w2c = torch.from_numpy(_w2c_rows(c2w_list)).to(E.device)
    seen = torch.empty(v.shape[0], dtype=torch.uint8, device=E.device)
    keep = torch.empty(f.shape[0], dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        lib.check(lib.nsr_cull_vertices(v.data_ptr(), v.shape[0], int(v.dtype == torch.float64), w2c.data_ptr(), K, int(H), int(W),
                                        float(fx), float(fy), float(cx), float(cy), f.data_ptr(), f.shape[0], seen.data_ptr(),
                                        keep.data_ptr(), E.stream()), "nsr_cull_vertices")
    return seen.bool(), keep.bool()


def cull_mesh(vertices, faces, c2w_list, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5, compact=False,
              engine: Optional[Engine] = None):
    """(vertices, faces) with every face removed that no pose of ``c2w_list`` sees any vertex of (cull_mesh.py).  As the
    reference's ``mesh.update_faces`` the vertex array is returned unchanged; ``compact=True`` drops unreferenced vertices
    and renumbers the faces."""
    E = engine or _gpu()
    _, keep = cull_masks(vertices, faces, c2w_list, H, W, fx, fy, cx, cy, E)
    v = vertices if isinstance(vertices, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vertices))
    v = v.to(E.device)
    f = _faces(E, faces)[keep]
    if compact:
        used = torch.zeros(v.shape[0], dtype=torch.bool, device=E.device)
        used[f.reshape(-1).long()] = True
        remap = torch.cumsum(used.long(), 0) - 1
        v, f = v[used], remap[f.long()].to(torch.int32)
    return v, f


# --------------------------------------------------------------------------------------------------
# PLY
# --------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def read_mesh(path: str):
    """(vertices float64 [V, 3], faces int64 [F, 3]) of a PLY file: binary little-endian or ASCII, any extra vertex properties
    (normals, colours, alpha) skipped, the face list counted by uchar / int / uint with int / uint indices.  Other elements
    are skipped; a face that is not a triangle is an error."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property" and elements:
            if tok[1] == "list":
                elements[-1][2].append((tok[4], "list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    verts = np.zeros((0, 3), np.float64)
    faces = np.zeros((0, 3), np.int64)
    if fmt == "ascii":
        lines = data[body:].decode("ascii").split("\n")
        pos = 0
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                while not lines[pos].strip():
                    pos += 1
                rows.append(lines[pos].split())
                pos += 1
            if name == "vertex":
                names = [p[0] for p in props]
                cols = [names.index(c) for c in ("x", "y", "z")]
                verts = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).reshape(-1, 3)
            elif name == "face":
                fl = []
                for r in rows:
                    k = int(r[0])
                    if k != 3:
                        raise ValueError(f"{path}: face with {k} vertices (only triangles are supported)")
                    fl.append([int(x) for x in r[1:4]])
                faces = np.array(fl, dtype=np.int64).reshape(-1, 3)
        return verts, faces
    off = body
    for name, count, props in elements:
        if any(p[1] == "list" for p in props):
            if len(props) != 1:
                raise ValueError(f"{path}: element {name!r} mixes a list with other properties")
            _, _, ct, it = props[0]
            ct, it = np.dtype("<" + ct), np.dtype("<" + it)
            if count == 0:
                continue
            # every face a triangle: fixed-size records; anything else is caught by the count check
            rec = np.dtype([("n", ct), ("idx", it, 3)])
            need = off + rec.itemsize * count
            if need > len(data):
                raise ValueError(f"{path}: truncated, or not every face is a triangle")
            arr = np.frombuffer(data, dtype=rec, count=count, offset=off)
            if not (arr["n"] == 3).all():
                bad = int(arr["n"][arr["n"] != 3][0])
                raise ValueError(f"{path}: face with {bad} vertices (only triangles are supported)")
            if name == "face":
                faces = arr["idx"].astype(np.int64)
            off = need
        else:
            rec = np.dtype([(p[0], "<" + p[1]) for p in props])
            arr = np.frombuffer(data, dtype=rec, count=count, offset=off)
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
            off += rec.itemsize * count
    return verts, faces


# the 2-D metric and the rasterizer live in raster.py (which imports this module's engine and ICP)
from .raster import calc_2d_metric, cam_position, depth_l1, render_depth, sample_views  # noqa: E402


# --------------------------------------------------------------------------------------------------
# command line: eval_recon.py -3d / calc_2d_metric and cull_mesh.py
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
    else:
        v, f = read_mesh(args.input_mesh)
        poses = load_poses(args.traj)
        _, keep = cull_masks(v, f, poses)
        write_ply(args.output_mesh, v, f[keep.cpu().numpy()])
    return 0


if __name__ == "__main__":
    sys.exit(main())
