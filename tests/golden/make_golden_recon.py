#!/usr/bin/env python3
"""Mint tests/golden/recon_eval.npz by executing the UNMODIFIED reference ``src/tools/eval_recon.py`` (accuracy, completion,
completion_ratio, :24-43) and ``src/tools/cull_mesh.py`` (run as a script) on CPU.

Run (in the build container only; the reference tree does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_recon.py

open3d / trimesh are absent: stub modules let eval_recon.py import (the three metric functions use scipy's cKDTree only).
numpy 2 shims (np.float, np.bool, torch.from_numpy of a tensor) and Tensor.cuda -> identity live in this script only.  cull_mesh.py runs through runpy
with sys.argv set; its ``trimesh.load`` is a stub that returns the fixture mesh and records ``update_faces``; the
per-vertex mask is read from the script's globals (``whole_mask``: True = no pose sees the vertex).
"""
import os
import runpy
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, os.path.join(REF, "src", "tools"))
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

if not hasattr(np, "float"):
    np.float = float
if not hasattr(np, "bool"):
    np.bool = bool
torch.Tensor.cuda = lambda self, *a, **k: self
# numpy 2 hands np.linalg.inv(<float32 tensor>) back as a tensor (Tensor.__array_wrap__; still inverted in single precision):
# torch.from_numpy passes a tensor through, as the older stack the reference was written against returned an ndarray here
_from_numpy = torch.from_numpy
torch.from_numpy = lambda a: a if isinstance(a, torch.Tensor) else _from_numpy(a)

for _m in ("open3d", "trimesh", "tqdm"):
    if _m not in sys.modules:
        sys.modules[_m] = types.ModuleType(_m)
if not hasattr(sys.modules["tqdm"], "tqdm"):
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it

import eval_recon  # noqa: E402

H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5


def room_surface(rng, n, lo=(-2.0, -1.5, 0.0), hi=(2.5, 1.5, 2.6)):
    """points on the six faces of a box, in proportion to their areas"""
    lo, hi = np.array(lo), np.array(hi)
    ext = hi - lo
    areas = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = lo + rng.uniform(size=(n, 3)) * ext
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, lo[ax], hi[ax])
    return p


def clouds(rng):
    """(name, gt, rec) fixture pairs"""
    out = []
    gt = room_surface(rng, 3000)
    rec = room_surface(rng, 2500) + rng.normal(scale=0.01, size=(2500, 3))
    out.append(("room", gt, rec))
    out.append(("uniform", rng.uniform(-1, 1, (2000, 3)), rng.uniform(-1.1, 1.1, (1500, 3))))
    centres = rng.uniform(-3, 3, (6, 3))
    cl = lambda n: centres[rng.integers(0, 6, n)] + rng.normal(scale=0.08, size=(n, 3))   # noqa: E731
    out.append(("clustered", cl(2000), cl(1800)))
    base = rng.uniform(-1, 1, (400, 3))
    dup_gt = np.concatenate([base, base[:150], base[:40]])                                 # duplicated reference points
    dup_rec = np.concatenate([base[:200] + 0.02, base[200:260]])                          # some queries ON reference points
    out.append(("duplicates", dup_gt, dup_rec))
    far = rng.normal(size=(8, 3))
    far = 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)
    out.append(("far", room_surface(rng, 1500), np.concatenate([room_surface(rng, 1200), far])))
    return out


def pose_from(rng, t, yaw, pitch):
    """a Replica-style c2w (camera looking along its -z after load_poses' flips) at t"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    c = np.eye(4)
    c[:3, :3] = Rz @ Rx
    c[:3, 3] = t
    return c


def cull_fixture(rng, n_poses=20):
    raw = [pose_from(rng, rng.uniform([-1, -1, 0.5], [1.5, 1, 2.0]), rng.uniform(-np.pi, np.pi), rng.uniform(1.2, 1.9))
           for _ in range(n_poses)]
    traj = np.stack([p.reshape(-1) for p in raw])                 # the traj.txt rows
    # what load_poses makes of them: y, z flipped, float32
    eff = []
    for p in raw:
        c = p.copy()
        c[:3, 1] *= -1
        c[:3, 2] *= -1
        eff.append(c.astype(np.float32).astype(np.float64))
    pts = [rng.uniform([-3, -3, -1], [3, 3, 3.5], (1500, 3))]      # all over: in view, behind cameras, outside the frusta
    for k in range(n_poses):                                        # near the image edges of some pose (0.01 .. 0.5 px)
        c = eff[k]
        for u, v in [(0.02, 300.0), (W - 0.02, 100.0), (600.0, 0.05), (900.0, H - 0.05), (-0.3, 200.0), (W + 0.4, 500.0),
                     (500.0, -0.2), (100.0, H + 0.3), (0.5, 0.5), (W - 0.5, H - 0.5)]:
            Z = -rng.uniform(0.5, 3.0)
            cam = np.array([-(u - CX) * Z / FX, (v - CY) * Z / FY, Z, 1.0])
            pts.append((c @ cam)[None, :3])
        cam = np.array([0.1, 0.1, 0.7, 1.0])                         # behind the camera (positive z)
        pts.append((c @ cam)[None, :3])
    verts = np.concatenate(pts)
    # keep the fixture clear of the mask boundaries (>= 1e-3 px in fp64, with the fp32 inverses the reference uses): an
    # fp32 rounding there may flip a comparison, and the test allows no exceptions
    p = verts.astype(np.float32).astype(np.float64)
    clear = np.ones(len(verts), bool)
    for c in eff:
        w = np.linalg.inv(c.astype(np.float32)).astype(np.float64)[:3]
        cam = p @ w[:, :3].T + w[:, 3]
        z = cam[:, 2] + 1e-5
        u, v = (FX * -cam[:, 0] + CX * cam[:, 2]) / z, (FY * cam[:, 1] + CY * cam[:, 2]) / z
        edge = np.minimum.reduce([np.abs(u), np.abs(u - W), np.abs(v), np.abs(v - H)])
        clear &= ~((edge < 1e-3) & (z <= 0))
    verts = verts[clear]
    faces = np.stack([rng.permutation(len(verts))[:3] for _ in range(2500)]).astype(np.int64)
    return traj, verts, faces


class StubMesh:
    def __init__(self, vertices, faces):
        self.vertices = vertices
        self.faces = faces
        self.face_mask = None

    def update_faces(self, mask):
        self.face_mask = np.asarray(mask).copy()

    def export(self, path):
        pass


def main():
    rng = np.random.default_rng(2024)
    out = {}
    names = []
    for name, gt, rec in clouds(rng):
        names.append(name)
        out[f"{name}/gt"] = gt
        out[f"{name}/rec"] = rec
        out[f"{name}/accuracy"] = np.float64(eval_recon.accuracy(gt, rec))
        out[f"{name}/completion"] = np.float64(eval_recon.completion(gt, rec))
        for th in (0.05, 0.02):
            out[f"{name}/completion_ratio_{th}"] = np.float64(eval_recon.completion_ratio(gt, rec, dist_th=th))
    out["cloud_names"] = np.array(names)

    traj, verts, faces = cull_fixture(rng)
    mesh = StubMesh(verts, faces)
    sys.modules["trimesh"].load = lambda path, process=False: mesh
    with tempfile.TemporaryDirectory() as td:
        tp = os.path.join(td, "traj.txt")
        with open(tp, "w") as f:
            for row in traj:
                f.write(" ".join("%.17g" % x for x in row) + "\n")
        saved = sys.argv
        sys.argv = ["cull_mesh.py", "--input_mesh", "fixture.ply", "--traj", tp, "--output_mesh", os.path.join(td, "out.ply")]
        try:
            g = runpy.run_path(os.path.join(REF, "src", "tools", "cull_mesh.py"), run_name="__main__")
        finally:
            sys.argv = saved
    out["cull/traj"] = traj
    out["cull/vertices"] = verts
    out["cull/faces"] = faces
    out["cull/vertex_seen"] = ~np.asarray(g["whole_mask"], dtype=bool)
    out["cull/face_keep"] = np.asarray(mesh.face_mask, dtype=bool)
    path = os.path.join(HERE, "recon_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, {n: (float(out[f"{n}/accuracy"]), float(out[f"{n}/completion"])) for n in names},
          "cull: seen", int(out["cull/vertex_seen"].sum()), "/", len(verts), "faces kept", int(out["cull/face_keep"].sum()), "/", len(faces))


if __name__ == "__main__":
    main()
