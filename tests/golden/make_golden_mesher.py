#!/usr/bin/env python3
"""Mint tests/golden/mesher_masks.npz by executing the UNMODIFIED reference ``Mesher.point_masks`` and
``Mesher.get_grid_uniform`` (src/utils/Mesher.py:53-212, :322-347) on CPU.

Run (in the build container only; the reference tree does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesher.py

open3d / skimage / trimesh / cv2 (imported by the module and by src.utils.datasets) are absent: empty stub modules let
the module import; neither method touches them.  The Mesher object is built without its constructor (which reads a
dataset); the attributes point_masks and get_grid_uniform read are set directly.  Three keyframes of a 24 x 32 camera,
points in and around their frusta, points_batch_size 37 (so that the per-chunk maximum depth of the depth-test branch,
:166, differs from chunk to chunk).
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
REF = "/root/reference"
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

for _m in ("cv2", "open3d", "skimage", "skimage.measure", "trimesh", "imageio"):
    if _m not in sys.modules:
        sys.modules[_m] = types.ModuleType(_m)

from src.utils.Mesher import Mesher  # noqa: E402


def pose(rng, t):
    a = rng.normal(size=3) * 0.15
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + Kx + Kx @ Kx / 2.0                       # near-identity rotation (orthonormalised below)
    u, _, vt = np.linalg.svd(R)
    c = np.eye(4)
    c[:3, :3] = u @ vt
    c[:3, 3] = t
    return torch.tensor(c, dtype=torch.float32)


def main():
    rng = np.random.default_rng(11)
    H, W, fx, fy, cx, cy = 24, 32, 30.0, 29.0, 15.7, 11.4
    kf_c2w = [pose(rng, t) for t in ([0.0, 0.0, 0.0], [0.6, -0.2, 0.4], [-0.5, 0.3, -0.3])]
    kf_depth = [torch.tensor(rng.uniform(1.5, 5.0, size=(H, W)) * (rng.uniform(size=(H, W)) > 0.05), dtype=torch.float32)
                for _ in kf_c2w]
    all_c2w = torch.stack(kf_c2w + [pose(rng, [0.2, 0.1, -0.6]), pose(rng, [-0.3, -0.4, 0.2])])
    n = 1200
    pts = np.stack([rng.uniform(-5, 5, n), rng.uniform(-4, 4, n), rng.uniform(-8.0, 1.0, n)], 1).astype(np.float32)
    pts[:40, 2] = rng.uniform(-2.0, -0.5, 40)                # near the image centre, in front of the cameras
    pts[:40, :2] *= 0.1
    chunk = 37

    m = Mesher.__new__(Mesher)
    m.points_batch_size = chunk
    m.H, m.W, m.fx, m.fy, m.cx, m.cy = H, W, fx, fy, cx, cy
    kfs = [{"est_c2w": c, "depth": d} for c, d in zip(kf_c2w, kf_depth)]
    out = {}
    for mode in range(3):
        m.depth_test = mode == 2
        s, f, u = m.point_masks(torch.from_numpy(pts), kfs, all_c2w, len(all_c2w) - 1, "cpu", get_mask_use_all_frames=(mode == 0))
        assert not (s & f).any() and ((s.astype(int) + f + u) == 1).all()
        out[f"mask_mode{mode}"] = np.where(s, 1, np.where(f, 2, 0)).astype(np.uint8)
    m.marching_cubes_bound = torch.from_numpy(np.array([[-2.9, 8.9], [-3.2, 5.5], [-3.3, 8.3]]) * 1.0)
    grid = m.get_grid_uniform(9)
    np.savez_compressed(os.path.join(HERE, "mesher_masks.npz"), points=pts, chunk=np.int64(chunk), H=np.int64(H), W=np.int64(W),
                        intr=np.array([fx, fy, cx, cy]), kf_c2w=torch.stack(kf_c2w).numpy(), kf_depth=torch.stack(kf_depth).numpy(),
                        all_c2w=all_c2w.numpy(), mc_bound=m.marching_cubes_bound.numpy(), grid_res=np.int64(9),
                        grid_points=grid["grid_points"].numpy(), **out)
    print({k: np.bincount(v, minlength=3).tolist() for k, v in out.items()})


if __name__ == "__main__":
    main()
