#!/usr/bin/env python3
"""Mint tests/golden/depth_eval.npz by executing the UNMODIFIED reference ``viewmatrix`` and ``check_proj`` of
``src/tools/eval_recon.py`` on CPU: the candidate c2w of calc_2d_metric's rejection loop (:164-176) and its "sees an unseen
point" verdict, for a fixed set of draws and a fixture unseen cloud.

Run (in the build container only; the reference tree does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depth.py

open3d / trimesh are absent: stub modules let eval_recon.py import; Tensor.cuda -> identity and numpy 2 shims live in this
script only.  trimesh.sample.volume_rectangular is replaced by its formula on the recorded uniforms
((u - 0.5) * extents, then the 4x4 transform applied to the homogeneous points), random.uniform by the recorded target
uniforms: the loop body is restated around the two reference functions, which run as they are.
"""
import os
import sys
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
_from_numpy = torch.from_numpy
torch.from_numpy = lambda a: a if isinstance(a, torch.Tensor) else _from_numpy(a)

for _m in ("open3d", "trimesh", "tqdm"):
    if _m not in sys.modules:
        sys.modules[_m] = types.ModuleType(_m)

import eval_recon  # noqa: E402

H, W, FOCAL = 500, 500, 300
CX, CY = H / 2.0 - 0.5, W / 2.0 - 0.5


def main():
    rng = np.random.default_rng(20261015)
    # a box the size of a Replica room, rotated about z and lifted, as get_cam_position returns one
    extents = np.array([2.6, 5.0, 6.3]) * np.array([0.3, 0.7, 0.7])
    a = 0.4
    transform = np.eye(4)
    transform[:3, :3] = [[0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)], [1.0, 0.0, 0.0]]
    transform[:3, 3] = [0.3, -0.2, 1.7]
    # the unseen cloud: a patch of points outside one wall and a few scattered ones
    unseen = np.concatenate([rng.uniform([-4.0, 3.0, 0.0], [4.0, 3.4, 3.0], (300, 3)), rng.uniform(-5, 5, (20, 3))])
    draws = rng.random((400, 6))
    c2ws, seen = [], []
    for d in draws:
        p = (d[:3] - 0.5) * extents
        origin = np.dot(transform, np.append(p, 1.0))[:3].reshape(-1)
        tx, ty, tz = (round(-10000.0 + 20000.0 * float(x), 2) for x in d[3:])
        target = np.array([tx, ty, tz]) - np.array(origin)
        c2w = eval_recon.viewmatrix(target, [0, 0, -1], origin)
        tmp = np.eye(4)
        tmp[:3, :] = c2w
        c2w = tmp
        s = eval_recon.check_proj(unseen, W, H, FOCAL, FOCAL, CX, CY, c2w)
        c2ws.append(c2w)
        seen.append(bool(s))
    out = os.path.join(HERE, "depth_eval.npz")
    np.savez_compressed(out, extents=extents, transform=transform, unseen=unseen, draws=draws, c2w=np.array(c2ws),
                        seen=np.array(seen))
    print(out, f"{len(draws)} draws, {int(np.sum(seen))} see the unseen cloud")


if __name__ == "__main__":
    main()
