#!/usr/bin/env python3
"""Mint the golden fixture of the overlap keyframe selection by executing the UNMODIFIED reference
``Mapper.keyframe_selection_overlap`` (src/Mapper.py:166-228) on the CPU, on a Mapper built the way
``make_golden_callers.py`` builds it (same stub modules; this script imports that one for them).

Run in the build container only (the reference tree does not exist on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_keyframes.py

Writes ``tests/golden/keyframe_overlap.npz``: the intrinsics and one 120x160 depth image (a block of zero-depth pixels
included), and per case ``<case>/``:
    indices       the pixel draw of the call (recorded by wrapping the module's ``get_samples``)
    c2w, est_c2w  the current pose and the K keyframe poses (fp32)
    percent       [K] percent_inside per keyframe in id order (recorded by wrapping ``sorted`` in the module's globals)
    sorted_ids    [K] the ids in the order ``sorted`` returned them
    candidates    the array handed to ``np.random.permutation`` (ids with a share above 0, sorted)
    k, pixels, n_samples, out (the returned list; -1 padded never: `out_len` says how long it is)
    rng_keys / rng_pos / rng_has_gauss / rng_gauss   numpy's global MT19937 state before the call
    after         np.random.random(4) right after the call
Cases: K in {0, 1, 7, 40, 150}; poses equal to the current one (ties: the stable order matters); poses facing away (share 0);
poses whose image plane cuts the point cloud (points at z ~ 0) or that see it across the 20-pixel border; k above the
candidate count and k = 0; one call with pixels = 150, N_samples = 24 (3600 points: more than one LDS chunk of the kernel).
"""
import builtins
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_callers as mgc                          # noqa: E402  (stub modules + the reference on sys.path)
import numpy as np                                         # noqa: E402
import torch                                               # noqa: E402

import src.Mapper as ref_mapper_mod                        # noqa: E402
from src.Mapper import Mapper                              # noqa: E402

H, W, FX, FY, CX, CY = 120, 160, 131.0, 129.5, 79.5, 60.25
OUT = os.path.join(HERE, "keyframe_overlap.npz")


def rot(axis, ang):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def pose(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return torch.from_numpy(m.astype(np.float32))


def depth_image(rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 1.6 + 0.6 * np.sin(xx / 23.0) * np.cos(yy / 17.0) + 0.004 * (xx - yy) + rng.normal(0, 0.01, (H, W))
    d[40:70, 100:135] = 0.0                                # missing depth
    d[:6, :] = 0.0
    return torch.from_numpy(d.astype(np.float32))


def keyframes(rng, cur, kinds):
    """kinds: list of 'near', 'same', 'away', 'cut', 'shift'"""
    c = cur.numpy().astype(np.float64)
    fwd = -c[:3, 2]                                        # the camera looks down its -z axis
    out = []
    for kind in kinds:
        if kind == "same":
            out.append(cur.clone())
        elif kind == "near":
            R = rot(rng.normal(size=3), rng.uniform(0.0, 0.35)) @ c[:3, :3]
            out.append(pose(R, c[:3, 3] + rng.uniform(-0.3, 0.3, 3)))
        elif kind == "away":
            R = c[:3, :3] @ rot([0, 1, 0], np.pi + rng.uniform(-0.2, 0.2))
            out.append(pose(R, c[:3, 3] + rng.uniform(-0.1, 0.1, 3)))
        elif kind == "cut":                                # inside the cloud, looking sideways: z ~ 0 for many points
            R = c[:3, :3] @ rot([0, 1, 0], np.pi / 2 * rng.choice([-1, 1]) + rng.uniform(-0.1, 0.1))
            out.append(pose(R, c[:3, 3] + fwd * rng.uniform(1.2, 2.0)))
        elif kind == "shift":                              # the same view shifted sideways: the border cuts through the points
            out.append(pose(c[:3, :3], c[:3, 3] + c[:3, 0] * rng.uniform(-0.9, 0.9) + c[:3, 1] * rng.uniform(-0.6, 0.6)))
    return out


CASES = [  # name, kinds, k, pixels, n_samples
    ("k0", [], 3, 100, 16),
    ("k1", ["near"], 3, 100, 16),
    ("k7", ["same", "near", "same", "away", "near", "same", "shift"], 10, 100, 16),
    ("k40", ["near"] * 14 + ["same"] * 4 + ["away"] * 6 + ["cut"] * 8 + ["shift"] * 8, 3, 100, 16),
    ("k150", ["near"] * 60 + ["same"] * 10 + ["away"] * 20 + ["cut"] * 30 + ["shift"] * 30, 3, 100, 16),
    ("kzero", ["near", "same", "near", "shift", "away", "cut", "near"], 0, 100, 16),
    ("px150n24", ["near"] * 5 + ["same"] * 2 + ["away", "cut", "cut", "shift", "shift"], 3, 150, 24),
]


def main():
    cfg, bound, grids, dec, _ = mgc.build()
    slam = mgc.make_slam(cfg, bound, grids, dec)
    slam.H, slam.W, slam.fx, slam.fy, slam.cx, slam.cy = H, W, FX, FY, CX, CY
    m = Mapper(cfg, None, slam)
    assert (m.H, m.W, m.fx, m.fy, m.cx, m.cy) == (H, W, FX, FY, CX, CY) and m.device == "cpu"
    rng = np.random.default_rng(2024)
    depth = depth_image(rng)
    color = torch.from_numpy(rng.uniform(0, 1, (H, W, 3)).astype(np.float32))
    out = {"intr": np.array([H, W, FX, FY, CX, CY], dtype=np.float64), "depth": depth.numpy(),
           "cases": np.array([c[0] for c in CASES])}

    rec = {}
    _gs = ref_mapper_mod.get_samples

    def rec_get_samples(H0, H1, W0, W1, n, HH, WW, fx, fy, cx, cy, c2w, d, col, device):
        st = torch.get_rng_state()                         # the draw get_sample_uv is about to make (common.py:99)
        rec["indices"] = torch.randint((H1 - H0) * (W1 - W0), (n,), device=device).numpy().copy()
        torch.set_rng_state(st)
        return _gs(H0, H1, W0, W1, n, HH, WW, fx, fy, cx, cy, c2w, d, col, device)

    def rec_sorted(it, *a, **k):
        it = list(it)
        rec["percent"] = np.array([float(d["percent_inside"]) for d in it], dtype=np.float64)
        rec["ids_in"] = [d["id"] for d in it]
        r = builtins.sorted(it, *a, **k)
        rec["sorted_ids"] = np.array([d["id"] for d in r], dtype=np.int64)
        return r

    _perm = np.random.permutation

    def rec_perm(x):
        rec["candidates"] = np.array(x).copy()
        return _perm(x)

    ref_mapper_mod.get_samples = rec_get_samples
    ref_mapper_mod.sorted = rec_sorted
    np.random.permutation = rec_perm
    try:
        for ci, (name, kinds, k, pixels, n_samples) in enumerate(CASES):
            c = rng.uniform(-0.3, 0.3)
            cur = pose(rot([0.2, 1.0, 0.1], c), [0.1 * ci, 0.05, 0.4])
            kfs = keyframes(rng, cur, kinds)
            perm = rng.permutation(len(kfs))                   # interleave the kinds
            kfs = [kfs[i] for i in perm]
            kfd = [{"est_c2w": p, "idx": 50 * i} for i, p in enumerate(kfs)]
            rec.clear()
            torch.manual_seed(100 + ci)
            np.random.seed(200 + ci)
            np.random.random(ci)                               # a state that is not fresh from a seed
            name_, keys, pos, has_gauss, gauss = np.random.get_state()
            sel = m.keyframe_selection_overlap(color, depth, cur, kfd, k, N_samples=n_samples, pixels=pixels)
            after = np.random.random(4)
            p = f"{name}/"
            K = len(kfs)
            if K:
                assert rec["ids_in"] == list(range(K))
            out[p + "indices"] = rec["indices"]
            out[p + "c2w"] = cur.numpy()
            out[p + "est_c2w"] = np.stack([t.numpy() for t in kfs]) if K else np.zeros((0, 4, 4), np.float32)
            out[p + "percent"] = rec.get("percent", np.zeros(0))
            out[p + "sorted_ids"] = rec.get("sorted_ids", np.zeros(0, np.int64))
            out[p + "candidates"] = rec["candidates"]
            out[p + "k"] = np.array(k)
            out[p + "pixels"] = np.array(pixels)
            out[p + "n_samples"] = np.array(n_samples)
            out[p + "out"] = np.array(sel, dtype=np.int64)
            out[p + "out_types"] = np.array([type(v).__name__ for v in sel])
            out[p + "rng_keys"] = np.asarray(keys, dtype=np.uint32)
            out[p + "rng_pos"] = np.array(pos)
            out[p + "rng_has_gauss"] = np.array(has_gauss)
            out[p + "rng_gauss"] = np.array(gauss, dtype=np.float64)
            out[p + "after"] = after
            n = pixels * n_samples
            cnt = np.rint(out[p + "percent"] * n).astype(np.int64)
            print(f"{name}: K={K} k={k} n={n} candidates={len(rec['candidates'])} out={sel} "
                  f"zero-share={int((cnt == 0).sum())} counts[:8]={cnt[:8].tolist()}")
    finally:
        ref_mapper_mod.get_samples = _gs
        del ref_mapper_mod.sorted
        np.random.permutation = _perm
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
