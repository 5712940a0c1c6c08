"""Overlap keyframe selection on the GPU (nice_slam_amd.KeyframeSelector) against the reference's numpy loop
(Mapper.keyframe_selection_overlap, src/Mapper.py:166-228, as tests/keyframe_reference.py restates it, fed with the same
1600 points), for K in {0, 10, 40, 110, 250, 1000} keyframes, pixels = 100, N_samples = 16, on a 680 x 1200 frame.
Writes profiles/keyframe_timing.json.

    python tools/keyframe_timing.py [--out profiles/keyframe_timing.json] [--reps 50]

Per K (medians over --reps warmed-up calls, milliseconds):
    drop_in_ms       KeyframeSelector.keyframe_selection_overlap, wall clock (the draw, the launch, the counts to the host,
                     sort and permutation), pose inverses cached (the steady state of a mapping run)
    drop_in_cold_ms  the same with an empty cache (every pose copied to the host and inverted)
    overlap_ms       KeyframeSelector.overlap + torch.cuda.synchronize, wall clock (cached inverses)
    kernel_ms        device events around the one nsr_keyframe_overlap launch
    numpy_loop_ms    the reference's per-keyframe loop on the host, from the points on the host (what it does after its copy)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import keyframe_reference as kr  # noqa: E402
from nice_slam_amd import KeyframeSelector, _capi  # noqa: E402
from nice_slam_amd.common import _stream  # noqa: E402
from nice_slam_amd.keyframes import EDGE, t_vals  # noqa: E402

H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5
DEV = "cuda:0"


def numpy_loop(vertices, est, k):
    """The reference's host work after its copy of the points, as tests/keyframe_reference.py restates it: per keyframe a numpy
    inverse, the (4,4) @ (N,4,1) and (3,3) @ (N,3,1) matmuls and the border test, then the shares, sort and permutation."""
    inside = kr.inside_matmul(vertices, est, H, W, FX, FY, CX, CY)[0]
    return kr.select(inside.sum(1), vertices.shape[0], k)


def scene(rng, K):
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (2.0 + 0.8 * np.sin(xx / 90.0) * np.cos(yy / 70.0)).astype(np.float32)
    c2w = np.eye(4, dtype=np.float32)
    est = []
    for _ in range(K):
        a = rng.normal(size=3)
        a *= rng.uniform(0, 1.0) / np.linalg.norm(a)
        th = np.linalg.norm(a) + 1e-12
        Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        m = np.eye(4)
        m[:3, :3] = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
        m[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        est.append(m.astype(np.float32))
    return depth, c2w, est


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_timing.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ks", default="0,10,40,110,250,1000")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    lib = _capi.get_lib()
    rows = []
    for K in [int(v) for v in args.ks.split(",")]:
        depth, c2w, est = scene(rng, K)
        d_dev, c_dev = torch.from_numpy(depth).to(DEV), torch.from_numpy(c2w).to(DEV)
        kfd = [{"est_c2w": torch.from_numpy(m).to(DEV)} for m in est]
        poses = [kf["est_c2w"] for kf in kfd]
        sel = KeyframeSelector(H, W, FX, FY, CX, CY)

        def drop_in():
            return sel.keyframe_selection_overlap(None, d_dev, c_dev, kfd, 3)

        def drop_in_cold():
            sel._inv = {}
            return sel.keyframe_selection_overlap(None, d_dev, c_dev, kfd, 3)

        def overlap():
            sel.overlap(c_dev, d_dev, poses)
            torch.cuda.synchronize()

        for f in (drop_in, overlap, drop_in_cold, drop_in):          # warm-up (the last leaves the cache filled)
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        row = {"K": K, "pixels": 100, "n_samples": 16, "drop_in_ms": med(drop_in, args.reps),
               "overlap_ms": med(overlap, args.reps), "drop_in_cold_ms": med(drop_in_cold, args.reps)}
        drop_in()
        # the kernel alone, between device events
        idx = torch.randint(H * W, (100,), device=DEV)
        w2c = torch.from_numpy(sel.w2c_rows(poses)).to(DEV)
        counts = torch.empty((max(K, 1),), dtype=torch.int32, device=DEV)
        tv = t_vals(16)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ks = []
        if K:
            for r in range(args.reps + 5):
                ev0.record()
                lib.check(lib.nsr_keyframe_overlap(idx.data_ptr(), 100, 16, tv.ctypes.data_as(C.POINTER(C.c_float)), H, W, FX, FY, CX, CY,
                                                   EDGE, c_dev.data_ptr(), 4, d_dev.data_ptr(), w2c.data_ptr(), K, counts.data_ptr(),
                                                   _stream(DEV)), "nsr_keyframe_overlap")
                ev1.record()
                ev1.synchronize()
                if r >= 5:
                    ks.append(ev0.elapsed_time(ev1))
        row["kernel_ms"] = float(np.median(ks)) if ks else 0.0
        # the reference's host loop on the same points
        pts = kr.points(idx.cpu().numpy(), depth, c2w, FX, FY, CX, CY, 16)
        est_host = [m.copy() for m in est]
        numpy_loop(pts.copy(), est_host, 3)
        row["numpy_loop_ms"] = med(lambda: numpy_loop(pts.copy(), est_host, 3), max(3, args.reps // 5 if K >= 250 else args.reps))
        row["numpy_loop_per_keyframe_ms"] = row["numpy_loop_ms"] / K if K else None
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "frame": [H, W], "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
