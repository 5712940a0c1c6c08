#!/usr/bin/env python3
"""Phase-by-phase timing of reconstruction evaluation (nice_slam_amd.recon) on one MI355X, at 200k and 2M points, with
scipy's cKDTree / numpy on the same inputs for comparison:

  read      read_mesh of a binary PLY of the analytic room (tests/recon_scenes.py) meshed by marching_cubes
  sample    sample_surface of n points (philox)
  grid      NNIndex build over n reference points (bounds, plan, keys, sort, tables)
  nn_acc / nn_comp   the two nearest-neighbour passes of recon_metrics (query, grid built on the other set)
  icp_iter  one ICP iteration on the room mesh's vertices (query + statistics + update), the mean over a 30-iteration run
  cull      nsr_cull_vertices of the mesh's vertices over 2000 poses (and of 1M vertices)

Each phase runs once for warm-up, then `--reps` timed runs ending with torch.cuda.synchronize(); medians in ms.
    python tools/recon_eval_timing.py --out profiles/recon_eval_timing.json [--sizes 200000 2000000] [--reps 5] [--no-cpu]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import recon_scenes as RS  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def cpu_timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_eval_timing.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[200000, 2000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--no-cpu", action="store_true", help="skip the cKDTree / numpy comparison")
    args = ap.parse_args()
    from scipy.spatial import cKDTree
    from nice_slam_amd import marching_cubes, recon
    from nice_slam_amd.engine import gpu
    from nice_slam_amd.ply import write_ply
    E = gpu()
    f, sp, org = RS.room_lattice(args.res)
    v, fc = marching_cubes(torch.from_numpy(f).to(DEV), 0.0, sp, org)
    out = {"device": torch.cuda.get_device_name(0), "mesh": {"res": args.res, "V": int(v.shape[0]), "F": int(fc.shape[0])}, "sizes": {}}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "room.ply")
        write_ply(path, v.cpu().numpy(), fc.cpu().numpy())
        out["mesh"]["read_ms"] = timed(lambda: recon.read_mesh(path), args.reps)
    for n in args.sizes:
        r = {}
        gt = torch.from_numpy(RS.room_surface_points(n, 1)).to(DEV)
        rec = recon.sample_surface(v, fc, n, seed=0)[0]
        r["sample_ms"] = timed(lambda: recon.sample_surface(v, fc, n, seed=0), args.reps)
        r["grid_ms"] = timed(lambda: recon.NNIndex(gt), args.reps)
        ig, ir = recon.NNIndex(gt), recon.NNIndex(rec)
        r["nn_acc_ms"] = timed(lambda: ig.query(rec), args.reps)
        r["nn_comp_ms"] = timed(lambda: ir.query(gt), args.reps)
        _, _, nc = ig.query(rec, with_candidates=True)
        r["candidates_per_query_mean"] = float(nc.double().mean())
        r["candidates_per_query_max"] = int(nc.max())
        r["recon_metrics_ms"] = timed(lambda: recon.recon_metrics(gt, rec), args.reps)
        if not args.no_cpu:
            g, q = gt.cpu().numpy(), rec.cpu().numpy()
            r["ckdtree_build_ms"] = cpu_timed(lambda: cKDTree(g))
            tree = cKDTree(g)
            r["ckdtree_query_ms"] = cpu_timed(lambda: tree.query(q))
        out["sizes"][str(n)] = r
        print(n, json.dumps(r), flush=True)
    # ICP on the mesh's vertices (a 2 deg / 2 cm offset), 30 iterations
    M = RS.rigid([0.3, 0.5, 1.0], 2.0, [0.02, -0.01, 0.01])
    src = v.clone()
    E.transform(src, np.linalg.inv(M))
    t = time.perf_counter()
    T, fit, rmse, it = recon._icp(E, src, v, max_iteration=30, relative_fitness=0.0, relative_rmse=0.0)
    torch.cuda.synchronize()
    out["icp"] = {"iterations": it, "ms_total": (time.perf_counter() - t) * 1e3, "fitness": fit, "rmse": rmse,
                  "error_vs_truth": float(np.abs(T - M).max())}
    out["icp"]["ms_per_iteration"] = out["icp"]["ms_total"] / max(it, 1)
    # cull: 2000 poses on a circle inside the room
    poses = [torch.from_numpy(RS.rigid([0.2 * np.sin(3 * a), 1.0, 0.1], np.rad2deg(a), [2.5 + np.cos(a), 2.0 + np.sin(a), 1.5])).float()
             for a in 2 * np.pi * np.arange(2000) / 2000]
    out["cull"] = {"poses": 2000, "V": int(v.shape[0]), "ms": timed(lambda: recon.cull_masks(v, fc, poses), args.reps)}
    big = torch.from_numpy(RS.room_surface_points(1000000, 3)).to(DEV)
    nof = torch.zeros((0, 3), dtype=torch.int32, device=DEV)
    out["cull"]["ms_1M_vertices"] = timed(lambda: recon.cull_masks(big, nof, poses), args.reps)
    print(json.dumps({k: out[k] for k in ("icp", "cull")}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
