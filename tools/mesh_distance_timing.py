#!/usr/bin/env python3
"""Timing of the point-to-mesh distance (nice_slam_amd.recon.MeshIndex) on one MI355X beside the point-to-point search it is
an alternative to (NNIndex), at the sizes of the 3-D metric: 200k queries against the analytic room (tests/recon_scenes.py)
meshed at 256^3 by marching_cubes, and against 200k samples of that mesh.

  mesh_build / mesh_query     MeshIndex over the room mesh (bounds, plan, count, scan, fill, sort, tables); query of n samples
  point_build / point_query   NNIndex over n samples of the mesh; query of n samples (another seed)
  faces_examined              per query, mean and max, for surface samples (what the pruning test bounds) and uniform points
  floor                       the same surface scored by both estimators: two independent n-point samples of the exact room
                              against each other (points), and each sample of the room mesh against the room mesh itself (mesh)
  surface_metrics             the whole mesh estimator of the room mesh against a copy shifted by 1 cm, beside calc_3d_metric

Each phase runs once for warm-up, then `--reps` timed runs ending with torch.cuda.synchronize(); medians in ms.
    python tools/mesh_distance_timing.py --out profiles/mesh_distance_timing.json [--n 200000] [--res 256] [--reps 5]
"""
import argparse
import json
import os
import sys
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance_timing.json"))
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from nice_slam_amd import marching_cubes, recon
    n = args.n
    f, sp, org = RS.room_lattice(args.res)
    v, fc = marching_cubes(torch.from_numpy(f).to(DEV), 0.0, sp, org)
    out = {"device": torch.cuda.get_device_name(0), "queries": n, "mesh": {"res": args.res, "V": int(v.shape[0]), "F": int(fc.shape[0])}}
    a = recon.sample_surface(v, fc, n, seed=0)[0]
    b = recon.sample_surface(v, fc, n, seed=1)[0]
    rng = np.random.default_rng(0)
    uni = torch.from_numpy(rng.uniform(RS.ROOM_LO - RS.MARGIN, RS.ROOM_HI + RS.MARGIN, (n, 3))).to(DEV)

    mi = recon.MeshIndex(v, fc)
    out["mesh"].update(pairs=mi.npairs, oversize=mi.nover, workspace_mb=mi.ws.numel() / 2 ** 20)
    out["mesh_build_ms"] = timed(lambda: recon.MeshIndex(v, fc), args.reps)
    out["mesh_query_ms"] = timed(lambda: mi.query(a), args.reps)
    out["mesh_query_uniform_ms"] = timed(lambda: mi.query(uni), args.reps)
    for name, q in (("surface", a), ("uniform", uni)):
        nc = mi.query(q, with_candidates=True)[3]
        out[f"faces_examined_{name}"] = {"mean": float(nc.double().mean()), "max": int(nc.max())}
    ni = recon.NNIndex(b)
    out["point_build_ms"] = timed(lambda: recon.NNIndex(b), args.reps)
    out["point_query_ms"] = timed(lambda: ni.query(a), args.reps)
    out["points_examined_surface"] = {"mean": float(ni.query(a, with_candidates=True)[2].double().mean())}

    # the floor: one surface, two estimators
    g1 = torch.from_numpy(RS.room_surface_points(n, 1)).to(DEV)
    g2 = torch.from_numpy(RS.room_surface_points(n, 2)).to(DEV)
    acc, comp, _ = recon.recon_metrics(g1, g2)
    d = mi.query(a)[0]
    out["floor"] = {"points_exact_room_accuracy_cm": acc * 100, "points_exact_room_completion_cm": comp * 100,
                    "points_room_mesh_samples_cm": float(ni.query(a)[0].mean()) * 100,
                    "mesh_room_mesh_samples_cm": float(d.mean()) * 100, "mesh_room_mesh_samples_max_cm": float(d.max()) * 100}

    shifted = v.clone()
    shifted[:, 2] += 0.01
    out["surface_metrics_ms"] = timed(lambda: recon.surface_metrics((shifted, fc), (v, fc), align=False, n_points=n), args.reps)
    out["calc_3d_metric_ms"] = timed(lambda: recon.calc_3d_metric((shifted, fc), (v, fc), align=False, n_points=n), args.reps)
    m = recon.surface_metrics((shifted, fc), (v, fc), align=False, n_points=n, thresholds=(0.05, 0.01))
    p = recon.calc_3d_metric((shifted, fc), (v, fc), align=False, n_points=n)
    out["shift_1cm"] = {"mesh": {k: (x if not isinstance(x, dict) else {str(t): y for t, y in x.items()}) for k, x in m.items()}, "points": p}
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
