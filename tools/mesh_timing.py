#!/usr/bin/env python3
"""Phase-by-phase timing of mesh extraction (nice_slam_amd.Mesher.get_mesh) on one MI355X, at 256^3 and 512^3 over the
Replica room0 bound, on two fields:

  decoder   Mesher.get_mesh on a scene_util scene (random grids and decoders at Replica room0 shapes), forecast path
            (show_forecast=True: lattice masks, coarse + fine queries) and default path (fine query, masks over vertices)
  analytic  a room (walls, floor, ceiling, a table and two spheres) as an occupancy-like field computed on the device:
            the same library phases without the decoder query

Each configuration runs once for warm-up, then `--reps` timed runs; a phase ends with torch.cuda.synchronize().
Writes JSON (median ms per phase, V and F) to --out.
    python tools/mesh_timing.py --out profiles/mesh_timing.json [--res 256 512] [--reps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
ROOM0_MC_BOUND = [[-2.9, 8.9], [-3.2, 5.5], [-3.3, 8.3]]      # configs/Replica/room0.yaml mapping.marching_cubes_bound


class PhaseTimer:
    def __init__(self):
        self.t = {}
        self.last = None

    def start(self):
        torch.cuda.synchronize()
        self.last = time.perf_counter()

    def __call__(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.t[name] = self.t.get(name, 0.0) + (now - self.last) * 1e3
        self.last = now


def poses(center, n=8):
    out = []
    for k in range(n):
        a = 2 * np.pi * k / n
        c = np.eye(4, dtype=np.float32)
        c[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=np.float32)
        c[:3, 3] = center
        out.append(torch.from_numpy(c))
    return out


def make_mesher(res, sc=None):
    from nice_slam_amd import Mesher
    from scene_util import build_product
    renderer, dec, grids = build_product(sc, DEV)
    H, W, fx, fy, cx, cy = sc["intr"]
    cfg = {"coarse": True, "scale": 1.0, "occupancy": True,
           "meshing": {"resolution": res, "level_set": 0.0, "clean_mesh_bound_scale": 1.02, "remove_small_geometry_threshold": 0.2,
                       "color_mesh_extraction_method": "direct_point_query", "get_largest_components": False, "depth_test": False},
           "mapping": {"marching_cubes_bound": ROOM0_MC_BOUND}}
    slam = types.SimpleNamespace(renderer=renderer, bound=sc["bound"], nice=True, verbose=False, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy)
    return Mesher(cfg, None, slam), dec, grids


def decoder_field(res, reps, show_forecast, depth_test):
    from scene_util import make_scene
    sc = make_scene(seed=31, n_rays=16, scene="replica_room0", fine_scale=1.0)
    m, dec, grids = make_mesher(res, sc)
    m.depth_test = depth_test
    center = sc["bound"].mean(1).numpy().astype(np.float32)
    kfs = [{"est_c2w": c, "depth": sc["depth_img"]} for c in poses(center)]
    est = torch.stack([k["est_c2w"] for k in kfs])
    z = m.eval_points(m.get_grid_uniform(64, DEV)["grid_points"], dec, grids, "fine", DEV)[:, 3]
    m.level_set = float(torch.quantile(z[z < 100], 0.5))
    runs = []
    with tempfile.TemporaryDirectory() as td:
        for r in range(reps + 1):
            pt = PhaseTimer()
            pt.start()
            t0 = time.perf_counter()
            v, f, _ = m.get_mesh(os.path.join(td, "m.ply"), grids, dec, kfs, est, len(kfs) - 1, DEV, show_forecast=show_forecast,
                                 timer=pt)
            total = (time.perf_counter() - t0) * 1e3
            if r:
                runs.append(dict(pt.t, total=total))
    return summarise(runs, V=int(v.shape[0]), F=int(f.shape[0]), keyframes=len(kfs), level_set=m.level_set)


def room_field(res):
    b = np.array(ROOM0_MC_BOUND)
    xyz = [np.linspace(b[i][0] - 0.05, b[i][1] + 0.05, res) for i in range(3)]
    X, Y, Z = torch.meshgrid(*[torch.tensor(a, dtype=torch.float32, device=DEV) for a in xyz], indexing="ij")
    inner = torch.stack([X - (b[0][0] + 0.3), (b[0][1] - 0.3) - X, Y - (b[1][0] + 0.3), (b[1][1] - 0.3) - Y,
                         Z - (b[2][0] + 0.3), (b[2][1] - 0.3) - Z]).min(0).values
    f = -inner                                                                     # occupied outside the inner room box
    table = torch.stack([0.8 - (X - 3.0).abs(), 0.5 - (Y + 1.5).abs(), 0.6 - (Z - 2.0).abs()]).min(0).values
    s1 = 0.7 - torch.sqrt((X - 6.0) ** 2 + (Y - 1.0) ** 2 + (Z - 5.0) ** 2)
    s2 = 0.4 - torch.sqrt((X - 1.0) ** 2 + (Y - 2.5) ** 2 + (Z - 6.5) ** 2)
    f = torch.maximum(torch.maximum(f, table), torch.maximum(s1, s2))
    return f.contiguous(), xyz


def analytic_field(res, reps):
    from nice_slam_amd import marching_cubes
    from nice_slam_amd.mesher import keep_components, point_masks_raw
    from nice_slam_amd.ply import write_ply
    H, W, fx, fy, cx, cy = 680, 1200, 600.0, 600.0, 599.5, 339.5
    cams = poses(np.array([3.0, 1.0, 2.5], np.float32))
    depths = [torch.full((H, W), 4.0) for _ in cams]
    runs = []
    with tempfile.TemporaryDirectory() as td:
        for r in range(reps + 1):
            pt = PhaseTimer()
            pt.start()
            vol, xyz = room_field(res)
            pt("field")
            pts = torch.stack(torch.meshgrid(*[torch.tensor(a, device=DEV) for a in (xyz[1], xyz[0], xyz[2])], indexing="ij"), -1)
            pts = pts[..., [1, 0, 2]].reshape(-1, 3).float()
            code = point_masks_raw(pts, cams, depths, H, W, fx, fy, cx, cy, 1, 500000)
            pt("masks")
            del pts
            v, f = marching_cubes(vol, 0.0, [a[2] - a[1] for a in xyz], [a[0] for a in xyz])
            pt("marching_cubes")
            vc = point_masks_raw(v, cams, depths, H, W, fx, fy, cx, cy, 1, 500000)
            f = f[~(vc != 1)[f.long()].all(1)]
            v, f = keep_components(v, f, False, 0.2)
            pt("clean")
            write_ply(os.path.join(td, "room.ply"), v.cpu().numpy(), f.cpu().numpy())
            pt("export")
            if r:
                runs.append(dict(pt.t, total=sum(pt.t.values())))
    return summarise(runs, V=int(v.shape[0]), F=int(f.shape[0]), seen_lattice_share=float((code == 1).float().mean()))


def summarise(runs, **extra):
    keys = runs[0].keys()
    return dict({k + "_ms": float(np.median([r[k] for r in runs])) for k in keys}, reps=len(runs), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.json"))
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "bound": ROOM0_MC_BOUND,
           "method": "warm-up run, then the median of --reps runs; torch.cuda.synchronize() at each phase boundary", "runs": {}}
    for res in a.res:
        out["runs"][f"decoder_forecast_{res}"] = decoder_field(res, a.reps, True, True)
        print(res, "decoder forecast", out["runs"][f"decoder_forecast_{res}"], flush=True)
        out["runs"][f"decoder_default_{res}"] = decoder_field(res, a.reps, False, True)
        print(res, "decoder default", out["runs"][f"decoder_default_{res}"], flush=True)
        out["runs"][f"analytic_room_{res}"] = analytic_field(res, a.reps)
        print(res, "analytic", out["runs"][f"analytic_room_{res}"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
