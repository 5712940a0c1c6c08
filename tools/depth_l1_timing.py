#!/usr/bin/env python3
"""Timing of the depth rasterizer and the 2-D depth metric (nice_slam_amd/raster.py) on the GPU; output committed as
profiles/depth_l1_timing.json.

    python tools/depth_l1_timing.py --out profiles/depth_l1_timing.json

Scenes: the analytic room of tests/raster_reference.py (a 5 x 4 x 3 m box and a table block), tessellated into ~1M and ~2M
triangles.  Measured: one 500 x 500 view (the binning call and the resolve call apart, and together), a batch of 64 views,
the view test of 64 candidates against a 1M-point cloud, and calc_2d_metric end to end with 1000 views on two ~1M-triangle
meshes (the reconstruction: the room with its floor raised by 2 cm)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_reference as R  # noqa: E402
from nice_slam_amd import raster  # noqa: E402
from nice_slam_amd.engine import gpu, pose_stack, w2c_rows  # noqa: E402


def room(scale):
    v, f = R.box_mesh([0.0, 0.0, 0.0], [5.0, 4.0, 3.0], (5 * scale, 4 * scale, 3 * scale))
    tv, tf = R.box_mesh([1.2, 1.0, 0.0], [2.8, 2.0, 0.75], (16, 10, 6))
    return np.concatenate([v, tv]), np.concatenate([f, tf + len(v)]).astype(np.int32)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def split(v, f, c2w, near):
    """(bin ms, depth ms) of one call each, library entry points timed apart with events"""
    E = gpu()
    lib = E.lib
    vt = torch.from_numpy(v.astype(np.float32)).cuda()
    ft = torch.from_numpy(f).cuda()
    w2c = torch.from_numpy(w2c_rows(pose_stack(c2w), np.float64)).cuda()
    K = w2c.shape[0]
    ws = torch.empty(int(lib.nsr_raster_workspace_bytes(len(v), len(f), K, 500, 500)), dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    out = torch.empty((K, 500, 500), dtype=torch.float32, device="cuda")
    args = (500, 500, 300.0, 300.0, 249.5, 249.5, float(near), 20.0)
    b = lambda: lib.check(lib.nsr_raster_bin(vt.data_ptr(), len(v), ft.data_ptr(), len(f), w2c.data_ptr(), K, *args, ws.data_ptr(),  # noqa: E731
                                             n.data_ptr(), E.stream()), "bin")
    b()
    torch.cuda.synchronize()
    bins = torch.empty(int(n.item()), dtype=torch.int32, device="cuda")
    d = lambda: lib.check(lib.nsr_raster_depth(vt.data_ptr(), len(v), ft.data_ptr(), len(f), w2c.data_ptr(), K, *args, ws.data_ptr(),  # noqa: E731
                                               bins.data_ptr(), bins.numel(), out.data_ptr(), E.stream()), "depth")
    return timed(b), timed(d), int(n.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_l1_timing.json"))
    ap.add_argument("--n_imgs", type=int, default=1000)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "image": [500, 500], "renders": []}
    rng = np.random.default_rng(0)
    eyes = rng.uniform([0.5, 0.5, 0.9], [4.5, 3.5, 2.6], (64, 3))
    c2w = np.stack([R.look_from(e, e + rng.normal(size=3)) for e in eyes])
    for scale in (73, 103):
        v, f = room(scale)
        vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        one = timed(lambda: raster.render_depth(vt, ft, c2w[:1]))
        b64 = timed(lambda: raster.render_depth(vt, ft, c2w), reps=3)
        bin_ms, depth_ms, n1 = split(v, f, c2w[:1], 0.05)
        bin64, depth64, n64 = split(v, f, c2w, 0.05)
        res["renders"].append({"triangles": int(len(f)), "vertices": int(len(v)), "render_1_view_ms": one,
                               "bin_1_view_ms": bin_ms, "resolve_1_view_ms": depth_ms, "entries_1_view": n1,
                               "render_64_views_ms": b64, "per_view_ms_at_64": b64 / 64, "bin_64_views_ms": bin64,
                               "resolve_64_views_ms": depth64, "entries_64_views": n64})
        print(res["renders"][-1], flush=True)
    pts = np.concatenate([rng.uniform([-4.0, 4.1, 0.0], [9.0, 4.5, 3.0], (1_000_000, 3))])
    pts_t = torch.from_numpy(pts).cuda()
    res["view_test_1M_points_64_candidates_ms"] = timed(lambda: raster.views_unseen(c2w, pts_t))
    print("view test", res["view_test_1M_points_64_candidates_ms"], flush=True)
    gv, gf = room(73)
    rv = gv.copy()
    rv[rv[:, 2] == 0.0, 2] = 0.02
    gvt, gft, rvt = torch.from_numpy(gv).cuda(), torch.from_numpy(gf).cuda(), torch.from_numpy(rv).cuda()
    for align in (False, True):
        torch.cuda.synchronize()
        t = time.perf_counter()
        m = raster.calc_2d_metric((rvt, gft), (gvt, gft), align=align, n_imgs=a.n_imgs, unseen=pts_t)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        res[f"calc_2d_metric_{a.n_imgs}_views_align_{align}"] = {"seconds": dt, "depth_l1_cm": m["depth_l1_cm"],
                                                                 "triangles": int(len(gf))}
        print("metric", align, dt, m["depth_l1_cm"], flush=True)
    # where the end-to-end time goes: the pieces of one run, timed apart
    E = gpu()
    t = time.perf_counter()
    ext, tr = raster.cam_position(gvt, gft)
    res["cam_position_s"] = time.perf_counter() - t
    t = time.perf_counter()
    poses = raster.sample_views(ext, tr, a.n_imgs, pts_t, 0, engine=E)
    res["sample_views_s"] = time.perf_counter() - t
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k0 in range(0, len(poses), 100):
        d0 = raster.render_depth(gvt, gft, poses[k0:k0 + 100])
        d1 = raster.render_depth(rvt, gft, poses[k0:k0 + 100])
        raster.depth_l1(d0, d1)
    torch.cuda.synchronize()
    res["render_and_l1_s"] = time.perf_counter() - t
    print(res, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
