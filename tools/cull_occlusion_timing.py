#!/usr/bin/env python3
"""Timing of the occlusion-aware cull (nice_slam_amd/raster.py visibility_counts, recon.cull_masks(occlusion=True)) on the GPU;
output committed as profiles/cull_occlusion_timing.json.

    python tools/cull_occlusion_timing.py --out profiles/cull_occlusion_timing.json
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/cull_occlusion_timing.py --profile_run     # per-kernel shares of (c)

Scene: the analytic room of tests/raster_reference.py (a 5 x 4 x 3 m box and a table block) tessellated into ~1M triangles, its
~0.5M vertices tested against 200 poses at 680 x 1200 (cull_mesh.py's camera; rendered at 340 x 600).  Measured, each as the
median of alternating runs (b, c, b, c, ...) after a warm-up of both:
  (a) the frustum-only cull (recon.cull_masks), for context;
  (b) the stock composition, written here: render_depth of all views, then the contract's test as torch gathers;
  (c) the new path (recon.cull_masks(occlusion=True): rasterize a batch of views, one points_visible launch, next batch);
with the peak device memory of (b) and (c), and of (c) again at half of the poses: it is bounded by one batch (at most 64
views), not by K."""
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
from nice_slam_amd import raster, recon  # noqa: E402
from nice_slam_amd.engine import pose_stack, w2c_rows  # noqa: E402

H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5
EPS = 0.03


def room(scale):
    v, f = R.box_mesh([0.0, 0.0, 0.0], [5.0, 4.0, 3.0], (5 * scale, 4 * scale, 3 * scale))
    tv, tf = R.box_mesh([1.2, 1.0, 0.0], [2.8, 2.0, 0.75], (16, 10, 6))
    return np.concatenate([v, tv]), np.concatenate([f, tf + len(v)]).astype(np.int32)


def stock_counts(vt, ft, c2w, near, far=1e3, chunk=8):
    """the contract of points_visible_kernel on stock kernels: every view's depth image first, then gathers"""
    m = raster.raster_divisor(H, W)
    Hs, Ws, fx, fy, cx, cy = raster.scaled_camera(H, W, FX, FY, CX, CY, m)
    depth = raster.render_depth(vt, ft, c2w, Hs, Ws, fx, fy, cx, cy, near=near, far=far)          # [K, Hs, Ws]
    w = torch.from_numpy(w2c_rows(pose_stack(c2w), np.float64)).to(vt.device).reshape(-1, 3, 4)
    p = vt.float()
    count = torch.zeros(len(p), dtype=torch.int32, device=vt.device)
    for k0 in range(0, len(w), chunk):
        wk = w[k0:k0 + chunk]                                                                     # [k, 3, 4]
        cam = ((wk[:, None, :, 0] * p[None, :, None, 0] + wk[:, None, :, 1] * p[None, :, None, 1])
               + wk[:, None, :, 2] * p[None, :, None, 2]) + wk[:, None, :, 3]                     # [k, N, 3] fp32
        x, y, z = cam[..., 0].double(), cam[..., 1].double(), cam[..., 2].double()
        i = torch.floor(((x / z) * fx + cx) + 0.5)
        j = torch.floor(((y / z) * fy + cy) + 0.5)
        ok = (z >= near) & (z <= far) & (i >= 0) & (i < Ws) & (j >= 0) & (j < Hs)
        idx = torch.where(ok, j * Ws + i, torch.zeros_like(i)).long()
        d = torch.gather(depth[k0:k0 + chunk].reshape(len(wk), -1), 1, idx)
        vis = ok & ((d == 0) | (z <= d.double() + EPS))
        count += vis.sum(0).to(torch.int32)
    return count


def run(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_occlusion_timing.json"))
    ap.add_argument("--scale", type=int, default=73, help="room tessellation (73: ~1M triangles)")
    ap.add_argument("--views", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile_run", action="store_true", help="one warm-up and one run of (c) only, for a kernel trace")
    a = ap.parse_args()
    v, f = room(a.scale)
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    rng = np.random.default_rng(0)
    eyes = rng.uniform([0.5, 0.5, 0.9], [4.5, 3.5, 2.6], (a.views, 3))
    c2w = np.stack([R.look_from(e, e + rng.normal(size=3)) for e in eyes])
    loaded = c2w.copy()                                # as load_poses returns them: y and z axes flipped, float32
    loaded[:, :3, 1] *= -1
    loaded[:, :3, 2] *= -1
    poses = [torch.from_numpy(p).float() for p in loaded]
    opencv = pose_stack(poses, flip_yz=True)
    near = raster.NEAR_REL * raster.max_extent(vt)

    new = lambda n=a.views: recon.cull_masks(vt, ft, poses[:n], occlusion=True, eps=EPS)[0]      # noqa: E731
    if a.profile_run:
        new(8)
        seen, dt, _ = run(new)
        print("profile run: (c) %.3f s, %d of %d vertices seen" % (dt, int(seen.sum()), len(v)), flush=True)
        return
    stock = lambda: stock_counts(vt, ft, opencv, near) >= 1                                         # noqa: E731
    frustum = lambda: recon.cull_masks(vt, ft, poses)[0]                                            # noqa: E731
    for fn in (frustum, stock, new):                   # warm-up of every shape
        fn()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "rendered_at": list(raster.scaled_camera(H, W, FX, FY, CX, CY, 2)[:2]),
           "triangles": int(len(f)), "vertices": int(len(v)), "views": a.views, "eps": EPS,
           "max_views_per_launch": raster.MAX_VIEWS_PER_LAUNCH, "order": "a, then b c b c ...",
           "stock_s": [], "new_s": [], "stock_peak_bytes": [], "new_peak_bytes": []}
    seen_a, res["frustum_only_s"], _ = run(frustum)
    for _ in range(a.reps):
        seen_b, dt, peak = run(stock)
        res["stock_s"].append(dt)
        res["stock_peak_bytes"].append(peak)
        seen_c, dt, peak = run(new)
        res["new_s"].append(dt)
        res["new_peak_bytes"].append(peak)
        print("b %.3f s  c %.3f s" % (res["stock_s"][-1], res["new_s"][-1]), flush=True)
    res["stock_median_s"], res["new_median_s"] = float(np.median(res["stock_s"])), float(np.median(res["new_s"]))
    res["stock_and_new_disagree_on"] = int((seen_b != seen_c).sum())
    res["seen_frustum_only"], res["seen_with_occlusion"] = int(seen_a.sum()), int(seen_c.sum())
    _, res["new_half_of_the_views_s"], res["new_half_of_the_views_peak_bytes"] = run(lambda: new(a.views // 2))
    print(res, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
