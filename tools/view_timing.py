#!/usr/bin/env python3
"""Timing of the replay view (nice_slam_amd/viewer.py) on the GPU; output committed as profiles/view_timing.json.

    python tools/view_timing.py --out profiles/view_timing.json

Scene: the analytic room of tools/depth_l1_timing.py at ~1M triangles, 960 x 540.  Measured: the mesh layer (render_mesh, back
faces culled, vertex colours) for 1 and 64 views beside render_depth on the same mesh and views in the same run (the ratio is
reported; the reference's Open3D window cannot run here, so there is no baseline), vertex normals, the point layer for 64 frames
of 4400 points each over one shared base, and a 2000-frame replay end to end (four ~250k-triangle meshes, one every 500 frames)
with its rendering and its JPEG writing timed apart."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_reference as R  # noqa: E402
from nice_slam_amd import raster, viewer  # noqa: E402
from nice_slam_amd.ply import write_ply  # noqa: E402

H, W = viewer.HEIGHT, viewer.WIDTH


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


def replay(frames, res):
    rng = np.random.default_rng(1)
    est = np.zeros((frames, 4, 4))
    for i in range(frames):
        a = 2 * np.pi * i / frames
        eye = np.array([2.5 + 1.5 * np.cos(a), 2.0 + 1.0 * np.sin(a), 1.5])
        m = R.look_from(eye, eye + [-np.sin(a), np.cos(a), -0.1])
        m[:3, 1] *= -1
        m[:3, 2] *= -1
        est[i] = m
    gt = est.copy()
    gt[:, :3, 3] += rng.normal(scale=0.01, size=(frames, 3))
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "mesh"))
        os.makedirs(os.path.join(d, "ckpts"))
        tris = 0
        for i in range(0, frames, 500):
            v, f = room(36)
            tris = len(f)
            write_ply(os.path.join(d, "mesh", f"{i:05d}_mesh.ply"), v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
        torch.save({"estimate_c2w_list": torch.from_numpy(est).float(), "gt_c2w_list": torch.from_numpy(gt).float(), "idx": frames - 1},
                   os.path.join(d, "ckpts", "00000.tar"))
        torch.cuda.synchronize()
        t = time.perf_counter()
        n = viewer.replay_run(d, 1.0)
        torch.cuda.synchronize()
        total = time.perf_counter() - t
        # the same walk without the files: what is left is mesh loading, scene assembly and the kernels
        e, g, N = viewer.load_run(d, 1.0)
        t = time.perf_counter()
        rp = viewer.Replay(e[0], cam_scale=0.3, estimate_c2w_list=e, gt_c2w_list=g)
        for i in range(N + 1):
            mf = os.path.join(d, "mesh", f"{i:05d}_mesh.ply")
            if os.path.isfile(mf):
                rp.update_mesh(mf)
            rp.update_pose(1, e[i], gt=False)
            rp.update_pose(1, g[i], gt=True)
            if i % 10 == 0:
                rp.update_cam_trajectory(i, gt=False)
                rp.update_cam_trajectory(i, gt=True)
            rp.snapshot()
            if (i + 1) % viewer.FRAMES_PER_LAUNCH == 0:
                rp.flush()
        rp.flush()
        torch.cuda.synchronize()
        render = time.perf_counter() - t
    res["replay"] = {"frames": int(n), "mesh_triangles": int(tris), "meshes": len(range(0, frames, 500)), "total_s": total,
                     "render_only_s": render, "jpeg_and_copy_s": total - render, "frames_per_s": n / total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_timing.json"))
    ap.add_argument("--frames", type=int, default=2000)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W]}
    rng = np.random.default_rng(0)
    cam = viewer.default_camera(H, W)
    eyes = rng.uniform([0.5, 0.5, 0.9], [4.5, 3.5, 2.6], (64, 3))
    c2w = np.stack([R.look_from(e, e + rng.normal(size=3)) for e in eyes])
    v, f = room(73)
    f = f[:, ::-1].copy()                         # as Replay leaves a mesh: seen from inside, the walls face the camera
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    col = torch.from_numpy(rng.integers(0, 256, (len(v), 3), dtype=np.uint8)).cuda()
    res["triangles"], res["vertices"] = int(len(f)), int(len(v))
    res["vertex_normals_ms"] = timed(lambda: viewer.vertex_normals(vt, ft))
    nrm = viewer.vertex_normals(vt, ft)
    for K in (1, 64):
        mesh = timed(lambda: viewer.render_mesh(vt, ft, c2w[:K], H, W, *cam, colors=col, normals=nrm, cull="back", near=0.05), reps=3)
        nocull = timed(lambda: viewer.render_mesh(vt, ft, c2w[:K], H, W, *cam, colors=col, normals=nrm, near=0.05), reps=3)
        depth = timed(lambda: raster.render_depth(vt, ft, c2w[:K], H, W, *cam, near=0.05, far=1000.0), reps=3)
        res[f"views_{K}"] = {"render_mesh_cull_back_ms": mesh, "render_mesh_no_cull_ms": nocull, "render_depth_ms": depth,
                             "ratio_no_cull_to_depth": nocull / depth, "ratio_cull_back_to_depth": mesh / depth}
        print(K, res[f"views_{K}"], flush=True)
    rgb, depth, _ = viewer.render_mesh(vt, ft, c2w[:1], H, W, *cam, colors=col, normals=nrm, cull="back", near=0.05)
    pts = torch.from_numpy(rng.uniform([0.0, 0.0, 0.0], [5.0, 4.0, 3.0], (64 * 4400, 3))).cuda()
    pcol = torch.from_numpy(rng.integers(0, 256, (64 * 4400, 3), dtype=np.uint8)).cuda()
    offsets = np.arange(65) * 4400
    views = np.repeat(c2w[:1], 64, 0)
    res["points_64_frames_4400_ms"] = timed(lambda: viewer.draw_points(rgb[0], depth[0], pts, pcol, offsets, views, *cam, near=0.05))
    print("points", res["points_64_frames_4400_ms"], flush=True)
    replay(a.frames, res)
    print(res["replay"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
