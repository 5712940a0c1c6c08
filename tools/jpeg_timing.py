#!/usr/bin/env python3
"""Timing of the JPEG encoder (nice_slam_amd/jpeg.py) on the GPU against PIL on the same pixels; output committed as
profiles/jpeg_timing.json.

    python tools/jpeg_timing.py --out profiles/jpeg_timing.json

Encoder calls: batches of 1 and 8 replay frames at 960 x 540 and one figure sheet of 680 x 1200 inputs (1384 x 3632), each with
what it takes to have the files' bytes on the host: ``encode_jpeg`` (kernels, two read-backs) against the read-back of the pixels
and ``Image.save(quality=90)`` into memory.  The two are timed alternately in one process, after a warm-up of both; medians and
ranges (min, max) of the repeats are reported, and ``gpu_faster`` says whether the ranges do not overlap.

Replay: the 2000-frame replay of tools/view_timing.py (four ~250k-triangle meshes, 960 x 540) through ``viewer.replay_run`` with
``encoder="pil"``, ``encoder="gpu"`` and ``video="vis.avi"``, alternating, in one process, on one run directory."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import raster_reference as R  # noqa: E402
from nice_slam_amd import imgeval, jpeg, viewer  # noqa: E402
from nice_slam_amd.ply import write_ply  # noqa: E402

H, W = viewer.HEIGHT, viewer.WIDTH


def room(scale):
    v, f = R.box_mesh([0.0, 0.0, 0.0], [5.0, 4.0, 3.0], (5 * scale, 4 * scale, 3 * scale))
    tv, tf = R.box_mesh([1.2, 1.0, 0.0], [2.8, 2.0, 0.75], (16, 10, 6))
    return np.concatenate([v, tv]), np.concatenate([f, tf + len(v)]).astype(np.int32)


def walk(frames, rng):
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
    return est, gt


def stats(ts):
    return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": float(min(ts)) * 1e3, "max_ms": float(max(ts)) * 1e3, "repeats": len(ts)}


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def pil_encode(batch):
    out = []
    for img in batch.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=90)
        out.append(buf.getvalue())
    return out


def encoder_calls(res, reps):
    rng = np.random.default_rng(0)
    est, gt = walk(64, rng)
    rp = viewer.Replay(est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt)
    v, f = room(36)
    rp.update_mesh((v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8)))
    for i in range(8):
        rp.update_pose(1, est[8 * i], gt=False)
        rp.update_pose(1, gt[8 * i], gt=True)
        rp.update_cam_trajectory(8 * i, gt=False)
        rp.snapshot()
    frames = rp.flush()
    y, x = np.mgrid[0:680, 0:1200].astype(np.float32)
    color = np.stack([0.5 + 0.5 * np.sin(x / 17 + y / 29), 0.5 + 0.5 * np.cos(x / 23 - y / 13), 0.5 + 0.5 * np.sin(x / 11) * np.cos(y / 19)], -1)
    depth = (2.0 + np.sin(x / 90) + np.cos(y / 70)).astype(np.float32)
    noise = rng.normal(scale=0.03, size=color.shape).astype(np.float32)
    sheet = imgeval.figure_sheet(color + noise, color, depth + noise[..., 0], depth)
    res["calls"] = {}
    for name, batch in (("frames_1_960x540", frames[:1]), ("frames_8_960x540", frames), ("sheet_1_680x1200_inputs", sheet[None])):
        batch = batch.contiguous()
        for _ in range(2):                                       # warm-up of both
            g, p = jpeg.encode_jpeg(batch), pil_encode(batch)
        tg, tp = [], []
        for _ in range(reps):
            tg.append(clock(lambda: jpeg.encode_jpeg(batch)))
            tp.append(clock(lambda: pil_encode(batch)))
        sg, sp = stats(tg), stats(tp)
        res["calls"][name] = {"shape": list(batch.shape), "gpu": sg, "pil": sp, "gpu_bytes": sum(map(len, g)), "pil_bytes": sum(map(len, p)),
                              "gpu_faster": sg["max_ms"] < sp["min_ms"], "ratio_of_medians_pil_to_gpu": sp["median_ms"] / sg["median_ms"]}
        print(name, res["calls"][name], flush=True)


def replays(res, frames, rounds):
    rng = np.random.default_rng(1)
    est, gt = walk(frames, rng)
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
        modes = {"pil": dict(encoder="pil"), "gpu": dict(encoder="gpu"), "video": dict(video="vis.avi")}
        times = {k: [] for k in modes}
        sizes = {}
        viewer.replay_run(d, 1.0, every=max(1, frames // 64), encoder="gpu")            # warm-up: code objects, the allocator
        for _ in range(rounds):
            for k, kw in modes.items():
                n = [0]
                times[k].append(clock(lambda: n.__setitem__(0, viewer.replay_run(d, 1.0, **kw))))
                assert n[0] == frames
                sizes[k] = sum(os.path.getsize(os.path.join(d, "tmp_rendering", p)) for p in os.listdir(os.path.join(d, "tmp_rendering")))
        sizes["vis.avi"] = os.path.getsize(os.path.join(d, "vis.avi"))
    out = {"frames": frames, "mesh_triangles": int(tris), "meshes": len(range(0, frames, 500)), "jpeg_bytes": sizes}
    for k, ts in times.items():
        out[k] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "rounds": len(ts)}
    out["gpu_faster"] = out["gpu"]["max_s"] < out["pil"]["min_s"]
    out["video_faster"] = out["video"]["max_s"] < out["pil"]["min_s"]
    res["replay"] = out
    print(out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_timing.json"))
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "quality": 90, "subsampling": "4:2:0"}
    encoder_calls(res, a.reps)
    replays(res, a.frames, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
