#!/usr/bin/env python3
"""Timing of the frame preparation (nice_slam_amd/datasets.py) on the GPU against the host path it replaces; output committed
as profiles/frame_timing.json.

    python tools/frame_timing.py --out profiles/frame_timing.json

Per frame, at two shapes -- a Replica frame (680 x 1200, nothing but / 255 and the depth scale) and a TUM frame (480 x 640,
distortion, crop_size 384 x 512, crop_edge 8):

  prepare       FramePreparer.prepare on the decoded host arrays: the upload of the raw bytes (u8 colour, u16 depth) and the
                launches, a host clock around the call and a device synchronise;
  host          what BaseDataset.__getitem__ (src/utils/datasets.py:77-113) does after the decode, restated in numpy / torch
                fp64 on this machine's CPU (tests/frames_reference.py), plus the upload of its fp64 colour and fp32 depth, timed
                the same way;
  kernels_only  prepare on arrays that are already on the device, device events around the call.

The two paths are timed alternately inside one process after a warm-up, the medians and the spread of the repeats are recorded,
and their results on the timed input are compared.  The file decode (PIL here, cv2 there) is in neither figure."""
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

import frames_reference as R  # noqa: E402
from nice_slam_amd.datasets import FramePreparer  # noqa: E402


def summary(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "repeats": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_timing.json"))
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_timing needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(), "shapes": {}}
    for name in R.BIG_CASES:
        cfg, color, depth, bgr = R.build_case(name)
        color, depth = color[0], depth[0]
        prep = FramePreparer(cfg)
        keep = {}

        def gpu_path():
            keep["gpu"] = prep.prepare(color, depth, bgr=bgr)
            torch.cuda.synchronize()

        def host_path():
            ref = R.prepare(color, depth, cfg, bgr)
            keep["host"] = (torch.from_numpy(ref["color64"]).cuda(), torch.from_numpy(ref["depth"]).cuda())
            torch.cuda.synchronize()

        times = {"prepare": [], "host": [], "kernels_only": []}
        for fn in (gpu_path, host_path):                # warm-up: code objects, the allocator's blocks
            fn()
            fn()
        dc, dd = torch.from_numpy(color).cuda(), torch.from_numpy(depth.view(np.int16)).cuda()
        prep.prepare(dc, dd, bgr=bgr)
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for key, fn in (("prepare", gpu_path), ("host", host_path)):
                t0 = time.perf_counter()
                fn()
                times[key].append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            prep.prepare(dc, dd, bgr=bgr)
            e1.record()
            e1.synchronize()
            times["kernels_only"].append(e0.elapsed_time(e1))
        entry = {k: summary(v) for k, v in times.items()}
        entry["speedup_prepare_over_host"] = entry["host"]["median_ms"] / entry["prepare"]["median_ms"]
        entry["upload_bytes"] = {"prepare": int(color.nbytes + depth.nbytes),
                                 "host": int(keep["host"][0].numel() * 8 + keep["host"][1].numel() * 4)}
        entry["max_abs_colour_difference"] = float((keep["gpu"][0].double() - keep["host"][0]).abs().max())
        entry["depth_bit_identical"] = bool(torch.equal(keep["gpu"][1], keep["host"][1]))
        entry["out_size"] = list(keep["gpu"][1].shape)
        res["shapes"][name] = entry
        print(name, entry, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
