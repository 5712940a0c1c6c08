#!/usr/bin/env python3
"""Timing of the PNG decoder (nice_slam_amd/png.py, csrc/nsr_png.h) on the GPU against PIL on the same files; output committed as
profiles/png_decode_timing.json.

    python tools/png_decode_timing.py --out profiles/png_decode_timing.json

Four shapes: one 680 x 1200 16-bit depth frame as Pillow writes it (Replica's shape), batches of 8 and of 32 of them, and one
480 x 640 RGB frame (TUM RGB-D's shape).  Each path is timed with what it takes to have the pixels on the device: ``decode_png``
(the chunk walk with its CRCs, the upload of the compressed bytes, the kernels, the status read-back) against ``Image.open`` +
``np.array`` + the upload of the pixels.  The two are timed alternately in one process after a warm-up of both, a host clock around
the call with a device synchronise; medians and ranges (min, max) of the repeats are reported, ``gpu_faster`` says whether the
ranges do not overlap, and the uploaded bytes of both paths are given.  Every decode is compared with PIL's pixels before it is
timed."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nice_slam_amd import png  # noqa: E402


def stats(ts):
    return {"median_ms": float(np.median(ts)) * 1e3, "min_ms": float(min(ts)) * 1e3, "max_ms": float(max(ts)) * 1e3, "repeats": len(ts)}


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def pil_decode(files):
    out = []
    for f in files:
        with Image.open(io.BytesIO(f)) as im:
            a = np.array(im)
        out.append(a.view(np.int16) if a.dtype == np.uint16 else a)      # (u16 travels as its bytes, as FramePreparer takes them)
    return torch.from_numpy(np.stack(out)).cuda()


def saved(a):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    return buf.getvalue()


def depth_file(seed):
    """680 x 1200 u16 millimetres: a room of a few planes and a curved surface with sensor-like noise of a few millimetres on half
    of the pixels (a rendered Replica frame has none and is smaller; a TUM frame has more)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:680, 0:1200].astype(np.float64)
    wall = 2500 + 0.6 * x + 0.2 * y
    floor = 5200 - 5.5 * y
    blob = 1800 + 0.002 * ((x - 500 - 20 * seed) ** 2 + (y - 300) ** 2)
    d = np.minimum(np.minimum(wall, np.maximum(floor, 900)), blob)
    d += (rng.random(d.shape) < 0.5) * rng.integers(-3, 4, d.shape)
    return saved(d.astype(np.uint16))


def colour_file(seed):
    """480 x 640 RGB: smooth shading with texture noise"""
    rng = np.random.default_rng(100 + seed)
    y, x = np.mgrid[0:480, 0:640].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 90 + k) * np.cos(y / 70 - k) for k in range(3)], -1)
    return saved(np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_timing.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    import zlib
    res = {"device": torch.cuda.get_device_name(0), "pillow": Image.__version__, "zlib": zlib.ZLIB_RUNTIME_VERSION, "calls": {}}
    depth = [depth_file(k) for k in range(32)]
    for name, files in (("depth_1_680x1200_u16", depth[:1]), ("depth_8_680x1200_u16", depth[:8]), ("depth_32_680x1200_u16", depth),
                        ("colour_1_480x640_rgb", [colour_file(0)])):
        info = png.probe_png(files[0])
        for _ in range(2):                                           # warm-up of both
            g, p = png.decode_png(files), pil_decode(files)
        assert torch.equal(g.view(p.dtype), p), name
        tg, tp = [], []
        for _ in range(a.reps):
            tg.append(clock(lambda: png.decode_png(files)))
            tp.append(clock(lambda: pil_decode(files)))
        sg, sp = stats(tg), stats(tp)
        streams = [sum(map(len, png.parse_png(f)["idat"])) for f in files]
        res["calls"][name] = {"files": len(files), "kind": info["kind"], "height": info["height"], "width": info["width"],
                              "file_bytes": [len(f) for f in files], "gpu": sg, "pil": sp,
                              "gpu_upload_bytes": sum(streams) + len(files) * png.FRAME_DTYPE.itemsize,
                              "pil_upload_bytes": int(p.numel() * p.element_size()), "gpu_faster": sg["max_ms"] < sp["min_ms"],
                              "ratio_of_medians_pil_to_gpu": sp["median_ms"] / sg["median_ms"], "pixels_equal_pil": True}
        print(name, res["calls"][name], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
