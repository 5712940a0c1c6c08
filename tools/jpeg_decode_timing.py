#!/usr/bin/env python3
"""Timing of the JPEG decoder (nice_slam_amd/jpeg.py, csrc/nsr_jpegdec.h) on the GPU against PIL on the same files; output committed
as profiles/jpeg_decode_timing.json.

    python tools/jpeg_decode_timing.py --out profiles/jpeg_decode_timing.json

Three shapes: one 680 x 1200 frame as Replica stores them (4:2:0, quality 90, no restart markers: one chain), a batch of 8 of
them, and one 960 x 540 replay frame written by ``encode_jpeg`` (a restart interval per MCU row: 34 chains).  Each path is timed
with what it takes to have the pixels on the device: ``decode_jpeg`` (parse, upload of the file, kernels, the status read-back)
against ``Image.open`` + ``np.array(im.convert("RGB"))`` + the upload of the pixels.  The two are timed alternately in one
process after a warm-up of both, a host clock around the call with a device synchronise; medians and ranges (min, max) of the
repeats are reported, ``gpu_faster`` says whether the ranges do not overlap, and the uploaded bytes of both paths are given.  The
single Replica-shaped frame is also decoded at other subsequence sizes, which moves the work between the tiles' serial walk and
the lanes' own decoding.  Every decode is compared with PIL's pixels before it is timed."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import jpeg_reference as R  # noqa: E402
from nice_slam_amd import jpeg  # noqa: E402


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
            out.append(np.array(im.convert("RGB")))
    return torch.from_numpy(np.stack(out)).cuda()


def replica_file(seed):
    """680 x 1200, quality 90, 4:2:0, no restart markers, about 240 KB as a rendered Replica frame is: the recipe image of the
    tests at a third of the size, enlarged (its per-pixel noise at full size would make a file twice as long)"""
    buf = io.BytesIO()
    Image.fromarray(R.recipe_image(227, 400, seed=seed)).resize((1200, 680), Image.BICUBIC).save(buf, "JPEG", quality=90)
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_timing.json"))
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "pillow": Image.__version__, "libjpeg_turbo": features.version("libjpeg_turbo"),
           "subsequence_bytes": 128, "calls": {}}
    replica = [replica_file(k) for k in range(8)]
    replay = jpeg.encode_jpeg(torch.from_numpy(R.recipe_image(540, 960, seed=9)).cuda(), 90, "4:2:0")
    for name, files in (("replica_1_680x1200", replica[:1]), ("replica_8_680x1200", replica), ("replay_1_960x540_encode_jpeg", replay)):
        info = jpeg.probe_jpeg(files[0])
        for _ in range(2):                                           # warm-up of both
            g, p = jpeg.decode_jpeg(files), pil_decode(files)
        assert torch.equal(g, p), name
        tg, tp = [], []
        for _ in range(a.reps):
            tg.append(clock(lambda: jpeg.decode_jpeg(files)))
            tp.append(clock(lambda: pil_decode(files)))
        sg, sp = stats(tg), stats(tp)
        scan = [q["scan_end"] - q["scan_begin"] for q in map(jpeg._parse, files)]
        chains = 1 if not info["restart_interval"] else -(-(-(-info["width"] // 16) * -(-info["height"] // 16)) // info["restart_interval"])
        res["calls"][name] = {"files": len(files), "sampling": info["sampling"], "restart_interval": info["restart_interval"], "chains_per_frame": chains,
                              "scan_bytes": scan, "tiles_per_chain": [-(-s // chains // (1024 * 128)) for s in scan],
                              "gpu": sg, "pil": sp, "gpu_upload_bytes": sum(map(len, files)) + len(files) * jpeg._FRAME_DTYPE.itemsize,
                              "pil_upload_bytes": int(p.numel()), "gpu_faster": sg["max_ms"] < sp["min_ms"],
                              "ratio_of_medians_pil_to_gpu": sp["median_ms"] / sg["median_ms"], "pixels_equal_pil": True}
        print(name, res["calls"][name], flush=True)
    sweep = {}
    want = pil_decode(replica[:1])
    for sb in (32, 64, 128, 256, 512, 1024):
        for _ in range(2):
            assert torch.equal(jpeg.decode_jpeg(replica[:1], subsequence_bytes=sb), want), sb
        sweep[str(sb)] = dict(stats([clock(lambda: jpeg.decode_jpeg(replica[:1], subsequence_bytes=sb)) for _ in range(a.reps)]),
                              tiles=-(-(-(-len(replica[0]) // sb)) // 1024))
        print("subsequence_bytes", sb, sweep[str(sb)], flush=True)
    res["replica_1_by_subsequence_bytes"] = sweep
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
