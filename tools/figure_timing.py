#!/usr/bin/env python3
"""Timing of the rendering figure (nice_slam_amd/csrc/nsr_figure.h) on the GPU; output committed as profiles/figure_timing.json.

    python tools/figure_timing.py --out profiles/figure_timing.json

Per 680 x 1200 frame (Replica's image), one frame and a batch of 8: the launches of ``nsr_figure_sheet`` into buffers that exist
(``hip_launches``), ``imgeval.figure_sheet`` as a user calls it (``hip``: conversions and allocations included), and the same
sheet composed from stock torch operators on the same GPU (``torch``: amax, divide, index_select into the colour map, clamp,
cat).  The three are timed in turn inside one process: a round is ``--calls`` back-to-back calls between two device events, the
time per call is the round's over the calls; medians and the range over ``--rounds`` rounds are recorded.  The bytes the sheet
needs (32 read per source pixel, 3 written per sheet pixel) over the launches' time stand next to the bandwidth of a plain
device copy measured the same way in the same process, and the two sheets are compared byte for byte."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import figure_reference as R  # noqa: E402
from nice_slam_amd import imgeval  # noqa: E402

H, W = 680, 1200
STRIDE, MARGIN, GAP = 1, 8, 8


def torch_sheet(color, gt_color, depth, gt_depth, lut):
    """the sheet of figure_sheet from stock torch operators (stride 1): u8 [B, SH, SW, 3]"""
    B = depth.shape[0]
    vmax = gt_depth.amax((1, 2), keepdim=True)
    valid = gt_depth != 0
    dres = torch.where(valid, (gt_depth - depth).abs(), torch.zeros_like(depth))
    cres = torch.where(valid[..., None], (gt_color - color).abs(), torch.zeros_like(color))

    def cmap(v):
        t = v / vmax
        idx = (t * 256.0).clamp(0.0, 255.0).nan_to_num(0.0).long()
        idx = torch.where(t >= 1.0, torch.full_like(idx, 255), idx)
        idx = torch.where(vmax == 0, torch.zeros_like(idx), idx)
        out = lut.index_select(0, idx.reshape(-1)).reshape(*v.shape, 3)
        return torch.where(torch.isnan(v)[..., None], torch.full_like(out, 255), out)

    def rgb(v):
        return (v.clamp(0.0, 1.0) * 255.0).to(torch.uint8)

    def white(h, w):
        return torch.full((B, h, w, 3), 255, dtype=torch.uint8, device=depth.device)

    rows = []
    for panels in ((cmap(gt_depth), cmap(depth), cmap(dres)), (rgb(gt_color), rgb(color), rgb(cres))):
        rows.append(torch.cat([white(H, MARGIN), panels[0], white(H, GAP), panels[1], white(H, GAP), panels[2], white(H, MARGIN)], 2))
    SW = rows[0].shape[2]
    return torch.cat([white(MARGIN, SW), rows[0], white(GAP, SW), rows[1], white(MARGIN, SW)], 1)


def rounds_of(fns, rounds, calls):
    """{name: [ms per call, ...]}: the callables in turn, ``rounds`` rounds of ``calls`` back-to-back calls between two events"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / calls)
    return times


def summary(ms, frames):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "per_frame_ms": float(np.median(ms)) / frames, "rounds": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "figure_timing.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("figure_timing needs the GPU")
    E = imgeval.gpu()
    lut = torch.from_numpy(R.LUT).cuda()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "layout": {"stride": STRIDE, "margin": MARGIN, "gap": GAP},
           "calls_per_round": a.calls, "sheet": {}}
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for B in (1, 8):
        imgs = [torch.from_numpy(x).cuda() for x in R.make_images(B, H, W, seed=B)]
        SH, SW = imgeval.figure_sheet_size(H, W, STRIDE, MARGIN, GAP)
        sheet = torch.empty((B, SH, SW, 3), dtype=torch.uint8, device="cuda")
        vmax = torch.empty(B, dtype=torch.float32, device="cuda")
        keep = {}

        def launches():
            E.call("nsr_figure_sheet", *(x.data_ptr() for x in imgs), B, H, W, STRIDE, MARGIN, GAP, vmax.data_ptr(), sheet.data_ptr())

        fns = {"hip_launches": launches,
               "hip": lambda: keep.__setitem__("hip", imgeval.figure_sheet(*imgs, STRIDE, MARGIN, GAP)),
               "torch": lambda: keep.__setitem__("torch", torch_sheet(*imgs, lut)),
               "copy_256MiB": lambda: dst.copy_(src)}
        t = rounds_of(fns, a.rounds, a.calls)
        entry = {k: summary(v, B) for k, v in t.items()}
        bytes_needed = 32 * B * H * W + 3 * B * SH * SW
        entry["bytes_needed"] = bytes_needed
        entry["hip_launches_GB_per_s"] = bytes_needed / (entry["hip_launches"]["median_ms"] * 1e-3) / 1e9
        entry["copy_GB_per_s"] = 2 * src.numel() / (entry["copy_256MiB"]["median_ms"] * 1e-3) / 1e9          # read + written
        entry["speedup_hip_launches_over_torch"] = entry["torch"]["median_ms"] / entry["hip_launches"]["median_ms"]
        entry["speedup_hip_over_torch"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        entry["differing_bytes_hip_vs_torch"] = int((keep["hip"] != keep["torch"]).sum())
        entry["differing_bytes_launches_vs_function"] = int((sheet != keep["hip"]).sum())
        res["sheet"][f"batch_{B}"] = entry
        print(B, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
