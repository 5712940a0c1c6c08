#!/usr/bin/env python3
"""Timing of the rendering evaluation (nice_slam_amd/imgeval.py) on the GPU; output committed as
profiles/render_eval_timing.json.

    python tools/render_eval_timing.py --out profiles/render_eval_timing.json

Per 680 x 1200 frame (Replica's image): the metrics launch of nice_slam_amd.image_metrics (with and without the residual maps,
one frame and a batch of 8), the same metrics written with stock torch operators on the same GPU (fp32, separable Gaussian by
two grouped conv2d), and Renderer.render_img itself on the Replica-sized test scene.  The two metric implementations are timed
alternately inside one process (device events around each call), the medians and the spread of the repeats are recorded, and
their results on the timed input are compared."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import imgmetrics_reference as R  # noqa: E402
from nice_slam_amd import imgeval  # noqa: E402

H, W = 680, 1200


def torch_metrics(color, gt_color, depth, gt_depth, residuals=False):
    """the metrics of image_metrics from stock torch operators, fp32 images, fp64 sums: [B] tensors"""
    a, b = color.clamp(0.0, 1.0), gt_color.clamp(0.0, 1.0)
    valid = gt_depth != 0
    sq = ((a - b) ** 2).double().sum(-1)
    n_valid = valid.sum((1, 2)).double()
    out = {"psnr": -10.0 * torch.log10(sq.sum((1, 2)) / (3.0 * sq[0].numel())),
           "psnr_valid": -10.0 * torch.log10((sq * valid).sum((1, 2)) / (3.0 * n_valid)),
           "depth_l1_cm": 100.0 * ((gt_depth - depth).abs().double() * valid).sum((1, 2)) / n_valid,
           "depth_max": gt_depth.amax((1, 2))}
    g = torch.exp(-((torch.arange(R.WIN, device=a.device, dtype=torch.float32) - R.WIN // 2) ** 2) / (2 * R.SIGMA ** 2))
    g = g / g.sum()
    x, y = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
    m = torch.cat([x, y, x * x, y * y, x * y], 1)                                   # [B, 15, H, W]
    m = F.conv2d(m, g.view(1, 1, 1, -1).expand(15, 1, 1, -1), groups=15)
    m = F.conv2d(m, g.view(1, 1, -1, 1).expand(15, 1, -1, 1), groups=15)
    mx, my, xx, yy, xy = m.split(3, 1)
    vx, vy, vxy = xx - mx * mx, yy - my * my, xy - mx * my
    s = ((2 * mx * my + R.C1) * (2 * vxy + R.C2)) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2))
    out["ssim"] = s.double().mean((1, 2, 3))
    if residuals:
        out["depth_residual"] = (gt_depth - depth).abs() * valid
        out["color_residual"] = (gt_color - color).abs() * valid[..., None]
    return out


def alternate(fns, reps):
    """{name: [ms, ...]} of the callables run in turn, ``reps`` rounds, device events around each call"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    return times


def summary(ms, frames):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
            "per_frame_ms": float(np.median(ms)) / frames, "repeats": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_eval_timing.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--render-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_eval_timing needs the GPU")
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "metrics": {}}
    for B in (1, 8):
        imgs = [torch.from_numpy(x).cuda() for x in R.make_images(B, H, W, seed=B)]
        ws = {}
        fns = {"hip": lambda: ws.__setitem__("hip", imgeval.image_metrics(*imgs)),
               "hip_residuals": lambda: ws.__setitem__("hipr", imgeval.image_metrics(*imgs, residuals=True)),
               "torch": lambda: ws.__setitem__("torch", torch_metrics(*imgs)),
               "torch_residuals": lambda: ws.__setitem__("torchr", torch_metrics(*imgs, residuals=True))}
        t = alternate(fns, a.reps)
        entry = {k: summary(v, B) for k, v in t.items()}
        entry["max_abs_difference_hip_vs_torch"] = {k: float((ws["hip"][k].double() - ws["torch"][k].double()).abs().nan_to_num().max())
                                                    for k in ("psnr", "psnr_valid", "ssim", "depth_l1_cm", "depth_max")}
        entry["speedup_hip_over_torch"] = entry["torch"]["median_ms"] / entry["hip"]["median_ms"]
        res["metrics"][f"batch_{B}"] = entry
        print(B, entry, flush=True)
        del imgs, ws
    # render_img on the Replica-sized test scene, one frame at its own pose, then its evaluation
    from scene_util import make_scene, build_product
    sc = make_scene(seed=6, small=False, n_rays=16)
    renderer, dec, grids = build_product(sc, "cuda:0")
    gt_depth, gt_color, c2w = sc["depth_img"].cuda(), sc["color_img"].cuda(), sc["c2w"].cuda()
    out = {}
    with torch.no_grad():
        t = alternate({"render_img": lambda: out.__setitem__("r", renderer.render_img(grids, dec, c2w, "cuda:0", "color", gt_depth=gt_depth))},
                      a.render_reps)
    res["render_img"] = summary(t["render_img"], 1)
    depth, _, color = out["r"]
    t0 = time.perf_counter()
    ev = imgeval.evaluate_rendering(renderer, grids, dec, [(0, gt_color, gt_depth, c2w)], device="cuda:0")
    torch.cuda.synchronize()
    res["evaluate_rendering_1_frame_ms"] = (time.perf_counter() - t0) * 1e3
    res["evaluate_rendering_means"] = ev["mean"]
    res["metrics_share_of_an_evaluated_frame"] = res["metrics"]["batch_1"]["hip"]["median_ms"] / (
        res["render_img"]["median_ms"] + res["metrics"]["batch_1"]["hip"]["median_ms"])
    print(res["render_img"], res["evaluate_rendering_means"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
