#!/usr/bin/env python3
"""Timing of the trajectory evaluation (nice_slam_amd/csrc/nsr_trajeval.h) on the GPU; output committed as
profiles/traj_eval_timing.json, its numbers quoted in DESIGN.md 3.17.

    python tools/traj_eval_timing.py --out profiles/traj_eval_timing.json

On one trajectory of ``--frames`` poses held on the device (2 000: a Replica sequence), timed in turn inside one process:
  hip_launch        ``nsr_ate_eval`` of the whole trajectory into a record that exists, between two device events
  hip_curve_launch  the same launch with one problem per prefix 0..k, k = 1 .. frames - 1
  hip_plot_launch   ``nsr_ate_plot`` (432 x 576) into an image that exists
  hip               ``evaluate_ate(...).dict()`` as a user calls it: allocation, launch and the read-back of one record; wall clock
  hip_curve         ``ate_curve(...).rmse.cpu()``; wall clock
  host              what the runner does today: both pose lists read back, then ``slam.ate_rmse`` in numpy; wall clock
  host_curve        ``slam.ate_rmse`` on every prefix of the lists read back once (one round: it takes seconds)
A launch round is ``--calls`` back-to-back calls between two events; a wall-clock round is one call between two synchronisations;
medians and the range over ``--rounds`` rounds are recorded, and the two sides' numbers are compared."""
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

import trajeval_reference as R  # noqa: E402
from nice_slam_amd import slam, trajeval  # noqa: E402
from nice_slam_amd.engine import gpu  # noqa: E402


def event_rounds(fn, rounds, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def wall_rounds(fn, rounds, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "rounds": int(len(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_eval_timing.json"))
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("traj_eval_timing needs the GPU")
    E = gpu()
    n = a.frames
    est_h, gt_h = R.walk(n, 11)
    est, gt = torch.from_numpy(est_h).cuda(), torch.from_numpy(gt_h).cuda()
    last = torch.tensor([n - 1], dtype=torch.int64, device="cuda")
    lasts = torch.arange(1, n, dtype=torch.int64, device="cuda")
    rec = torch.empty((1, trajeval.REC), dtype=torch.float64, device="cuda")
    recs = torch.empty((n - 1, trajeval.REC), dtype=torch.float64, device="cuda")
    img = torch.empty((trajeval.PLOT_H, trajeval.PLOT_W, 3), dtype=torch.uint8, device="cuda")
    keep = {}

    def plot():
        E.call("nsr_ate_plot", est.data_ptr(), gt.data_ptr(), n, last.data_ptr(), 1.0, rec.data_ptr(), trajeval.PLOT_H, trajeval.PLOT_W, img.data_ptr())

    res = {"device": torch.cuda.get_device_name(0), "frames": n, "calls_per_round": a.calls}
    res["hip_launch"] = summary(event_rounds(lambda: trajeval._launch(E, est, gt, last, 1.0, rec), a.rounds, a.calls))
    res["hip_curve_launch"] = summary(event_rounds(lambda: trajeval._launch(E, est, gt, lasts, 1.0, recs), a.rounds, max(1, a.calls // 4)))
    res["hip_plot_launch"] = summary(event_rounds(plot, a.rounds, a.calls))
    res["hip"] = summary(wall_rounds(lambda: keep.__setitem__("hip", trajeval.evaluate_ate(est, gt).dict()), a.rounds))
    res["hip_curve"] = summary(wall_rounds(lambda: keep.__setitem__("hip_curve", trajeval.ate_curve(est, gt, lasts).rmse.cpu().numpy()), a.rounds))
    res["host"] = summary(wall_rounds(lambda: keep.__setitem__("host", slam.ate_rmse(est.cpu().numpy(), gt.cpu().numpy())), a.rounds))

    def host_curve():
        e, g = est.cpu().numpy(), gt.cpu().numpy()
        keep["host_curve"] = np.array([slam.ate_rmse(e[:k + 1], g[:k + 1])["rmse"] for k in range(1, n)])

    res["host_curve"] = summary(wall_rounds(host_curve, 1, warm=0))
    res["rmse_hip"], res["rmse_host"] = keep["hip"]["absolute_translational_error.rmse"], keep["host"]["rmse"]
    res["curve_max_abs_difference"] = float(np.abs(keep["hip_curve"] - keep["host_curve"]).max())
    res["speedup_hip_over_host"] = res["host"]["median_ms"] / res["hip"]["median_ms"]
    res["speedup_hip_curve_over_host_curve"] = res["host_curve"]["median_ms"] / res["hip_curve"]["median_ms"]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
