"""Phase times of the mesh bound from keyframes (nice_slam_amd.bound) on the GPU: touch, integrate, extract, pre-filter, host
hull, and the point-in-hull test over 256^3 / 512^3 lattices, for 8 and 200 keyframes of a Replica-sized (680 x 1200) analytic
room (tests/bound_reference.py).  Writes profiles/bound_timing.json.

    python tools/bound_timing.py [--out profiles/bound_timing.json] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bound_reference as R  # noqa: E402
from nice_slam_amd import bound  # noqa: E402

H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5
DEV = "cuda:0"


def phases(kfs):
    marks = []

    def tick(name):
        torch.cuda.synchronize()
        marks.append((name, time.perf_counter()))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = bound.bound_from_frames(kfs, H, W, FX, FY, CX, CY, 1.0, 1.02, timer=tick)
    out, prev = {}, t0
    for name, t in marks:
        out[name] = (t - prev) * 1e3
        prev = t
    out["total"] = (prev - t0) * 1e3
    return out, b


def contains_ms(b, res, reps):
    ax = [torch.linspace(float(R.ROOM_LO[d]) - 0.3, float(R.ROOM_HI[d]) + 0.3, res, dtype=torch.float64, device=DEV) for d in range(3)]
    yy, xx, zz = torch.meshgrid(ax[1], ax[0], ax[2], indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1).float()
    del xx, yy, zz
    b.contains(pts[:1000])
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        inside = b.contains(pts)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(inside.float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "scale": 1.0, "bound_scale": 1.02,
           "note": "ms per phase (median of reps after one warm-up); timer marks are synchronised, so phases do not overlap; "
                   "'touch' includes the depth upload and the unit box / bitmap passes, 'hull' is host C++ in libnsr.so",
           "runs": []}
    for n in (8, 200):
        kfs = R.room_keyframes(n, H, W, FX, FY, CX, CY, seed=11, holes=False)
        gk = [{"est_c2w": torch.from_numpy(k["est_c2w"]).float().to(DEV), "depth": torch.from_numpy(k["depth"]).to(DEV)} for k in kfs]
        phases(gk)                                                  # warm-up
        reps = [phases(gk) for _ in range(args.reps)]
        b = reps[-1][1]
        med = {k: float(np.median([r[0][k] for r in reps])) for k in reps[0][0]}
        run = {"keyframes": n, "phases_ms": med, "stats": b.stats, "planes": int(b.planes.shape[0])}
        for lat in (256, 512):
            ms, frac = contains_ms(b, lat, args.reps)
            run[f"contains_{lat}_ms"] = ms
            run[f"contains_{lat}_inside_fraction"] = frac
        print(json.dumps(run), flush=True)
        res["runs"].append(run)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
