"""What a tracked frame costs with the pose algebra on the host and with it on the device.

The tiny sequence of tests/perf/ate_study.py (14 frames, 120 x 160, its schedule) is run, alternating in one process after a
warm-up of both, by
  (a) tools/slam_synthetic.MiniSLAM on the fused path: the trajectory is a list of host tensors; per tracked frame the motion
      model and the quaternion are numpy (``tracking_pose_s``), 7 floats go up (``tracking_reset_s``) and the history of the
      iterations comes back for an argmin on the host (``tracking_wait_s``, which also holds the GPU's time for the iterations);
  (b) nice_slam_amd.slam.NICE_SLAM on the same frames held in memory: the trajectory is device memory, a tracked frame is one
      graph replay and reads nothing back.
Both wait for the device after every tracked frame HERE, so that a frame's wall time can be taken at all ((b) never waits by
itself).  Writes profiles/slam_run_timing.json: the median wall time per tracked frame of each, the spread over the repeats,
and (a)'s split.

    python tools/slam_run_timing.py [--repeats 7] [--out profiles/slam_run_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "perf"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slam_run_timing.json"))
    args = ap.parse_args()
    import tempfile
    import torch
    import ate_study
    import slam_synthetic as ss
    import slam_run_util as U
    from nice_slam_amd.slam import NICE_SLAM
    dev = torch.device("cuda", 0)
    seq, cfg_a, init = ate_study.setup(dev)
    mem = U.MemorySequence(seq)
    tmp = tempfile.mkdtemp(prefix="slam_run_timing_")
    cfg_b = U.merged_config(seq, output=os.path.join(tmp, "out"))
    cfg_b["coarse"] = False                                   # MiniSLAM's runs of this schedule have no coarse mapper either
    cfg_b["meshing"]["eval_rec"] = False
    n_tracked = ate_study.FRAMES - 1

    def run_a(sd):                                            # tests/perf/ate_compare.run("fused", ...), keeping the unrounded timers
        t0 = time.perf_counter()
        torch.manual_seed(sd)
        ops = ss.ProductOps(seq, dev, seed=sd, fused=True)
        with torch.no_grad():
            for k, v in init["grids"].items():
                ops.c[k].copy_(v.to(dev))
            ops.decoders.load_state_dict({k: v.to(dev) for k, v in init["params"].items()})
        mini = ss.MiniSLAM(ops, seq, cfg_a, seed=sd)
        r = dict(mini.run(), **mini.timers)
        torch.cuda.synchronize()
        return {"tracked_frame_ms": 1e3 * r["tracking_s"] / n_tracked, "wall_s": time.perf_counter() - t0, "ate_cm": r["ate"]["rmse"] * 100,
                "split_ms_per_frame": {k: 1e3 * r.get(k, 0.0) / n_tracked for k in ("tracking_pose_s", "tracking_reset_s", "tracking_refresh_s",
                                                                                    "tracking_launch_s", "tracking_wait_s")},
                "capture_s": r["tracking_capture_s"]}

    def run_b(sd):
        torch.manual_seed(sd)
        t0 = time.perf_counter()
        slam = NICE_SLAM(cfg_b, types.SimpleNamespace(input_folder=None, output=None, nice=True), decoders="random", dataset=mem, seed=sd,
                         sync_timers=True)
        r = slam.run()
        # the first tracked frame holds the capture and is listed apart: every other one is in track_frame_s
        return {"tracked_frame_ms": 1e3 * statistics.mean(slam.track_frame_s), "tracked_frame_median_ms": 1e3 * statistics.median(slam.track_frame_s),
                "wall_s": time.perf_counter() - t0, "ate_cm": r["ate"]["rmse"] * 100, "capture_s": r["tracking_capture_s"],
                "log_s": r["log_s"], "mesh_s": r["mesh_s"]}

    run_a(0), run_b(0)                                        # warm-up of both: code objects, allocator pools
    a, b = [], []
    for k in range(args.repeats):
        a.append(run_a(k))
        b.append(run_b(k))

    def spread(v):
        v = sorted(v)
        return {"median": statistics.median(v), "min": v[0], "max": v[-1], "values": v}

    res = {"sequence": [ate_study.FRAMES, ate_study.HEIGHT, ate_study.WIDTH], "schedule": ate_study.SCHEDULE, "repeats": args.repeats,
           "tracked_frames_per_run": n_tracked, "tracking_iters_per_frame": cfg_a["tracking"]["iters"],
           "note": "ms of wall time per tracked frame, the device waited for after every frame in both; (a) averages its run's 13 frames less "
                   "the capture, (b) its 12 frames behind the capture",
           "minislam_host_poses": {"tracked_frame_ms": spread([r["tracked_frame_ms"] for r in a]),
                                   "split_ms_per_frame": {k: spread([r["split_ms_per_frame"][k] for r in a]) for k in a[0]["split_ms_per_frame"]},
                                   "ate_cm": spread([r["ate_cm"] for r in a]), "wall_s": spread([r["wall_s"] for r in a])},
           "runner_device_poses": {"tracked_frame_ms": spread([r["tracked_frame_ms"] for r in b]),
                                   "tracked_frame_median_ms": spread([r["tracked_frame_median_ms"] for r in b]),
                                   "ate_cm": spread([r["ate_cm"] for r in b]), "wall_s": spread([r["wall_s"] for r in b]),
                                   "log_s": spread([r["log_s"] for r in b]), "mesh_s": spread([r["mesh_s"] for r in b])}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({"minislam_ms": res["minislam_host_poses"]["tracked_frame_ms"]["median"],
                      "runner_ms": res["runner_device_poses"]["tracked_frame_ms"]["median"],
                      "minislam_split_ms": {k: v["median"] for k, v in res["minislam_host_poses"]["split_ms_per_frame"].items()}}))


if __name__ == "__main__":
    main()
