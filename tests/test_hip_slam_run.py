"""GPU: the runner (nice_slam_amd/slam.py).  A tracked frame reads nothing back from the device; a run from a Replica-layout
folder leaves the reference's run directory (Logger.log's checkpoint, the final meshes), runs the iterations its schedule
implies and holds the trajectory; the command line prints one JSON line."""
import json
import os
import subprocess
import sys
import types
import weakref

import numpy as np
import pytest
import torch

import pose_reference as PR
import slam_run_util as U
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)


def _args(out=None):
    return types.SimpleNamespace(input_folder=None, output=out, nice=True)


def test_a_tracked_frame_reads_nothing_back(tmp_path):
    from nice_slam_amd.slam import NICE_SLAM
    dev = torch.device("cuda", 0)
    seq = U.sequence(dev)
    cfg = U.merged_config(seq, schedule={"iters_first": 60, "iters": 20, "every_frame": 2, "keyframe_every": 4}, output=str(tmp_path / "out"))
    torch.manual_seed(0)
    slam = NICE_SLAM(cfg, _args(), decoders="random", dataset=U.MemorySequence(seq, 4))
    frames = [slam.frame_reader[i] for i in range(4)]
    slam.tracker.track(0, frames[0][1], frames[0][2])
    slam.map_frame(0, frames[0][1], frames[0][2], first=True)                       # a small map
    slam.tracker.track(1, frames[1][1], frames[1][2])                               # one eager iteration and the capture
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        slam.tracker.track(2, frames[2][1], frames[2][2])
        slam.tracker.track(3, frames[3][1], frames[3][2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    hist = slam.tracker._ft["hist"].cpu().numpy()
    est, gt = slam.traj.est.cpu().numpy(), slam.traj.gt.cpu().numpy()
    assert hist.shape == (10, 8) and np.isfinite(hist).all() and slam.counters["tracking_iters"] == 30
    taken = PR.commit_ref(hist)
    assert taken is not None
    PR.gate(est[3], PR.pose_ref(hist[taken, 1:]), "traj[3]")
    assert slam.tracker._ft["best"].cpu().numpy().tobytes() == hist[taken].tobytes()
    assert np.array_equal(est[0], gt[0]) and np.isfinite(est).all()
    for i in (1, 2, 3):                                                             # every frame got a pose of its own, near the truth
        assert np.array_equal(est[i, 3], [0, 0, 0, 1]) and np.abs(est[i, :3, 3] - gt[i, :3, 3]).max() < 0.1, i
    slam.release()
    ref = weakref.ref(slam)
    del slam
    assert ref() is None                                                            # no cycle keeps the captured graph waiting for the collector


def test_bundle_adjustment_separate_rates_global_selection_and_colour_refinement(tmp_path):
    """The paths the 14-frame schedule above never reaches: more than four keyframes (local BA: the window's poses are gathered
    with get_tensor_from_camera and written back by Trajectory.store), 'global' selection, two learning rates in the tracker
    (TUM's seperate_LR), the recorded selections and the colour refinement of the last frame (Mapper.py:578-586)."""
    from nice_slam_amd.slam import NICE_SLAM
    dev = torch.device("cuda", 0)
    seq = U.sequence(dev)
    cfg = U.merged_config(seq, schedule={"iters_first": 200, "iters": 40, "every_frame": 1, "keyframe_every": 2}, output=str(tmp_path / "out"),
                          color_refine=True, keyframe_selection_method="global", save_selected_keyframes_info=True)
    cfg["tracking"]["seperate_LR"] = True
    cfg["coarse"] = False
    cfg["meshing"]["eval_rec"] = False
    torch.manual_seed(0)
    slam = NICE_SLAM(cfg, _args(), decoders="random", dataset=U.MemorySequence(seq))
    res = slam.run()
    # 14 mapped frames: 200, then 12 of 40, then the refinement's 5 calls of 40 * 5 // 5
    assert res["mapping_iters"] == 200 + 12 * 40 + 5 * 40 and res["tracking_iters"] == 130 and res["coarse_iters"] == 0, res
    assert res["keyframe_list"] == [0, 2, 4, 6, 8, 10, 12]
    est, gt = slam.traj.est.cpu().numpy().astype(np.float64), slam.traj.gt.cpu().numpy()
    kf = slam.kf_est[:7].cpu().numpy().astype(np.float64)
    for m in list(est) + list(kf):                                                  # every stored pose is a pose
        assert np.abs(m[:3, :3] @ m[:3, :3].T - np.eye(3)).max() < 1e-5 and np.array_equal(m[3], [0, 0, 0, 1])
    assert np.array_equal(kf[0], gt[0])                                             # the oldest keyframe of a window is never optimised
    moved = [k for k in range(7) if not np.array_equal(kf[k], est[2 * k])]
    assert moved, "bundle adjustment wrote no keyframe pose back"
    assert max(np.abs(kf[k][:3, 3] - gt[2 * k][:3, 3]).max() for k in range(7)) < 0.1
    ckpt = torch.load(os.path.join(str(tmp_path / "out"), "ckpts", "00013.tar"), map_location="cpu", weights_only=False)
    sel = ckpt["selected_keyframes"]
    assert sorted(sel) == list(range(14)) and sel[0] == [{"idx": 0, "gt_c2w": sel[0][0]["gt_c2w"], "est_c2w": sel[0][0]["est_c2w"]}]
    # a window of 5: three older keyframes, the last one, the frame; the refinement's is twice as wide: all seven and the frame
    assert len(sel[12]) == 5 and len(sel[13]) == 8 and sel[13][-1]["idx"] == 13 and sel[13][-2]["idx"] == 12
    print("ATE [cm] with BA, separate rates, global selection:", round(res["ate"]["rmse"] * 100, 3), "moved keyframes:", moved)
    assert res["ate"]["rmse"] * 100 < 3.0                                           # "holds the trajectory" of tests/test_hip_slam_ate.py
    # the system is freed by its reference count, not by the cycle collector (which could destroy a graph during a later capture)
    assert slam.tracker._ft is None
    ref = weakref.ref(slam)
    del slam
    assert ref() is None


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the sequence written once as a folder; three runs of it from its YAML pair, one per seed"""
    from nice_slam_amd.slam import NICE_SLAM, load_config
    root = tmp_path_factory.mktemp("slam_run")
    scene = U.write_folder(U.sequence("cpu"), root)
    out = []
    for sd in SEEDS:
        cfg = load_config(scene)
        torch.manual_seed(sd)
        slam = NICE_SLAM(cfg, _args(str(root / f"out{sd}")), decoders="random", seed=sd)
        out.append((slam, slam.run()))
    return scene, root, out


def test_run_from_a_folder_leaves_the_run_directory(runs):
    from nice_slam_amd import ply, viewer
    from nice_slam_amd.slam import CKPT_KEYS
    scene, root, out = runs
    for sd, (slam, res) in zip(SEEDS, out):
        d = str(root / f"out{sd}")
        assert res["output"] == d and sorted(os.listdir(os.path.join(d, "ckpts"))) == ["00013.tar"]
        ckpt = torch.load(os.path.join(d, "ckpts", "00013.tar"), map_location="cpu", weights_only=False)
        assert tuple(ckpt) == CKPT_KEYS                                             # exactly Logger.log's keys, in its order
        assert ckpt["idx"] == 13 and ckpt["keyframe_list"] == [0, 4, 8, 12] and ckpt["selected_keyframes"] is None
        assert all(not v.is_cuda for v in ckpt["c"].values()) and set(ckpt["c"]) == {"grid_coarse", "grid_middle", "grid_fine", "grid_color"}
        assert list(ckpt["decoder_state_dict"]) == list(slam.shared_decoders.state_dict())
        est, gt = ckpt["estimate_c2w_list"], ckpt["gt_c2w_list"]
        assert tuple(est.shape) == tuple(gt.shape) == (14, 4, 4) and not est.is_cuda
        assert torch.equal(est[0], gt[0]) and torch.equal(gt, torch.stack(slam.frame_reader.poses))
        e, g, n = viewer.load_run(d, 1.0)
        assert e.shape == (14, 4, 4) and g.shape == (14, 4, 4) and n == 13
        assert sorted(os.listdir(os.path.join(d, "mesh"))) == ["00013_mesh.ply", "final_mesh.ply", "final_mesh_eval_rec.ply"]
        for name in ("final_mesh.ply", "00013_mesh.ply", "final_mesh_eval_rec.ply"):
            v, f = ply.read_mesh(os.path.join(d, "mesh", name))[:2]
            assert len(v) > 0 and len(f) > 0, name
        assert open(os.path.join(d, "mesh", "final_mesh.ply"), "rb").read() == open(os.path.join(d, "mesh", "00013_mesh.ply"), "rb").read()


def test_run_counts_and_holds_the_trajectory(runs):
    scene, root, out = runs
    ates = []
    for sd, (slam, res) in zip(SEEDS, out):
        # 8 mapped frames (0, 2, ..., 12 and the last): 400 + 7 * 100; 13 tracked frames of 10 iterations
        assert res["mapping_iters"] == 1100 and res["tracking_iters"] == 130 and res["coarse_iters"] == 1100, (sd, res)
        assert res["keyframe_list"] == [0, 4, 8, 12] and res["n_img"] == 14
        ates.append(res["ate"]["rmse"] * 100)
    print("ATE [cm] of seeds", SEEDS, ":", [round(a, 3) for a in ates], "wall [s]:", [r["wall_s"] for _, r in out])
    assert sorted(ates)[1] < 3.0, ates                                              # the bound of tests/test_hip_slam_ate.py


def test_command_line_prints_one_json_line(runs):
    scene, root, _ = runs
    out = str(root / "out_cli")
    r = subprocess.run([sys.executable, "-m", "nice_slam_amd.slam", scene, "--random-decoders", "--output", out, "--frames", "5"],
                       cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = json.loads(lines[0])
    assert res["n_img"] == 5 and res["ate"]["compared_pose_pairs"] == 5 and np.isfinite(res["ate"]["rmse"]) and res["value"] == res["ate"]["rmse"] * 100
    assert res["tracking_iters"] == 40 and res["mapping_iters"] == 400 + 2 * 100    # frames 0, 2, 4 mapped
    assert os.path.exists(os.path.join(out, "ckpts", "00004.tar"))
    # without --random-decoders the missing checkpoints are an error that names the file
    r2 = subprocess.run([sys.executable, "-m", "nice_slam_amd.slam", scene, "--output", out, "--frames", "2"],
                        cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r2.returncode != 0 and "FileNotFoundError" in r2.stderr and "pretrained/coarse.pt" in r2.stderr
