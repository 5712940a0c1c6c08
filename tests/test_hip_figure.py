"""GPU tests of the rendering figure (nice_slam_amd/csrc/nsr_figure.h, nice_slam_amd/imgeval.py) and of the runner's figures
(nice_slam_amd/slam.py): the emulator test's batches and one 680 x 1200 frame against the numpy restatement
(tests/figure_reference.py) byte for byte; Visualizer.vis on the small scene against figure_sheet of render_img's own output;
one 14-frame run with the tracker's and the mapper's figures on (the files, the tracker's figure poses, the run's counters),
and a short run with the figures off whose tracked frames still read nothing back."""
import os
import types

import numpy as np
import pytest
import torch

import figure_reference as R
import pose_reference as PR
import slam_run_util as U
from nice_slam_amd import imgeval

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def imgs():
    return R.main_case()


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: "s%d_m%d_g%d" % l)
def test_sheet_matches_restatement(imgs, layout):
    R.assert_main_case_holds_its_cases(imgs)
    got, vmax = imgeval.figure_sheet(*imgs, *layout, return_vmax=True)
    want, want_vmax = R.expected_sheet(*imgs, *layout)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert vmax.cpu().numpy().tobytes() == want_vmax.tobytes()
    diff = int((got.cpu().numpy() != want).sum())
    print(f"layout {layout}: sheet {want.shape}, {diff} differing bytes")
    assert diff == 0
    assert torch.equal(imgeval.figure_sheet(*imgs, *layout), got)                        # two runs, the same bytes
    assert torch.equal(imgeval.figure_sheet(*(x[[2, 0, 1]] for x in imgs), *layout), got[[2, 0, 1]])


@pytest.mark.parametrize("hw", R.SMALL, ids=lambda s: "%dx%d" % s)
def test_small_images_match_restatement(hw):
    im = R.make_images(3, *hw, seed=11)
    for layout in R.LAYOUTS:
        want, _ = R.expected_sheet(*im, *layout)
        assert np.array_equal(imgeval.figure_sheet(*im, *layout).cpu().numpy(), want), layout


def test_replica_sized_frame_and_no_vmax_buffer():
    im = R.make_images(1, 680, 1200, seed=2)
    im[2][0, 5, 7], im[2][0, 9, 11] = np.nan, np.inf
    want, want_vmax = R.expected_sheet(*im)
    dev = [torch.from_numpy(x).cuda() for x in im]
    got, vmax = imgeval.figure_sheet(*dev, return_vmax=True)
    assert tuple(got.shape) == (1, 2 * 8 + 2 * 680 + 8, 2 * 8 + 3 * 1200 + 2 * 8, 3) and vmax.cpu().numpy().tobytes() == want_vmax.tobytes()
    diff = int((got.cpu().numpy() != want).sum())
    print("680 x 1200:", diff, "differing bytes of", want.size)
    assert diff == 0
    m = imgeval.image_metrics(*dev)
    assert m["depth_max"].cpu().numpy().tobytes() == want_vmax.tobytes()
    # the C entry without vmax_out: the maxima live in the sheet's own memory until the last launch
    E = imgeval.gpu()
    out = torch.zeros_like(got)
    E.call("nsr_figure_sheet", *(x.data_ptr() for x in dev), 1, 680, 1200, 1, 8, 8, None, out.data_ptr())
    assert torch.equal(out, got)
    # the colour map alone, with the frame's own maximum and with a given one
    assert np.array_equal(imgeval.colorize_depth(dev[3]).cpu().numpy(), R.colormap(im[3], want_vmax[0]))
    assert np.array_equal(imgeval.colorize_depth(dev[2], vmax=vmax).cpu().numpy(), R.colormap(im[2], want_vmax[0]))


def test_visualizer_on_the_small_scene(tmp_path):
    from PIL import Image
    from scene_util import make_scene, build_product
    from nice_slam_amd.poses import get_tensor_from_camera
    sc = make_scene(seed=6, small=True)
    renderer, dec, grids = build_product(sc, "cuda:0")
    gt_color, gt_depth, c2w = sc["color_img"].cuda(), sc["depth_img"].cuda(), sc["c2w"].cuda()
    vis = imgeval.Visualizer(1, 1, str(tmp_path / "vis"), renderer, False, "cuda:0")
    sheet = vis.vis(3, 7, gt_depth, gt_color, c2w, grids, dec)
    depth, _, color = renderer.render_img(grids, dec, c2w, "cuda:0", "color", gt_depth=gt_depth)
    assert depth.dtype == torch.float64                                                   # the figure takes it as fp32
    want = imgeval.figure_sheet(color, gt_color, depth, gt_depth)
    assert tuple(sheet.shape) == (1,) + tuple(want.shape) and torch.equal(sheet[0], want)
    ref, _ = R.expected_sheet(color.cpu().numpy()[None], gt_color.cpu().numpy()[None], depth.float().cpu().numpy()[None], gt_depth.cpu().numpy()[None])
    assert np.array_equal(want.cpu().numpy(), ref[0])
    with Image.open(tmp_path / "vis" / "00003_0007.jpg") as im:
        assert im.size == (want.shape[1], want.shape[0])
    # a camera tensor goes through get_camera_from_tensor: the same picture up to the pose's rounding; and two poses in one launch
    cam = get_tensor_from_camera(c2w[None])[0]
    both = vis.vis_many(4, [0, 1], [c2w, cam], gt_depth, gt_color, grids, dec)
    assert tuple(both.shape) == (2,) + tuple(want.shape) and torch.equal(both[0], want)
    assert sorted(os.listdir(tmp_path / "vis")) == ["00003_0007.jpg", "00004_0000.jpg", "00004_0001.jpg"]


def _args(out=None):
    return types.SimpleNamespace(input_folder=None, output=out, nice=True)


def test_run_draws_the_tracking_and_mapping_figures(tmp_path):
    from nice_slam_amd.slam import NICE_SLAM
    dev = torch.device("cuda", 0)
    seq = U.sequence(dev)
    out = str(tmp_path / "out")
    cfg = U.merged_config(seq, output=out, vis_freq=2, vis_inside_freq=50)
    cfg["tracking"].update(vis_freq=1, vis_inside_freq=5, no_vis_on_first_frame=False)
    cfg["meshing"]["eval_rec"] = False
    torch.manual_seed(0)
    slam = NICE_SLAM(cfg, _args(), decoders="random", dataset=U.MemorySequence(seq))
    assert slam.tracker.keep_start and slam.coarse_mapper.visualizer is None
    seen, real = [], slam.tracker.visualizer.vis_many

    def spy(idx, iters, poses, *a):
        ft = slam.tracker._ft
        if idx > 0:
            seen.append((idx, list(iters), [p.clone() for p in poses], ft["start"].clone(), ft["hist"].clone(), slam.traj.est.clone()))
        return real(idx, iters, poses, *a)

    slam.tracker.visualizer.vis_many = spy
    res = slam.run()
    # the counters of tests/test_hip_slam_run.py::test_run_counts_and_holds_the_trajectory
    assert res["mapping_iters"] == 1100 and res["tracking_iters"] == 130 and res["coarse_iters"] == 1100, res
    assert res["keyframe_list"] == [0, 4, 8, 12] and res["n_img"] == 14
    want = ["00000_0000.jpg"] + [f"{i:05d}_{it:04d}.jpg" for i in range(1, 14) for it in (0, 5)]
    assert sorted(os.listdir(os.path.join(out, "tracking_vis"))) == want
    # mapped: 0, 2, ..., 12 and 13; even ones are due; frame 0 is left out by mapping.no_vis_on_first_frame; 100 iterations: 0 and 50
    assert cfg["mapping"]["no_vis_on_first_frame"] and cfg["mapping"]["iters"] == 100
    want = [f"{i:05d}_{it:04d}.jpg" for i in range(2, 14, 2) for it in (0, 50)]
    assert sorted(os.listdir(os.path.join(out, "mapping_vis"))) == want
    assert slam.tracker.visualizer.drawn == 27 and slam.mapper.visualizer.drawn == 12
    # the tracker's figure poses: the motion model's vector, then the pose after iteration 4
    assert [s[0] for s in seen] == list(range(1, 14)) and all(s[1] == [0, 5] for s in seen)
    for idx, _, poses, start, hist, est in seen:
        assert torch.equal(poses[0], start) and torch.equal(poses[1], hist[4, 1:]) and not torch.equal(start, hist[0, 1:])
        cam, _ = PR.predict_ref(est.cpu().numpy(), idx, cfg["tracking"]["const_speed_assumption"])
        PR.gate(start.cpu().numpy(), cam, f"start of frame {idx}")                     # (the gate of tests/test_hip_pose.py's predict check)
    print("ATE [cm] with the figures on:", round(res["ate"]["rmse"] * 100, 3), "wall [s]:", res["wall_s"])


def test_figures_off_a_tracked_frame_reads_nothing_back(tmp_path):
    from nice_slam_amd.slam import NICE_SLAM
    dev = torch.device("cuda", 0)
    seq = U.sequence(dev)
    cfg = U.merged_config(seq, schedule={"iters_first": 60, "iters": 20, "every_frame": 2, "keyframe_every": 4}, output=str(tmp_path / "out"))
    assert cfg["tracking"]["vis_freq"] == 50 and cfg["mapping"]["vis_freq"] == 50
    torch.manual_seed(0)
    slam = NICE_SLAM(cfg, _args(), decoders="random", dataset=U.MemorySequence(seq, 4))
    assert not slam.tracker.keep_start
    frames = [slam.frame_reader[i] for i in range(4)]
    slam.tracker.track(0, frames[0][1], frames[0][2])
    slam.map_frame(0, frames[0][1], frames[0][2], first=True)
    slam.tracker.track(1, frames[1][1], frames[1][2])
    assert slam.tracker._ft["start"] is None                                              # the graph was captured without the copy
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        slam.tracker.track(2, frames[2][1], frames[2][2])
        slam.tracker.track(3, frames[3][1], frames[3][2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert slam.counters["tracking_iters"] == 30 and np.isfinite(slam.traj.est.cpu().numpy()).all()
    assert os.listdir(os.path.join(str(tmp_path / "out"), "tracking_vis")) == [] and slam.tracker.visualizer.drawn == 0
    assert os.listdir(os.path.join(str(tmp_path / "out"), "mapping_vis")) == [] and slam.mapper.visualizer.drawn == 0
    slam.release()
