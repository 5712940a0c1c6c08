"""GPU tests of the point-visibility kernel and what is built on it (nice_slam_amd/csrc/nsr_raster.h points_visible_kernel,
raster.visibility_counts / unseen_points, recon.cull_masks(occlusion=True)): counts of a 20k-vertex room and pillar over
several batches of views, on an image wide enough to be rendered at half scale, against the numpy restatement
(tests/occlusion_reference.py) bit for bit and run to run; the ``cull --occlusion`` and ``unseen`` commands end to end."""
import numpy as np
import pytest
import torch

import occlusion_reference as O
import raster_reference as R
from nice_slam_amd import raster, recon
from nice_slam_amd.engine import pose_stack

pytestmark = pytest.mark.gpu

# a strip 1200 pixels wide (over the rasterizer's 1024: rendered at 1 / 2 scale, 20 x 600) with a tall pixel, so that it
# still covers the room from floor to ceiling
H, W, FX, FY, CX, CY = 40, 1200, 500.0, 18.0, 599.5, 19.5
CAM = (H, W, FX, FY, CX, CY)
EYES = ([0.5, 2.0, 1.5], [4.4, 0.6, 1.0], [1.0, 3.4, 2.4], [3.6, 3.5, 0.6], [2.5, 0.5, 2.0], [4.5, 2.1, 1.4], [1.2, 0.7, 0.4])
TARGETS = ([2.5, 2.0, 1.5], [2.5, 2.0, 1.2], [2.5, 2.0, 0.5], [0.0, 0.0, 1.5], [2.5, 4.0, 1.0], [2.5, 2.0, 1.5], [5.0, 4.0, 3.0])


def test_counts_match_restatement():
    v, f, _ = O.room_and_pillar((72, 58, 43), (6, 6, 30))
    assert 19_000 < len(v) < 22_000 and len(v) % 256 != 0
    c2w = np.stack([R.look_from(e, t) for e, t in zip(EYES, TARGETS)])
    near, eps = 0.05, 0.03
    assert raster.raster_divisor(H, W) == 2
    got = raster.visibility_counts(v, v, f, c2w, *CAM, eps=eps, near=near, views_per_launch=3)      # batches of 3, 3 and 1
    assert got.dtype == torch.int32 and got.is_cuda
    got = got.cpu().numpy()
    want = O.visibility_counts(v, v, f, c2w, *CAM, eps, near)
    assert np.array_equal(got, want)
    frustum = O.frustum_counts(v, c2w, *CAM, near)
    assert want.max() >= 4 and (want < frustum).sum() > 1000 and (want > 0).sum() > 1000
    again = raster.visibility_counts(v, v, f, c2w, *CAM, eps=eps, near=near, views_per_launch=3).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    # the batch size does not change a count; fp32 points that are the vertices' own rounding neither
    one = raster.visibility_counts(v.astype(np.float32), v, f, c2w, *CAM, eps=eps, near=near).cpu().numpy()
    assert np.array_equal(one, got)


def test_commands(tmp_path):
    from nice_slam_amd.ply import read_mesh, write_ply
    v, f, _ = O.room_and_pillar((20, 16, 12), (4, 4, 12))
    c2w = np.stack([R.look_from(e, t) for e, t in zip(EYES[:4], TARGETS[:4])])
    mesh, traj, out, cloud = (str(tmp_path / n) for n in ("room.ply", "traj.txt", "culled.ply", "room_pc_unseen.npy"))
    write_ply(mesh, v, f)
    np.savetxt(traj, c2w.reshape(len(c2w), 16))                              # a trajectory file stores OpenCV poses
    pv, pf = read_mesh(mesh)
    poses = recon.load_poses(traj)
    opencv = pose_stack(poses, flip_yz=True)                                 # what the commands render from
    near = 0.01 * 5.0

    assert recon.main(["cull", "--input_mesh", mesh, "--traj", traj, "--output_mesh", out, "--occlusion", "--min_views", "2"]) == 0
    want = O.visibility_counts(pv, pv, pf, opencv, 680, 1200, 600.0, 600.0, 599.5, 339.5, 0.03, near)
    keep = (want >= 2)[pf].any(1)
    cv, cf = read_mesh(out)
    assert np.array_equal(np.asarray(cf), np.asarray(pf)[keep]) and len(cv) == len(pv)
    assert 0 < keep.sum() < len(pf)

    assert recon.main(["unseen", "--gt_mesh", mesh, "--traj", traj, "--output", cloud, "--n_points", "20000", "--seed", "5"]) == 0
    got = np.load(cloud)
    pts = recon.sample_surface(pv, pf, 20000, seed=5)[0].cpu().numpy()
    count = O.visibility_counts(pts, pv, pf, opencv, 680, 1200, 600.0, 600.0, 599.5, 339.5, 0.03, near)
    assert got.dtype == np.float64 and np.array_equal(got, pts[count == 0])
    assert 0 < len(got) < len(pts)
