"""GPU tests of the depth rasterizer and the 2-D depth metric (nice_slam_amd/csrc/nsr_raster.h, nice_slam_amd/raster.py) at
the reference's sizes: 500 x 500 depth stacks of a 300k-triangle room against the numpy restatement (tests/raster_reference.py)
bit for bit and run to run, very large triangles near the camera, the view test on a 1M-point cloud, the metric end to end
and the ``depth`` command in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_reference as R
from test_raster_emu import check_depth_batches
from nice_slam_amd import raster

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H, W, F, C = 500, 500, 300.0, 249.5
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([5.0, 4.0, 3.0])
TABLE_LO, TABLE_HI = np.array([1.2, 1.0, 0.0]), np.array([2.8, 2.0, 0.75])


def room(n=(200, 160, 120)):
    """the room's closed surface (inner side seen from the cameras) and a table block, 300k + triangles"""
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, n)
    tv, tf = R.box_mesh(TABLE_LO, TABLE_HI, (16, 10, 6))
    return np.concatenate([v, tv]), np.concatenate([f, tf + len(v)]).astype(np.int32)


def views(rng, n):
    out = []
    for _ in range(n):
        eye = rng.uniform([0.5, 0.5, 0.9], [4.5, 3.5, 2.6])
        out.append(R.look_from(eye, eye + rng.normal(size=3)))
    return np.stack(out)


@pytest.fixture(scope="module")
def scene():
    return room()


def test_room_matches_restatement(scene):
    v, f = scene
    assert len(f) >= 200_000
    c2w = views(np.random.default_rng(0), 16)
    near = 0.01 * 5.0
    got = raster.render_depth(v, f, c2w, near=near).cpu().numpy()
    want = R.render_views(v, f, c2w, H, W, F, F, C, C, near, 20.0)
    assert np.array_equal(got, want)
    assert (got > 0).all()                                                   # watertight from inside
    again = raster.render_depth(v, f, c2w, near=near).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    other = raster.render_depth(v * 1.001, f, c2w, near=near)
    l1 = raster.depth_l1(torch.from_numpy(got).cuda(), other).cpu().numpy()
    assert np.array_equal(l1, R.depth_l1(got, other.cpu().numpy()))
    assert np.array_equal(l1, raster.depth_l1(torch.from_numpy(got).cuda(), other).cpu().numpy())


def test_batches_of_views():
    check_depth_batches(None)


def test_large_near_triangles():
    # one triangle covering the whole image, one crossing the near plane, a small one behind both, all in front of a wall
    v = np.array([[-50.0, -50.0, 2.0], [50.0, -50.0, 2.5], [0.0, 60.0, 2.2],
                  [-1.0, -1.0, -0.5], [1.5, -0.5, 3.0], [0.0, 1.5, 1.0],
                  [-0.1, -0.1, 1.5], [0.1, -0.1, 1.5], [0.0, 0.1, 1.6]])
    f = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    c2w = np.stack([np.eye(4), R.look_from([0.1, 0.0, 0.0], [0.0, 0.2, 2.0])])
    near = 0.05
    got = raster.render_depth(v, f, c2w, near=near).cpu().numpy()
    want = R.render_views(v, f, c2w, H, W, F, F, C, C, near, 20.0)
    assert np.array_equal(got, want)
    assert (got > 0).all() and (got < 2.0).any()


def test_view_unseen_1m():
    rng = np.random.default_rng(3)
    pts = rng.uniform([-0.5, 3.0, 1.0], [0.5, 3.4, 2.0], (1_000_000, 3))          # a patch outside one wall
    c2w = []
    for _ in range(48):
        eye = rng.uniform([-1.0, -1.0, 0.5], [1.0, 1.0, 2.5])
        m = np.eye(4)
        m[:3, :] = raster.viewmatrix(rng.normal(size=3), [0, 0, -1], eye)
        c2w.append(m)
    c2w = np.stack(c2w)
    got = raster.views_unseen(c2w, pts)
    want = np.array([R.check_proj_sees(pts, c, H, W, F, F, C, C) for c in c2w])
    assert np.array_equal(got, want)
    assert got.any() and not got.all()
    assert np.array_equal(raster.views_unseen(c2w, torch.from_numpy(pts).float().cuda()), got)


def test_metric_end_to_end():
    v, f = room((50, 40, 30))
    same = raster.calc_2d_metric((v, f), (v, f), align=False, n_imgs=50, unseen=False)
    assert same["depth_l1_cm"] == 0.0 and same["per_view"].shape == (50,)
    aligned = raster.calc_2d_metric((v, f), (v, f), align=True, n_imgs=50, unseen=False)
    assert aligned["depth_l1_cm"] < 1e-6
    moved = v.copy()
    moved[moved[:, 2] == 0.0, 2] = 0.02
    m = raster.calc_2d_metric((moved, f), (v, f), align=False, n_imgs=50, unseen=False)
    assert 0.0 < m["depth_l1_cm"] < 2.0


def test_depth_command(tmp_path):
    from nice_slam_amd.ply import write_ply
    v, f = room((20, 16, 12))
    gt, rec = str(tmp_path / "gt.ply"), str(tmp_path / "rec.ply")
    write_ply(gt, v, f)
    moved = v.copy()
    moved[:, 0] += 0.01
    write_ply(rec, moved, f)
    np.save(str(tmp_path / "gt_pc_unseen.npy"), np.array([[50.0, 50.0, 50.0]]))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "nice_slam_amd.recon", "depth", "--rec_mesh", rec,
                          "--gt_mesh", gt, "--n_imgs", "20"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("Depth L1:")]
    assert len(line) == 1
    assert 0.0 <= float(line[0].split(":")[1]) < 1.0
