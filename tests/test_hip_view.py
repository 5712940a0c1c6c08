"""GPU tests of the replay view (nice_slam_amd/csrc/nsr_view.h, nice_slam_amd/viewer.py): the contract of tests/view_reference.py
on the device at 100 x 150 (partial tiles both ways) on a room of about 30k triangles with a table, 4 views and every cull mode;
one 540 x 960 frame with 5000 points; run-to-run byte equality; and the command line in a child process."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_reference as R
import view_reference as V
from test_view_emu import check_mesh_batches
from nice_slam_amd import raster, viewer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H, W = 100, 150
CAM = (110.0, 112.0, 74.5, 49.5)
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([5.0, 4.0, 3.0])
TABLE_LO, TABLE_HI = np.array([1.2, 1.0, 0.0]), np.array([2.8, 2.0, 0.75])
SHARE_CAP = 0.01


def room(n=(60, 50, 35), table=(16, 10, 6)):
    """the room's closed surface and a table block, every normal pointing out of its box: about 30k triangles"""
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, n)
    f = V.orient_outward(v, f, (ROOM_LO + ROOM_HI) / 2)
    tv, tf = R.box_mesh(TABLE_LO, TABLE_HI, table)
    tf = V.orient_outward(tv, tf, (TABLE_LO + TABLE_HI) / 2)
    return np.concatenate([v, tv]), np.concatenate([f, tf + len(v)]).astype(np.int32)


@pytest.fixture(scope="module")
def scene():
    v, f = room()
    rng = np.random.default_rng(0)
    c2w = []
    for _ in range(3):
        eye = rng.uniform([0.5, 0.5, 0.9], [4.5, 3.5, 2.6])
        c2w.append(R.look_from(eye, (TABLE_LO + TABLE_HI) / 2 + rng.normal(scale=0.3, size=3)))      # the table is in view
    c2w.append(R.look_from([-3.0, -2.5, 4.0], [2.5, 2.0, 1.0]))                   # from outside the room
    colors = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    nrm, sums = viewer.vertex_normals(v, f, return_sums=True)
    return v, f, np.stack(c2w), colors, nrm.cpu().numpy(), sums.cpu().numpy()


def check_colour(got, want, what):
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((diff > 0).mean())
    print(f"{what}: share of shaded channel values that differ from the fp64 restatement {share:.6f} (max {diff.max()})")
    assert diff.max() <= 1
    assert share <= SHARE_CAP


def test_vertex_normals(scene):
    v, f, _, _, nrm, sums = scene
    assert 25_000 <= len(f) <= 35_000
    want = V.normal_sums(v, f)
    assert np.array_equal(sums, want)                                            # bit for bit
    assert np.abs(nrm.astype(np.float64) - V.normalize_sums(want)).max() <= 5e-7
    again = viewer.vertex_normals(v, f, return_sums=True)
    assert again[0].cpu().numpy().tobytes() == nrm.tobytes() and again[1].cpu().numpy().tobytes() == sums.tobytes()


@pytest.mark.parametrize("cull", [None, "back", "front"])
def test_mesh_layer_matches_restatement(scene, cull):
    v, f, c2w, colors, nrm, _ = scene
    near, far = 0.05, 1000.0
    rgb, depth, face = (x.cpu().numpy() for x in viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, cull=cull, near=near, far=far))
    want = V.render_mesh_views(v, f, c2w, H, W, *CAM, near, far, nrm, colors, cull or "none")
    assert np.array_equal(depth, want[1])
    assert np.array_equal(face, want[2])
    check_colour(rgb, want[0], f"MI355X cull={cull}")
    assert (rgb[face < 0] == 255).all()
    if cull is None:
        assert np.array_equal(depth, raster.render_depth(v, f, c2w, H, W, *CAM, near=near, far=far).cpu().numpy())
        assert (depth[:3] > 0).all()
    elif cull == "back":                  # inside: only the table's outer faces face the camera; outside: the room's near walls
        table = face >= len(f) - 4 * (16 * 10 + 10 * 6 + 16 * 6)
        assert np.array_equal(table[:3], face[:3] >= 0) and table[:3].any() and (face[3] >= 0).any() and not table[3].any()
    else:
        assert (depth[:3] > 0).all()
    again = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, cull=cull, near=near, far=far)
    assert all(a.cpu().numpy().tobytes() == b.tobytes() for a, b in zip(again, (rgb, depth, face)))
    if cull == "front":                   # a mesh without colours
        grey = viewer.render_mesh(v, f, c2w[:1], H, W, *CAM, cull=cull, near=near, far=far)[0].cpu().numpy()
        check_colour(grey, V.render_mesh_views(v, f, c2w[:1], H, W, *CAM, near, far, nrm, None, cull)[0], "MI355X grey")


def test_batches_of_views():
    check_mesh_batches(None)


def test_points_full_frame(scene):
    v, f, _, colors, nrm, _ = scene
    Hf, Wf = 540, 960
    cam = viewer.default_camera(Hf, Wf)
    rng = np.random.default_rng(4)
    c2w = np.stack([R.look_from([0.6, 0.7, 1.6], [4.0, 3.0, 1.0]), R.look_from([4.2, 3.3, 1.2], [1.0, 1.0, 1.0])])
    flipped = f[:, ::-1].copy()                                                  # the room seen from inside with back faces culled
    rgb, depth, _ = viewer.render_mesh(v, flipped, c2w, Hf, Wf, *cam, colors=colors, normals=-nrm, cull="back", near=0.05)
    assert (depth > 0).all()
    counts = [5000, 1200]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    pts = rng.uniform(ROOM_LO - 0.5, ROOM_HI + 0.5, (sum(counts), 3))            # some behind the walls, some behind the camera
    pts[:400] = np.array([2.5, 2.0, 1.5]) + rng.normal(scale=0.02, size=(400, 3))                   # a dense clump: hundreds of points in one tile
    cols = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    got, owner = viewer.draw_points(rgb, depth, pts, cols, offsets, c2w, *cam, near=0.05, far=1000.0, return_owner=True)
    want, want_owner = V.draw_points(rgb.cpu().numpy(), depth.cpu().numpy(), pts, cols, offsets, c2w, *cam, 0.05, 1000.0, 4)
    assert np.array_equal(owner.cpu().numpy(), want_owner)
    assert np.array_equal(got.cpu().numpy(), want)
    drawn = [len(np.unique(o)) - 1 for o in want_owner]
    assert 500 < drawn[0] < 5000 and 100 < drawn[1] < 1200                       # the depth test and the frustum remove some
    shared = viewer.draw_points(rgb[0], depth[0], pts, cols, offsets, np.stack([c2w[0], c2w[0]]), *cam, near=0.05)
    assert shared[0].cpu().numpy().tobytes() == got[0].cpu().numpy().tobytes()
    again = viewer.draw_points(rgb, depth, pts, cols, offsets, c2w, *cam, near=0.05, far=1000.0)
    assert again.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()


def test_replay_command(tmp_path):
    from PIL import Image
    from nice_slam_amd.ply import write_ply
    out = tmp_path / "run"
    os.makedirs(out / "mesh")
    os.makedirs(out / "ckpts")
    rng = np.random.default_rng(9)
    for i, n in ((0, (10, 8, 6)), (6, (20, 16, 12))):
        v, f = room(n, (4, 3, 2))
        if i == 6:
            v = v * 1.1
        write_ply(str(out / "mesh" / f"{i:05d}_mesh.ply"), v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
    n, scale = 12, 2.0
    est, gt = torch.zeros((n + 3, 4, 4)), torch.zeros((n + 3, 4, 4))
    for i in range(n):
        for lst, wob in ((est, 0.03 * np.sin(i)), (gt, 0.0)):
            m = R.look_from([0.8 + 0.25 * i, 2.0 + wob, 1.4], [5.0, 2.0 + wob, 1.4])
            m[:3, 1] *= -1
            m[:3, 2] *= -1
            m[:3, 3] *= scale
            lst[i] = torch.from_numpy(m).float()
    torch.save({"estimate_c2w_list": est, "gt_c2w_list": gt, "idx": 5}, str(out / "ckpts" / "00005.tar"))
    torch.save({"estimate_c2w_list": est, "gt_c2w_list": gt, "idx": n - 1}, str(out / "ckpts" / "00011.tar"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "nice_slam_amd.viewer", "--output", str(out), "--scale", str(scale)],
                         cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "ffmpeg" in res.stdout and "00011.tar" in res.stdout
    files = sorted(glob.glob(str(out / "tmp_rendering" / "*.jpg")))
    assert [os.path.basename(p) for p in files] == [f"{k:06d}.jpg" for k in range(1, n + 1)]
    imgs = [np.asarray(Image.open(p).convert("RGB")).astype(np.int32) for p in files]
    assert all(im.shape == (540, 960, 3) for im in imgs)
    assert (imgs[0] < 250).mean() > 0.05                                         # a mesh is on the picture
    # the second mesh arrives with frame 6: the picture changes far more there than between two frames of one mesh
    step = [float(np.abs(a - b).mean()) for a, b in zip(imgs[:-1], imgs[1:])]
    assert step[5] > 5 * max(step[:5] + step[6:]) and step[5] > 1.0
