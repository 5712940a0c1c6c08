"""CPU tests of the point-visibility kernel and what is built on it (nice_slam_amd/csrc/nsr_raster.h points_visible_kernel,
raster.visibility_counts / unseen_points, recon.cull_masks(occlusion=True)), executed under the emulator (tests/emu/) at small
sizes: counts against the numpy restatement (tests/occlusion_reference.py) exactly, over several batches of views and a
point count that is no multiple of the block; what a pillar hides and what it does not; the scaled-image rule; the culling
masks; the unseen cloud; the ABI's error paths and the command line."""
import numpy as np
import pytest
import torch

import emu_harness
import occlusion_reference as O
import raster_reference as R
from nice_slam_amd import _capi, raster, recon
from nice_slam_amd.engine import Engine, pose_stack

H, W, FX, FY, CX, CY = 48, 64, 40.0, 42.0, 31.5, 23.5
CAM = (H, W, FX, FY, CX, CY)
NEAR, EPS = 0.05, 0.03
EYES = ([0.5, 2.0, 1.5], [4.4, 0.6, 1.0], [1.0, 3.4, 2.4], [3.6, 3.5, 0.6], [2.5, 0.5, 2.0])
TARGETS = ([2.5, 2.0, 1.5], [2.5, 2.0, 1.2], [2.5, 2.0, 0.5], [0.0, 0.0, 1.5], [2.5, 4.0, 1.0])


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def scene():
    """the room and pillar, five views and a point set: the mesh's vertices, points in and around the room, points closer
    to a camera than near; with the restated per-view visibility, computed once"""
    v, f, n_room = O.room_and_pillar()
    c2w = np.stack([R.look_from(e, t) for e, t in zip(EYES, TARGETS)])
    rng = np.random.default_rng(7)
    pts = np.concatenate([v, rng.uniform([-1.0, -1.0, -0.5], [6.0, 5.0, 3.5], (700, 3)),
                          np.array(EYES[0]) + rng.normal(scale=0.03, size=(17, 3))])
    assert len(pts) % 256 != 0 and len(pts) > 256
    vis = O.visibility_counts(pts, v, f, c2w, *CAM, EPS, NEAR, per_view=True)
    return {"v": v, "f": f, "n_room": n_room, "c2w": c2w, "pts": pts, "vis": vis}


def counts(E, pts, s, c2w=None, **kw):
    kw.setdefault("eps", EPS)
    return raster.visibility_counts(pts, s["v"], s["f"], s["c2w"] if c2w is None else c2w, *CAM, near=NEAR, engine=E, **kw).numpy()


def test_counts_match_restatement(E, scene):
    want = scene["vis"].sum(0).astype(np.int32)
    assert want.max() >= 3 and (want == 0).any()
    frustum = O.frustum_counts(scene["pts"], scene["c2w"], *CAM, NEAR)
    assert (want < frustum).sum() > 50                                       # occlusion decides many of them
    for dtype in (np.float64, np.float32):
        pts = scene["pts"].astype(dtype)
        w = want if dtype is np.float64 else O.visibility_counts(pts, scene["v"], scene["f"], scene["c2w"], *CAM, EPS, NEAR)
        got = counts(E, pts, scene, views_per_launch=2)                      # batches of 2, 2 and 1 views
        assert got.dtype == np.int32 and got.shape == (len(pts),)
        assert np.array_equal(got, w)
        assert np.array_equal(counts(E, pts, scene), w)                      # one batch: the same counts
        assert np.array_equal(counts(E, pts, scene, views_per_launch=1), w)
    assert raster.visibility_counts(scene["pts"][:0], scene["v"], scene["f"], scene["c2w"], *CAM, near=NEAR, engine=E).shape == (0,)


def test_huge_eps_is_the_frustum_count(E, scene):
    got = counts(E, scene["pts"], scene, eps=1e30, views_per_launch=2)
    assert np.array_equal(got, O.frustum_counts(scene["pts"], scene["c2w"], *CAM, NEAR))


def test_pillar_hides_the_wall_behind_it(E, scene):
    v, n_room = scene["v"], scene["n_room"]
    c2w = scene["c2w"][:1]                                                   # at (0.5, 2, 1.5) looking along +x at the pillar
    occ, inf = counts(E, v, scene, c2w), counts(E, v, scene, c2w, eps=1e30)
    assert np.all(occ <= inf)
    # the wall x = 5 behind the pillar: its silhouette there is |y - 2| < 0.3 * 4.5 / 1.7 = 0.79
    behind = np.zeros(len(v), bool)
    behind[:n_room] = (v[:n_room, 0] == 5.0) & (np.abs(v[:n_room, 1] - 2.0) <= 0.5)
    assert behind.sum() == 3 * 7
    assert np.all(inf[behind] == 1) and np.all(occ[behind] == 0)
    # the pillar's front face x = 2.2 is seen wherever it is in the image
    front = np.zeros(len(v), bool)
    front[n_room:] = v[n_room:, 0] == O.PILLAR_LO[0]
    assert inf[front].sum() >= 12 and np.array_equal(occ[front], inf[front])


def test_perpendicular_wall_is_seen(E, scene):
    v, n_room = scene["v"], scene["n_room"]
    c2w = R.look_from([1.5, 2.0, 1.5], [0.0, 2.0, 1.5])[None]                # facing the wall x = 0, the pillar behind the camera
    tight = 1e-4                                                             # the wall's depth is the same in every pixel
    occ, inf = counts(E, v, scene, c2w, eps=tight), counts(E, v, scene, c2w, eps=1e30)
    wall = np.zeros(len(v), bool)
    wall[:n_room] = v[:n_room, 0] == 0.0
    assert inf[wall].sum() >= 12
    assert np.array_equal(occ[wall], inf[wall])


def test_raster_div(E, scene):
    assert raster.raster_divisor(680, 1200) == 2 and raster.raster_divisor(1024, 1024) == 1 and raster.raster_divisor(40, 3073) == 4
    assert raster.scaled_camera(680, 1200, 600.0, 600.0, 599.5, 339.5, 2) == (340, 600, 300.0, 300.0, 299.5, 169.5)
    got = counts(E, scene["pts"], scene, raster_div=2, views_per_launch=3)
    fx, fy, cx, cy = FX / 2, FY / 2, (CX + 0.5) / 2 - 0.5, (CY + 0.5) / 2 - 0.5
    depth = R.render_views(scene["v"], scene["f"], scene["c2w"], 24, 32, fx, fy, cx, cy, NEAR, 1e3)
    w = R.w2c_rows(scene["c2w"])
    want = sum(O.visible(scene["pts"], w[k], depth[k], fx, fy, cx, cy, NEAR, 1e3, EPS).astype(np.int32) for k in range(len(w)))
    assert np.array_equal(got, want)
    assert not np.array_equal(got, scene["vis"].sum(0))                      # and it is another image than the full one


def traj(c2w):
    """the poses as load_poses returns them: float32 tensors, y and z axes flipped"""
    return [torch.from_numpy(t).float() for t in O.as_loaded(c2w)]


def test_cull_masks(E, scene):
    v, f = scene["v"], scene["f"]
    poses = traj(scene["c2w"])
    cam = dict(H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, engine=E)
    # the defaults leave today's path and results untouched
    seen0, keep0 = recon.cull_masks(v, f, poses, **cam)
    seen1, keep1 = recon.cull_masks(v, f, poses, occlusion=False, eps=0.5, min_views=3, stride=2, **cam)
    assert seen0.dtype == torch.bool and torch.equal(seen0, seen1) and torch.equal(keep0, keep1)
    # with occlusion: the restated counts of the same (float32) poses, turned back to the OpenCV convention
    c2w = pose_stack(poses, flip_yz=True)
    want = O.visibility_counts(v, v, f, c2w, *CAM, EPS, 0.01 * 5.0)
    seen, keep = recon.cull_masks(v, f, poses, occlusion=True, **cam)
    assert np.array_equal(seen.numpy(), want >= 1)
    assert np.array_equal(keep.numpy(), (want >= 1)[f].any(1))
    assert keep.any() and not keep.all()
    seen2, keep2 = recon.cull_masks(v, f, poses, occlusion=True, min_views=2, **cam)
    assert np.array_equal(seen2.numpy(), want >= 2)
    assert seen2.sum() < seen.sum() and not (seen2 & ~seen).any() and not (keep2 & ~keep).any()
    seen3, _ = recon.cull_masks(v, f, poses, occlusion=True, stride=2, eps=0.1, **cam)
    assert np.array_equal(seen3.numpy(), O.visibility_counts(v, v, f, c2w[::2], *CAM, 0.1, 0.01 * 5.0) >= 1)
    cv, cf = recon.cull_mesh(v, f, poses, H, W, FX, FY, CX, CY, engine=E, occlusion=True)
    assert cv.shape == v.shape and np.array_equal(cf.numpy(), f[keep.numpy()])


def test_unseen_points(E, scene):
    v, f = scene["v"], scene["f"]
    poses = traj(scene["c2w"][:2])
    got = raster.unseen_points((v, f), poses, n_points=1500, seed=3, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, engine=E)
    pts = recon.sample_surface(v, f, 1500, seed=3, engine=E)[0].numpy()
    want = O.visibility_counts(pts, v, f, pose_stack(poses, flip_yz=True), *CAM, EPS, 0.01 * 5.0)
    assert got.dtype == np.float64 and np.array_equal(got, pts[want == 0])
    assert 0 < len(got) < len(pts)


def test_abi_errors(E, scene):
    lib = E.lib
    pts = torch.from_numpy(scene["pts"][scene["vis"][0]][:10].copy())               # ten points the first view sees
    assert len(pts) == 10
    w = torch.from_numpy(R.w2c_rows(scene["c2w"][:1]))
    depth = torch.zeros((1, H, W), dtype=torch.float32)
    count = torch.zeros(10, dtype=torch.int32)

    def call(n=10, K=1, h=H, wd=W, near=NEAR, far=20.0, eps=EPS, p=pts):
        return lib.nsr_points_visible(None if p is None else p.data_ptr(), n, 1, w.data_ptr(), K, depth.data_ptr(), h, wd, FX, FY, CX, CY,
                                      near, far, eps, count.data_ptr(), None)

    for kw, msg in ((dict(n=0), b"no points"), (dict(n=-3), b"no points"), (dict(K=0), b"no views"), (dict(h=0), b"empty image"),
                    (dict(wd=-1), b"empty image"), (dict(near=1.0, far=1.0), b"near < far"), (dict(near=2.0, far=1.0), b"near < far"),
                    (dict(near=float("nan")), b"near < far"), (dict(eps=-1e-9), b"eps"), (dict(eps=float("nan")), b"eps"),
                    (dict(p=None), b"null pointer")):
        assert call(**kw) != 0, kw
        assert msg in lib.nsr_last_error(), (kw, lib.nsr_last_error())
    assert not count.any()
    assert call() == 0 and count.tolist() == [1] * 10                        # an empty depth image hides nothing
    with pytest.raises(_capi.NsrError, match="no views"):
        raster.visibility_counts(scene["pts"], scene["v"], scene["f"], np.zeros((0, 4, 4)), *CAM, engine=E)
    with pytest.raises(_capi.NsrError, match="empty mesh"):
        raster.visibility_counts(scene["pts"], scene["v"], scene["f"][:0], scene["c2w"], *CAM, engine=E)


def test_cli(capsys):
    with pytest.raises(SystemExit) as e:
        recon.main(["cull", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for opt in ("--input_mesh", "--traj", "--output_mesh", "--occlusion", "--eps", "--min_views", "--stride"):
        assert opt in out
    with pytest.raises(SystemExit) as e:
        recon.main(["unseen", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for opt in ("--gt_mesh", "--traj", "--output", "--n_points", "--seed"):
        assert opt in out
