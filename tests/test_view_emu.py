"""CPU tests of the replay view (nice_slam_amd/csrc/nsr_view.h, nice_slam_amd/viewer.py), executed under the emulator (tests/emu/)
at 48 x 64: vertex normals, the mesh layer in its three cull modes and the point layer against the numpy restatement
(tests/view_reference.py) -- depth, owning face, normal sums, point ownership and point colours bit for bit, shaded colours within
one level -- the camera wireframe and the viewer's pose against values written out by hand, a 12-frame toy replay, the ABI's error
paths and the command line."""
import numpy as np
import pytest
import torch

import emu_harness
import raster_reference as R
import view_reference as V
from test_raster_emu import BATCH_FAR, BATCH_NEAR, CX, CY, FX, FY, H, ROOM_HI, ROOM_LO, W, batch_case, mixed_scene, views
from nice_slam_amd import _capi, raster, viewer
from nice_slam_amd.engine import Engine

CAM = (FX, FY, CX, CY)
SHARE_CAP = 0.01            # of the shaded channel values may differ from the fp64 restatement (by one level)
SHARE_FP32 = 0.002          # what evaluating the restatement's own shading in fp32 instead of fp64 may change on these scenes


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


def oriented_room(n=(25, 20, 15), lo=ROOM_LO, hi=ROOM_HI):
    """the closed room of raster_reference.box_mesh, every face's normal pointing out of the room"""
    v, f = R.box_mesh(lo, hi, n)
    return v, V.orient_outward(v, f, (np.asarray(lo) + np.asarray(hi)) / 2)


def check_colour(got, want, what):
    """the gate of the shaded colour: every channel within one level of the fp64 restatement, at most 1 % different at all"""
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    share = float((diff > 0).mean())
    print(f"{what}: share of shaded channel values that differ from the fp64 restatement {share:.6f} (max {diff.max()})")
    assert diff.max() <= 1
    assert share <= SHARE_CAP
    return share


def mesh_case(E, v, f, c2w, near, far, colors, cull, normals=None):
    nrm_ref = V.normalize_sums(V.normal_sums(v, f)).astype(np.float32) if normals is None else normals
    rgb, depth, face = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, normals=normals, cull=cull, near=near, far=far, engine=E)
    rgb, depth, face = rgb.numpy(), depth.numpy(), face.numpy()
    nrm = viewer.vertex_normals(v, f, engine=E).numpy() if normals is None else normals       # what the kernel interpolated
    want = V.render_mesh_views(v, f, c2w, H, W, *CAM, near, far, nrm, colors, cull or "none")
    assert rgb.dtype == np.uint8 and depth.dtype == np.float32 and face.dtype == np.int32
    assert np.array_equal(depth, want[1])
    assert np.array_equal(face, want[2])
    assert np.array_equal(face >= 0, depth > 0)
    assert (rgb[face < 0] == 255).all()
    check_colour(rgb, want[0], f"cull={cull}")
    assert np.abs(nrm.astype(np.float64) - nrm_ref.astype(np.float64)).max() <= 5e-7
    return rgb, depth, face, want


# ---- vertex normals -------------------------------------------------------------------------------------------------------
def test_vertex_normals(E):
    rng = np.random.default_rng(11)
    v, f = mixed_scene(rng)
    k = len(v)
    # two faces on three new vertices that run opposite ways: their cross products cancel exactly; and a vertex of no face
    v = np.concatenate([v, [[1.0, 1.0, 1.0], [1.5, 1.25, 1.0], [1.0, 1.75, 1.5], [9.0, 9.0, 9.0]]])
    f = np.concatenate([f, np.array([[k, k + 1, k + 2], [k, k + 2, k + 1]], np.int32)])
    nrm, sums = viewer.vertex_normals(v, f, return_sums=True, engine=E)
    nrm, sums = nrm.numpy(), sums.numpy()
    want = V.normal_sums(v, f)
    assert sums.dtype == np.float64 and np.array_equal(sums, want)            # bit for bit
    assert np.array_equal(sums[k:], np.zeros((4, 3))) and np.array_equal(nrm[k:], np.zeros((4, 3), np.float32))
    # the restatement's sums against a plain Python loop in face order (the order is part of the contract)
    v32 = v.astype(np.float32).astype(np.float64)
    loop = np.zeros_like(want)
    for face in f[:400]:
        a, b, c = v32[face]
        u, w = b - a, c - a
        for vert in face:
            loop[vert] += [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
    touched = np.setdiff1d(np.unique(f[:400]), np.unique(f[400:]))
    assert len(touched) > 50 and np.array_equal(loop[touched], want[touched])
    # normalised fp32: two fp32 roundings of a value <= 1
    ref = V.normalize_sums(want)
    assert nrm.dtype == np.float32 and np.abs(nrm.astype(np.float64) - ref).max() <= 5e-7
    length = np.linalg.norm(nrm.astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0)) and (length > 0).sum() > 100
    # degenerate faces of the scene add zeros; area weighting: a big and a small face on one vertex
    vv = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0.1, 0], [0, 0, 0.1]], np.float64)
    ff = np.array([[0, 1, 2], [0, 3, 4]], np.int32)
    n2 = viewer.vertex_normals(vv, ff, engine=E).numpy()
    assert np.allclose(n2[0], np.array([0.01, 0, 16]) / np.hypot(0.01, 16), atol=1e-7)
    assert np.array_equal(viewer.vertex_normals(v, f, engine=E).numpy(), nrm)


# ---- mesh layer -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    rng = np.random.default_rng(1)
    v, f = mixed_scene(rng)
    c2w = views(rng, 4)
    colors = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    return v, f, c2w, colors


@pytest.mark.parametrize("cull", [None, "back", "front"])
def test_mesh_layer_matches_restatement(E, mixed, cull):
    v, f, c2w, colors = mixed
    near, far = 0.3, 2.5
    rgb, depth, face, want = mesh_case(E, v, f, c2w, near, far, colors, cull)
    assert (face >= 0).mean() > 0.5 and (face < 0).any()
    if cull is None:
        assert np.array_equal(depth, raster.render_depth(v, f, c2w, H, W, *CAM, near=near, far=far, engine=E).numpy())
    else:                                                   # the two culled images split the fragments of the unculled one
        none = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, near=near, far=far, engine=E)
        other = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, cull="front" if cull == "back" else "back", near=near, far=far,
                                   engine=E)
        d0, d1, d2 = none[1].numpy(), depth, other[1].numpy()
        both = np.where(d1 == 0, d2, np.where(d2 == 0, d1, np.minimum(d1, d2)))
        assert np.array_equal(d0, both)
        assert (d1 != d0).any()
    # bit-identical run to run
    again = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, cull=cull, near=near, far=far, engine=E)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(again, (rgb, depth, face)))
    # the restatement's own shading evaluated in fp32 stays far under the cap: the cap is not consumed by the inputs
    nrm = viewer.vertex_normals(v, f, engine=E).numpy()
    lo = V.render_mesh_views(v, f, c2w, H, W, *CAM, near, far, nrm, colors, cull or "none", dtype=np.float32)[0]
    share32 = float((lo != want[0]).mean())
    print(f"cull={cull}: fp32 against fp64 shading of the restatement differs on {share32:.6f} of the channel values")
    assert share32 < SHARE_FP32


def test_big_bins_room_inside(E):
    v, f = oriented_room()
    rng = np.random.default_rng(2)
    c2w = np.stack([R.look_from([0.3, 0.3, 0.3], [5.0, 4.0, 3.0]), views(rng, 1)[0]])      # from a corner: three walls in view
    colors = rng.integers(0, 256, (len(v), 3), dtype=np.uint8)
    # some tile's bin exceeds one batch of 256 entries: the first view alone has more than 256 entries per tile on average
    w = R.w2c_rows(c2w)
    lib = E.lib
    vt, ft, wt = torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f), torch.from_numpy(w)
    ws = torch.zeros(int(lib.nsr_view_workspace_bytes(len(v), len(f), 1, H, W)), dtype=torch.uint8)
    n = torch.zeros(1, dtype=torch.int64)
    assert lib.nsr_raster_bin(vt.data_ptr(), len(v), ft.data_ptr(), len(f), wt.data_ptr(), 1, H, W, *CAM, 0.05, 20.0, ws.data_ptr(),
                              n.data_ptr(), None) == 0
    ntiles = ((W + 31) // 32) * ((H + 31) // 32)
    assert int(n[0]) > 256 * ntiles
    for cull in (None, "back", "front"):
        rgb, depth, face, _ = mesh_case(E, v, f, c2w, 0.05, 20.0, colors, cull)
        # seen from inside, the outward faces of the room are all back faces
        if cull == "back":
            assert (face < 0).all() and (rgb == 255).all() and (depth == 0).all()
        else:
            assert (depth > 0).all()
    cast = np.stack([R.ray_cast_box_inside(c, ROOM_LO, ROOM_HI, H, W, *CAM) for c in c2w])
    assert np.abs(depth / cast - 1).max() < 1e-5


def ray_box(c2w, lo, hi):
    """fp64 (t_enter, t_exit) [H, W] of the pixel rays against the box from a camera outside it (inf / -inf: a miss)"""
    j, i = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.stack([(i - CX) / FX, (j - CY) / FY, np.ones_like(i)], -1) @ c2w[:3, :3].T
    o = c2w[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
    miss = (tn > tf) | (tf < 0)
    return np.where(miss, np.inf, tn), np.where(miss, -np.inf, tf)


def test_room_from_outside_shows_its_far_walls(E):
    """Replay flips the faces of the mesh it is given (viz.py:95-101) and culls back faces: a room whose normals point outwards
    is then seen from outside through its near wall"""
    v, f = oriented_room()
    c2w = np.stack([R.look_from([-4.0, -3.0, 4.5], [2.5, 2.0, 1.5]), R.look_from([9.0, 8.0, 1.0], [2.5, 2.0, 1.5])])
    flipped = f[:, ::-1].copy()
    t_in, t_out = (np.stack(x) for x in zip(*[ray_box(c, ROOM_LO, ROOM_HI) for c in c2w]))
    back = viewer.render_mesh(v, flipped, c2w, H, W, *CAM, cull="back", near=0.05, far=100.0, engine=E)[1].numpy()
    none = viewer.render_mesh(v, flipped, c2w, H, W, *CAM, cull=None, near=0.05, far=100.0, engine=E)[1].numpy()
    hit = back > 0
    assert hit.mean() > 0.1 and np.array_equal(hit, none > 0)
    assert np.abs(back[hit] / t_out[hit] - 1).max() < 1e-5                 # the far walls
    assert np.abs(none[hit] / t_in[hit] - 1).max() < 1e-5                  # without culling: the near wall
    assert (back[hit] > none[hit] + 0.5).mean() > 0.8
    # the same through Replay, whose flip is its own: it is handed the outward-oriented room
    rp = viewer.Replay(np.eye(4), width=W, height=H, engine=E)
    rp.update_mesh((v, f))
    assert np.array_equal(rp.mesh["f"].numpy(), flipped)


def check_mesh_batches(E):
    """render_mesh two views a launch against all three at once and the restatement (E: an engine, None: the GPU's)"""
    v, f, c2w = batch_case()
    colors = np.random.default_rng(3).integers(0, 256, (len(v), 3), dtype=np.uint8)
    draw = lambda step: [x.cpu().numpy() for x in viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, cull="back", near=BATCH_NEAR,
                                                                     far=BATCH_FAR, engine=E, views_per_launch=step)]
    two = draw(2)
    assert all(np.array_equal(a, b) for a, b in zip(two, draw(3)))
    nrm = viewer.vertex_normals(v, f, engine=E).cpu().numpy()
    want = V.render_mesh_views(v, f, c2w, H, W, *CAM, BATCH_NEAR, BATCH_FAR, nrm, colors, "back")
    assert np.array_equal(two[1], want[1]) and np.array_equal(two[2], want[2])
    check_colour(two[0], want[0], "two views a launch")
    with pytest.raises(ValueError, match="render_mesh: views_per_launch must be positive"):
        draw(0)


def test_batches_of_views(E):
    check_mesh_batches(E)


def test_duplicated_face_is_owned_by_the_smaller_id(E):
    v, f = oriented_room((5, 4, 3))
    c2w = views(np.random.default_rng(3), 2)
    base = viewer.render_mesh(v, f, c2w, H, W, *CAM, near=0.05, far=20.0, engine=E)
    j = int(np.bincount(base[2].numpy().reshape(-1)).argmax())               # the face that owns the most pixels
    for order in ("behind", "ahead"):
        if order == "behind":                                                # the copy has the larger id: ids unchanged
            ff, first, second = np.concatenate([f, f[j:j + 1]]), j, len(f)
        else:                                                                # the copy goes first: every id moves up by one
            ff, first, second = np.concatenate([f[j:j + 1], f]), 0, j + 1
        rgb, depth, face = (x.numpy() for x in viewer.render_mesh(v, ff, c2w, H, W, *CAM, near=0.05, far=20.0, engine=E))
        assert np.array_equal(depth, base[1].numpy())
        assert (face == first).sum() == (base[2].numpy() == j).sum() > 0 and not (face == second).any()


def test_mesh_without_colours_and_zero_normals(E, mixed):
    v, f, c2w, _ = mixed
    rgb, depth, face, _ = mesh_case(E, v, f, c2w[:2], 0.3, 2.5, None, None)
    hit = face >= 0
    assert (rgb[hit][:, 0] == rgb[hit][:, 1]).all() and (rgb[hit][:, 1] == rgb[hit][:, 2]).all()         # grey
    assert rgb[hit].max() <= 204 and rgb[hit].min() >= int(np.floor(255 * 0.8 * 0.35 + 0.5))              # 0.8 (a .. 1)
    # a zero interpolated normal: s = a exactly
    zero = np.zeros((len(v), 3), np.float32)
    rgb0 = viewer.render_mesh(v, f, c2w[:2], H, W, *CAM, normals=zero, near=0.3, far=2.5, engine=E)[0].numpy()
    assert (rgb0[hit] == int(np.floor(255 * (0.8 * 0.35) + 0.5))).all() and (rgb0[~hit] == 255).all()
    mesh_case(E, v, f, c2w[:1], 0.3, 2.5, None, "back", normals=zero)


# ---- point layer ----------------------------------------------------------------------------------------------------------
def point_case(E, base_rgb, base_d, pts, cols, offsets, c2w, near=0.1, far=10.0, size=4):
    got, owner = viewer.draw_points(base_rgb, base_d, pts, cols, offsets, c2w, *CAM, near=near, far=far, size=size, return_owner=True,
                                    engine=E)
    want, want_owner = V.draw_points(base_rgb, base_d, pts, cols, offsets, c2w, *CAM, near, far, size)
    got, owner = got.numpy(), owner.numpy()
    assert np.array_equal(owner, want_owner)
    assert np.array_equal(got, want)
    return got, owner


def at_pixel(u, v, z):
    """the camera-space point (the camera is the identity pose) that projects to (u, v) at depth z"""
    return [(u - CX) / FX * z, (v - CY) / FY * z, z]


def test_points_by_hand(E):
    base_rgb = np.full((H, W, 3), 200, np.uint8)
    base_d = np.zeros((H, W), np.float32)
    base_d[:, 32:] = 2.0                                                    # a wall at depth 2 on the right half
    behind = float(np.nextafter(np.float32(2.0), np.float32(3.0)))
    pts = np.array([at_pixel(0.2, 10.0, 1.0),            # 0: cut by the left border: columns -2 .. 1 -> 0 .. 1
                    at_pixel(20.0, 0.0, 1.0),            # 1: cut by the top border: rows -2 .. 1 -> 0 .. 1
                    at_pixel(W - 0.8, 20.0, 1.0),        # 2: cut by the right border
                    at_pixel(10.0, H - 1.0, 1.0),        # 3: cut by the bottom border
                    [0.0, 0.0, -1.0],                    # 4: behind the camera
                    at_pixel(16.0, 16.0, 50.0),          # 5: beyond far
                    at_pixel(40.0, 30.0, 2.0),           # 6: exactly at the base depth: drawn
                    at_pixel(50.0, 30.0, behind),        # 7: just behind it: hidden
                    at_pixel(20.0, 30.0, 1.5),           # 8, 9: one pixel block, equal depth: the smaller index wins
                    at_pixel(20.0, 30.0, 1.5),
                    at_pixel(22.0, 31.0, 1.25),          # 10: nearer, overlapping 8 / 9: it wins where it lies
                    at_pixel(-30.0, 10.0, 1.0)],         # 11: wholly outside
                   np.float64)
    cols = (np.arange(len(pts) * 3).reshape(-1, 3) % 199 + 1).astype(np.uint8)
    got, owner = point_case(E, base_rgb, base_d, pts, cols, [0, len(pts)], np.eye(4))
    own = owner[0]
    # i0 = floor(u - 2 + 0.5)
    assert set(np.argwhere(own == 0)[:, 1]) == {0, 1} and set(np.argwhere(own == 0)[:, 0]) == {8, 9, 10, 11}
    assert set(np.argwhere(own == 1)[:, 0]) == {0, 1} and set(np.argwhere(own == 1)[:, 1]) == {18, 19, 20, 21}
    assert set(np.argwhere(own == 2)[:, 1]) == {W - 3, W - 2, W - 1}
    assert set(np.argwhere(own == 3)[:, 0]) == {H - 3, H - 2, H - 1}
    for gone in (4, 5, 7, 9, 11):
        assert not (own == gone).any()
    assert (own == 6).sum() == 16 and (got[0][own == 6] == cols[6]).all()
    assert (own == 10).sum() == 16 and (own == 8).sum() == 16 - 6                 # 10 covers columns 20 .. 23, rows 29 .. 32; 8 columns 18 .. 21, rows 28 .. 31
    assert (got[0][own < 0] == 200).all()
    # sizes 1 and 5 (odd: i0 = floor(u - 2.5 + 0.5))
    g1, o1 = point_case(E, base_rgb, base_d, pts, cols, [0, len(pts)], np.eye(4), size=1)
    assert (o1[0] == 6).sum() == 1 and o1[0][30, 40] == 6
    g5, o5 = point_case(E, base_rgb, base_d, pts, cols, [0, len(pts)], np.eye(4), size=5)
    assert set(np.argwhere(o5[0] == 6)[:, 1]) == {38, 39, 40, 41, 42}


def test_points_frames_and_bases(E, mixed):
    v, f, c2w, colors = mixed
    rng = np.random.default_rng(7)
    c2w = c2w[:3]
    rgb, depth, _ = viewer.render_mesh(v, f, c2w, H, W, *CAM, colors=colors, near=0.3, far=2.5, engine=E)
    rgb, depth = rgb.numpy(), depth.numpy()
    counts = [700, 0, 37]                                                 # B = 3 frames, one of them empty
    offsets = np.concatenate([[0], np.cumsum(counts)])
    pts = np.array([2.5, 2.0, 1.5]) + rng.normal(scale=0.9, size=(sum(counts), 3))
    cols = rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    # more than 256 points in one tile: the first 300 of frame 0 are pushed into the top left tile of view 0
    cam_pts = np.stack([at_pixel(u, w_, z) for u, w_, z in zip(rng.uniform(2, 28, 300), rng.uniform(2, 28, 300), rng.uniform(0.4, 2.4, 300))])
    pts[:300] = cam_pts @ c2w[0][:3, :3].T + c2w[0][:3, 3]
    got, owner = point_case(E, rgb, depth, pts, cols, offsets, c2w, near=0.3, far=2.5)          # a base per frame
    assert len(np.unique(owner[0][:32, :32])) > 10                                              # the mesh hides most of them
    blank, owner_b = point_case(E, np.full((H, W, 3), 255, np.uint8), np.zeros((H, W), np.float32), pts, cols, offsets, c2w, near=0.3, far=2.5)
    assert len(np.unique(owner_b[0][:32, :32])) > 100                                           # over an empty base: every point is a candidate
    assert np.array_equal(got[1], rgb[1]) and (owner[1] == -1).all()                           # the empty frame copies its base
    assert (owner[2] >= 0).any() and owner[2].max() < 37
    hidden = sum(len(np.setdiff1d(np.arange(n), np.unique(o))) for n, o in zip(counts, owner))
    assert hidden > 50                                                                           # the depth test hides some
    shared, owner_s = point_case(E, rgb[0], depth[0], pts, cols, offsets, c2w, near=0.3, far=2.5)   # one shared base
    assert np.array_equal(shared[0], got[0]) and np.array_equal(shared[1], rgb[0])
    # no points at all, and run-to-run equality
    none, _ = point_case(E, rgb, depth, np.zeros((0, 3)), np.zeros((0, 3), np.uint8), [0, 0, 0, 0], c2w, near=0.3, far=2.5)
    assert np.array_equal(none, rgb)
    again = viewer.draw_points(rgb, depth, pts, cols, offsets, c2w, *CAM, near=0.3, far=2.5, engine=E).numpy()
    assert np.array_equal(again, got)


# ---- the scene around the mesh --------------------------------------------------------------------------------------------
def test_camera_actor_and_viewer_pose_by_hand():
    pts, col = viewer.camera_actor(np.eye(4), 0.5, is_gt=False)
    assert pts.shape == (1200, 3) and list(col) == [255, 0, 0]
    assert list(viewer.camera_actor(np.eye(4), 0.5, is_gt=True)[1]) == [0, 0, 0]
    # segment 0: corner 1 (-1, -1, 1.5) to corner 2 (1, -1, 1.5), scaled by 0.5, 100 points with both ends
    assert np.allclose(pts[0], [-0.5, -0.5, 0.75]) and np.allclose(pts[99], [0.5, -0.5, 0.75])
    assert np.allclose(pts[33], [-0.5 + 33 / 99, -0.5, 0.75])
    # segment 6: corner 1 to the apex; segment 10: (-0.5, 1, 1.5) to the tip (0, 1.2, 1.5); segment 11: the tip to (0.5, 1, 1.5)
    assert np.allclose(pts[600], [-0.5, -0.5, 0.75]) and np.allclose(pts[699], [0, 0, 0])
    assert np.allclose(pts[1000], [-0.25, 0.5, 0.75]) and np.allclose(pts[1099], [0, 0.6, 0.75])
    assert np.allclose(pts[1100], [0, 0.6, 0.75]) and np.allclose(pts[1199], [0.25, 0.5, 0.75])
    # moved by a pose: a quarter turn about z and a shift
    pose = np.array([[0.0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    moved, _ = viewer.camera_actor(pose, 0.5)
    assert np.allclose(moved[0], [0.5 + 1, -0.5 + 2, 0.75 + 3])
    # the viewer: 2 m along the z column, then the y and z columns negated
    first = np.array([[1.0, 0, 0, 1], [0, 0, -1, 2], [0, 1, 0, 3], [0, 0, 0, 1]])             # z column (0, -1, 0)
    keep = first.copy()
    want = np.array([[1.0, 0, 0, 1], [0, 0, 1, 0], [0, -1, 0, 3], [0, 0, 0, 1]])
    assert np.allclose(viewer.viewer_pose(first), want) and np.array_equal(first, keep)
    scaled = first.copy()
    scaled[:3, 2] *= 3.0                                                                      # the z column is normalised for the step
    assert np.allclose(viewer.viewer_pose(scaled)[:3, 3], [1, 0, 3])
    assert np.allclose(viewer.default_camera(540, 960), (270 / np.tan(np.pi / 6), 270 / np.tan(np.pi / 6), 479.5, 269.5))


def toy_run(n=12):
    """poses in the run's convention (x right, y up, z backwards) walking through the room, looking along +x"""
    est, gt = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    for i in range(n):
        for lst, wob in ((est, 0.03 * np.sin(i)), (gt, 0.0)):
            m = R.look_from([0.8 + 0.25 * i, 2.0 + wob, 1.4], [5.0, 2.0 + wob, 1.4])
            m[:3, 1] *= -1
            m[:3, 2] *= -1
            lst[i] = m
    return est, gt


@pytest.mark.parametrize("view", ["first", "follow"])
def test_replay_toy_run(E, view):
    est, gt = toy_run()
    rng = np.random.default_rng(5)
    meshes = {0: oriented_room((5, 4, 3)), 6: oriented_room((6, 5, 4), ROOM_LO - 0.25, ROOM_HI + 0.25)}
    meshes = {i: (v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8)) for i, (v, f) in meshes.items()}
    rp = viewer.Replay(est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, width=W, height=H, view=view, engine=E)
    cam = viewer.default_camera(H, W)
    keep = est.copy()
    for i in range(12):
        if i in meshes:
            rp.update_mesh(meshes[i])
        rp.update_pose(1, est[i], gt=False)
        rp.update_pose(1, gt[i], gt=True)
        if i % 10 == 0:
            rp.update_cam_trajectory(i, gt=False)
            rp.update_cam_trajectory(i, gt=True)
        rp.snapshot()
    got = rp.flush().numpy()
    assert got.shape == (12, H, W, 3) and got.dtype == np.uint8 and np.array_equal(est, keep)
    assert rp.flush().shape[0] == 0
    # the restatement: the same walk, every frame drawn on its own
    mesh, traj = None, {}
    shares = []
    for i in range(12):
        if i in meshes:
            v, f, c = meshes[i]
            f = f[:, ::-1]
            mesh = (v, f, c, viewer.vertex_normals(v, f, engine=E).numpy(), 0.01 * float((v.max(0) - v.min(0)).max()))
        poses = []
        for lst in (est, gt):
            m = lst[i].copy()
            m[:3, 2] *= -1
            poses.append(m)
        if i % 10 == 0:
            traj = {False: est[1:i, :3, 3], True: gt[1:i, :3, 3]}
        parts = [viewer.camera_actor(poses[0], 0.3, False)[0], viewer.camera_actor(poses[1], 0.3, True)[0], traj[False], traj[True]]
        cols = np.concatenate([np.broadcast_to(np.array(c, np.uint8), p.shape) for p, c in zip(parts, ((255, 0, 0), (0, 0, 0)) * 2)])
        pts = np.concatenate(parts)
        eye = viewer.viewer_pose(est[0] if view == "first" else est[i])[None]
        v, f, c, nrm, near = mesh
        base = V.render_mesh_views(v, f, eye, H, W, *cam, near, 1000.0, nrm, c, "back")
        want, _ = V.draw_points(base[0][0], base[1][0], pts, cols, [0, len(pts)], eye, *cam, near, 1000.0, 4)
        diff = np.abs(got[i].astype(np.int32) - want[0].astype(np.int32))
        assert diff.max() <= 1
        shares.append(float((diff > 0).mean()))
        point_pixels = (want[0] != base[0][0]).any(-1)
        assert np.array_equal(got[i][point_pixels], want[0][point_pixels])              # the colours of point pixels: exact
    assert max(shares) <= SHARE_CAP
    assert (got[5] != got[6]).any() and (got[0] != 255).any()
    # frame(): the scene as it is; reset() drops the cameras
    last = rp.frame().numpy()
    assert np.array_equal(last, got[11])
    rp.reset()
    assert (rp.frame().numpy() != last).any()


def test_replay_without_a_mesh_and_save(E, tmp_path):
    est, gt = toy_run(3)
    rp = viewer.Replay(est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, width=W, height=H, engine=E)
    assert (rp.frame().numpy() == 255).all()                                 # nothing to draw: white
    rp.update_pose(1, est[1])
    img = rp.frame().numpy()
    assert ((img == [255, 0, 0]).all(-1)).any() and (((img == 255).all(-1)) | ((img == [255, 0, 0]).all(-1))).all()
    rp.save(str(tmp_path / "a.jpg"))
    from PIL import Image
    assert Image.open(str(tmp_path / "a.jpg")).size == (W, H)
    with pytest.raises(ValueError, match="view"):
        viewer.Replay(est[0], view="orbit", engine=E)


# ---- the ABI and the command line -----------------------------------------------------------------------------------------
def test_abi_errors(E):
    lib = E.lib
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, (2, 2, 2))
    c2w = R.look_from([2.5, 2.0, 1.5], [4.0, 2.0, 1.5])
    with pytest.raises(_capi.NsrError, match="empty mesh"):
        viewer.render_mesh(v, f[:0], c2w, H, W, engine=E)
    with pytest.raises(_capi.NsrError, match="no views"):
        viewer.render_mesh(v, f, np.zeros((0, 4, 4)), H, W, engine=E)
    with pytest.raises(_capi.NsrError, match="near"):
        viewer.render_mesh(v, f, c2w, H, W, near=0.0, engine=E)
    with pytest.raises(_capi.NsrError, match="cull"):
        viewer.render_mesh(v, f, c2w, H, W, cull="sideways", engine=E)
    with pytest.raises(_capi.NsrError, match="empty mesh"):
        viewer.vertex_normals(v, f[:0], engine=E)
    with pytest.raises(_capi.NsrError, match="out of range"):
        viewer.vertex_normals(v, f + len(v), engine=E)
    with pytest.raises(_capi.NsrError, match="no views"):
        viewer.draw_points(np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.float32), np.zeros((0, 3)), np.zeros((0, 3), np.uint8), [0],
                           np.zeros((0, 4, 4)), engine=E)
    assert lib.nsr_view_workspace_bytes(len(v), 0, 1, H, W) == -1
    assert lib.nsr_view_workspace_bytes(len(v), len(f), 0, H, W) == -1
    assert lib.nsr_view_workspace_bytes(len(v), len(f), 1, 2000, W) == -1
    assert lib.nsr_view_workspace_bytes(len(v), len(f), 3, H, W) == lib.nsr_raster_workspace_bytes(len(v), len(f), 3, H, W) > 0
    vt, ft = torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)
    w = torch.from_numpy(R.w2c_rows(c2w))
    ws = torch.zeros(int(lib.nsr_view_workspace_bytes(len(v), len(f), 1, H, W)), dtype=torch.uint8)
    nrm = torch.zeros((len(v), 3), dtype=torch.float32)
    bins = torch.zeros(4096, dtype=torch.int32)
    depth, face, rgb = torch.zeros((H, W)), torch.zeros((H, W), dtype=torch.int32), torch.zeros((H, W, 3), dtype=torch.uint8)

    def mesh(K=1, near=0.1, far=20.0, nf=len(f), cull=0, n_entries=0):
        return lib.nsr_view_mesh(vt.data_ptr(), len(v), ft.data_ptr(), nf, w.data_ptr(), K, H, W, *CAM, near, far, ws.data_ptr(),
                                 bins.data_ptr(), n_entries, nrm.data_ptr(), None, cull, depth.data_ptr(), face.data_ptr(), rgb.data_ptr(),
                                 None)

    for kw, msg in ((dict(K=0), b"no views"), (dict(near=0.0), b"near"), (dict(near=0.5, far=0.5), b"near"), (dict(nf=0), b"empty mesh"),
                    (dict(cull=3), b"cull mode"), (dict(cull=-1), b"cull mode"), (dict(n_entries=-1), b"negative")):
        assert mesh(**kw) != 0
        assert msg in lib.nsr_last_error(), (kw, lib.nsr_last_error())
    assert mesh() == 0 and (face.numpy() == -1).all()                        # no entries: the background
    assert lib.nsr_view_normals(vt.data_ptr(), len(v), ft.data_ptr(), 0, None, None, 0, None, nrm.data_ptr(), None) != 0
    assert b"empty mesh" in lib.nsr_last_error()
    assert lib.nsr_view_normals(vt.data_ptr(), len(v), ft.data_ptr(), len(f), None, None, 0, None, nrm.data_ptr(), None) != 0
    assert b"null" in lib.nsr_last_error()
    off = torch.zeros(2, dtype=torch.int64)

    def points(B=1, near=0.1, far=20.0, size=4, h=H):
        return lib.nsr_view_points(None, None, 0, off.data_ptr(), w.data_ptr(), B, h, W, *CAM, near, far, size, rgb.data_ptr(),
                                   depth.data_ptr(), 0, rgb.data_ptr(), None, None)

    for kw, msg in ((dict(B=0), b"no views"), (dict(near=-1.0), b"near"), (dict(near=3.0, far=2.0), b"near"), (dict(size=0), b"size"),
                    (dict(size=65), b"size"), (dict(h=2000), b"1..1024")):
        assert points(**kw) != 0
        assert msg in lib.nsr_last_error(), (kw, lib.nsr_last_error())


def test_cli_help(capsys):
    with pytest.raises(SystemExit) as e:
        viewer.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for opt in ("--output", "--scale", "--config", "--no_gt_traj", "--size", "--view", "--every"):
        assert opt in out


def test_config_scale_follows_inherit_from(tmp_path):
    (tmp_path / "base.yaml").write_text("scale: 2.5\ndata:\n  output: x\n")
    (tmp_path / "scene.yaml").write_text(f"inherit_from: {tmp_path / 'base.yaml'}\ndata:\n  output: y\n")
    (tmp_path / "own.yaml").write_text(f"inherit_from: {tmp_path / 'base.yaml'}\nscale: 4\n")
    (tmp_path / "none.yaml").write_text("data:\n  output: z\n")
    assert viewer.config_scale(str(tmp_path / "scene.yaml")) == 2.5
    assert viewer.config_scale(str(tmp_path / "own.yaml")) == 4.0
    assert viewer.config_scale(str(tmp_path / "none.yaml")) == 1.0
