"""CPU tests of the depth rasterizer and the 2-D depth metric (nice_slam_amd/csrc/nsr_raster.h, nice_slam_amd/raster.py),
executed under the emulator (tests/emu/) at small sizes: depth stacks and per-view means against the numpy restatement
(tests/raster_reference.py) bit for bit, a closed room that must come out watertight and match an fp64 ray cast, candidate
views and verdicts against a golden minted from the reference's eval_recon.py (tests/golden/make_golden_depth.py), the
oriented box, the metric end to end, the ABI's error paths and the command line."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull

import emu_harness
import raster_reference as R
from nice_slam_amd import _capi, raster, recon
from nice_slam_amd.engine import Engine, gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "depth_eval.npz")
H, W, FX, FY, CX, CY = 48, 64, 40.0, 42.0, 31.5, 23.5
ROOM_LO, ROOM_HI = np.array([0.0, 0.0, 0.0]), np.array([5.0, 4.0, 3.0])


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


def render(E, v, f, c2w, near, far=20.0):
    return raster.render_depth(v, f, c2w, H, W, FX, FY, CX, CY, near=near, far=far, engine=E).numpy()


def mixed_scene(rng):
    """a room, loose triangles around the camera (some crossing the near plane, some behind it, some beyond far) and
    degenerate faces (a repeated index, three collinear vertices, a zero-area sliver)"""
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, (6, 5, 4))
    extra_v, extra_f = [], []
    base = len(v)
    cam = np.array([2.5, 2.0, 1.5])
    for _ in range(120):
        c = cam + rng.normal(scale=1.2, size=3)
        tri = c + rng.normal(scale=0.5, size=(3, 3))
        extra_f.append([base + len(extra_v), base + len(extra_v) + 1, base + len(extra_v) + 2])
        extra_v.extend(tri)
    # big triangles straddling the camera's plane and one far beyond the far plane
    for tri in ([[2.0, 1.0, 1.5], [3.2, 2.5, 1.4], [2.4, 3.0, 1.6]],
                [[1.0, 2.0, 0.5], [4.0, 2.2, 0.6], [2.5, 5.0, 2.5]],
                [[40.0, -30.0, -5.0], [45.0, 30.0, -5.0], [40.0, 0.0, 30.0]]):
        extra_f.append([base + len(extra_v), base + len(extra_v) + 1, base + len(extra_v) + 2])
        extra_v.extend(tri)
    k = base + len(extra_v)
    extra_v.extend([[3.5, 2.0, 1.0], [3.6, 2.1, 1.2], [3.7, 2.2, 1.4], [3.5, 2.5, 1.0]])
    extra_f.extend([[k, k, k + 3], [k, k + 1, k + 2], [k + 3, k + 3, k + 3]])
    return np.concatenate([v, np.array(extra_v)]), np.concatenate([f, np.array(extra_f, np.int32)])


def views(rng, n):
    out = []
    for _ in range(n):
        eye = np.array([2.5, 2.0, 1.5]) + rng.uniform(-0.6, 0.6, 3)
        out.append(R.look_from(eye, eye + rng.normal(size=3)))
    return np.stack(out)


def test_depth_matches_restatement(E):
    rng = np.random.default_rng(1)
    v, f = mixed_scene(rng)
    c2w = views(rng, 6)
    near, far = 0.3, 2.5
    got = render(E, v, f, c2w, near, far)
    want = R.render_views(v, f, c2w, H, W, FX, FY, CX, CY, near, far)
    assert got.dtype == np.float32 and got.shape == (6, H, W)
    assert np.array_equal(got, want)
    # the cases are there: faces crossing near, wholly behind the camera, and fragments cut by far
    w = R.w2c_rows(c2w)
    z = np.stack([R.vertex_pass(v, w[k])[:, 2][f] for k in range(len(w))])      # [K, F, 3]
    assert ((z.min(2) < near) & (z.max(2) > near)).any()
    assert (z.max(2) < 0).any()
    assert (z.max(2) > far).any() and (got == 0).any() and (got > 0).mean() > 0.5
    # every view is bit-identical run to run
    assert np.array_equal(render(E, v, f, c2w, near, far), got)
    # the per-view means
    other = render(E, v[::-1].copy(), (len(v) - 1 - f)[:, ::-1].copy(), c2w, near, far)
    l1 = raster.depth_l1(torch.from_numpy(got), torch.from_numpy(other * np.float32(1.01)), E).numpy()
    assert np.array_equal(l1, R.depth_l1(got, other * np.float32(1.01)))


BATCH_NEAR, BATCH_FAR = 0.3, 2.5


def batch_case():
    """the mixed scene and three of eight views, the one with the fewest bin entries last (counted on the CPU with the
    restatement's pixel boxes): drawn two views a launch, the second batch is smaller than the workspace it reuses and its
    entries end before the first batch's do in the reused bins"""
    rng = np.random.default_rng(1)
    v, f = mixed_scene(rng)
    cand = views(rng, 8)
    n = np.array([R.bin_entries(v, f, w, H, W, FX, FY, CX, CY, BATCH_NEAR) for w in R.w2c_rows(cand)])
    order = np.argsort(n, kind="stable")
    pick = [order[-1], order[-2], order[0]]
    assert n[pick[2]] < n[pick[1]] <= n[pick[0]]
    return v, f, cand[pick]


def check_depth_batches(E):
    """render_depth two views a launch against all three at once and the restatement (E: an engine, None: the GPU's)"""
    v, f, c2w = batch_case()
    draw = lambda step: raster.render_depth(v, f, c2w, H, W, FX, FY, CX, CY, near=BATCH_NEAR, far=BATCH_FAR, engine=E,
                                            views_per_launch=step).cpu().numpy()
    two = draw(2)
    assert np.array_equal(two, draw(3))
    assert np.array_equal(two, R.render_views(v, f, c2w, H, W, FX, FY, CX, CY, BATCH_NEAR, BATCH_FAR))
    with pytest.raises(ValueError, match="render_depth: views_per_launch must be positive"):
        draw(0)
    # the loop itself: batches of 2 and 1 in one workspace and one bin array, the last view's entries the fewest
    E = E or gpu()
    scene = raster.checked_scene(E, v, f, c2w, BATCH_NEAR, "test")
    camera = (H, W, FX, FY, CX, CY, BATCH_NEAR, BATCH_FAR)
    with E.guard():
        seen = [(k0, kb, tuple(wk.shape), ws.data_ptr(), bins.data_ptr(), bins.numel(), n)
                for k0, kb, wk, ws, bins, n in raster.binned_batches(E, scene, camera, 2, "test")]
        each = [b[5] for b in raster.binned_batches(E, scene, camera, 1, "test")]
    assert [s[:3] for s in seen] == [(0, 2, (2, 12)), (2, 1, (1, 12))]
    assert seen[0][3:6] == seen[1][3:6] and seen[0][5] >= seen[0][6]
    assert [s[6] for s in seen] == [each[0] + each[1], each[2]] and 0 < each[2] < min(each[:2])


def test_batches_of_views(E):
    check_depth_batches(E)


def test_watertight_room(E):
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, (25, 20, 15))
    rng = np.random.default_rng(2)
    c2w = views(rng, 4)
    got = render(E, v, f, c2w, 0.05)
    assert (got > 0).all()                                                   # no crack anywhere
    cast = np.stack([R.ray_cast_box_inside(c, ROOM_LO, ROOM_HI, H, W, FX, FY, CX, CY) for c in c2w])
    assert np.abs(got / cast - 1).max() < 1e-5
    assert np.array_equal(got, R.render_views(v, f, c2w, H, W, FX, FY, CX, CY, 0.05, 20.0))


def test_views_match_golden(E):
    g = np.load(GOLDEN)
    c2w = raster.views_from_draws(g["extents"], g["transform"], g["draws"])
    assert np.array_equal(c2w, g["c2w"])                                     # bit for bit
    sees = raster.views_unseen(c2w, g["unseen"], engine=E)
    assert np.array_equal(sees, g["seen"])
    assert g["seen"].any() and not g["seen"].all()
    assert [R.check_proj_sees(g["unseen"], c, 500, 500, 300.0, 300.0, 249.5, 249.5) for c in c2w[:60]] == list(g["seen"][:60])
    # the rejection loop: the first n unseen candidates in draw order
    got = raster.sample_views(g["extents"], g["transform"], 25, unseen=g["unseen"], draws=g["draws"], engine=E)
    assert np.array_equal(got, g["c2w"][~g["seen"]][:25])
    assert np.array_equal(raster.sample_views(g["extents"], g["transform"], 5, draws=g["draws"], engine=E), g["c2w"][:5])
    # a seeded stream is reproducible
    a = raster.sample_views(g["extents"], g["transform"], 7, unseen=g["unseen"], seed=3, engine=E)
    assert np.array_equal(a, raster.sample_views(g["extents"], g["transform"], 7, unseen=g["unseen"], seed=3, engine=E))


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_oriented_bounds_of_rotated_box(E):
    rng = np.random.default_rng(4)
    ext = np.array([4.0, 1.5, 2.5])
    v, f = R.box_mesh(-ext / 2, ext / 2, (4, 3, 3))
    Rm, c = rotation(rng), np.array([0.7, -1.2, 2.0])
    vw = v @ Rm.T + c
    to_origin, extents = raster.oriented_bounds(vw, E)
    assert np.allclose(extents, np.sort(ext), rtol=0, atol=1e-9)
    T = np.linalg.inv(to_origin)
    assert np.allclose(T[:3, 3], c, rtol=0, atol=1e-9)
    assert np.allclose(T[:3, :3].T @ T[:3, :3], np.eye(3), atol=1e-12) and np.linalg.det(T[:3, :3]) > 0
    local = (vw - T[:3, 3]) @ T[:3, :3]
    assert np.allclose(np.abs(local).max(0), np.sort(ext) / 2, atol=1e-9)
    # get_cam_position's factors and lift
    e2, t2 = raster.cam_position(vw, f, E)
    assert np.allclose(e2, np.sort(ext) * [0.3, 0.7, 0.7], atol=1e-9)
    assert np.allclose(t2[:3, 3], c + [0, 0, 0.4], atol=1e-9)


def brute_volume(p):
    hull = ConvexHull(p)
    best = np.inf
    for n in hull.equations[:, :3]:
        n = n / np.linalg.norm(n)
        t = np.eye(3)[np.argmin(np.abs(n))]
        u = np.cross(n, t)
        u /= np.linalg.norm(u)
        w = np.cross(n, u)
        q = np.stack([p @ u, p @ w], 1)
        h2 = q[ConvexHull(q).vertices]
        hn = p @ n
        for i in range(len(h2)):
            e = h2[(i + 1) % len(h2)] - h2[i]
            e /= np.linalg.norm(e)
            pe = np.array([-e[1], e[0]])
            a, b = q @ e, q @ pe
            best = min(best, (a.max() - a.min()) * (b.max() - b.min()) * (hn.max() - hn.min()))
    return best


def test_oriented_bounds_volume_is_minimal(E):
    rng = np.random.default_rng(5)
    for _ in range(3):
        p = rng.normal(size=(200, 3)) * [1.0, 2.0, 0.5]
        _, ext = raster.oriented_bounds(p, E)
        assert np.isclose(np.prod(ext), brute_volume(p), rtol=1e-9)
        assert np.all(np.diff(ext) >= 0)


def test_metric_end_to_end(E, tmp_path):
    gv, gf = R.box_mesh(ROOM_LO, ROOM_HI, (10, 8, 6))
    kw = dict(align=False, n_imgs=4, unseen=False, seed=1, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, engine=E)
    same = raster.calc_2d_metric((gv, gf), (gv, gf), **kw)
    assert same["depth_l1_cm"] == 0.0 and np.all(same["per_view"] == 0.0)
    # the floor raised by delta: the restatement's value for the same views
    rv = gv.copy()
    rv[rv[:, 2] == 0.0, 2] = 0.05
    m = raster.calc_2d_metric((rv, gf), (gv, gf), **kw)
    c2w = m["c2w"]
    assert c2w.shape == (4, 4, 4) and np.array_equal(c2w, same["c2w"])
    ext = lambda x: float((x.max(0) - x.min(0)).max())                     # noqa: E731
    a = R.render_views(gv, gf, c2w, H, W, FX, FY, CX, CY, 0.01 * ext(gv), 20.0)
    b = R.render_views(rv, gf, c2w, H, W, FX, FY, CX, CY, 0.01 * ext(rv), 20.0)
    per_view = R.depth_l1(a, b)
    assert np.array_equal(m["per_view"], per_view)
    acc = 0.0
    for x in per_view:
        acc += x
    assert m["depth_l1_cm"] == acc / len(per_view) * 100 and m["depth_l1_cm"] > 0
    # the views lie in the camera box: inside the room, under the lifted centre's slab
    assert np.all((c2w[:, :3, 3] > ROOM_LO) & (c2w[:, :3, 3] < ROOM_HI))
    # the unseen cloud beside a PLY is required by default
    from nice_slam_amd.ply import write_ply
    gt = str(tmp_path / "gt.ply")
    write_ply(gt, gv, gf)
    with pytest.raises(FileNotFoundError, match="_pc_unseen.npy"):
        raster.calc_2d_metric(gt, gt, align=False, n_imgs=1, engine=E)
    np.save(str(tmp_path / "gt_pc_unseen.npy"), np.array([[100.0, 100.0, 100.0]]))
    m2 = raster.calc_2d_metric(gt, gt, align=False, n_imgs=2, seed=1, H=H, W=W, fx=FX, fy=FY, cx=CX, cy=CY, engine=E)
    assert m2["depth_l1_cm"] == 0.0


def test_abi_errors(E):
    lib = E.lib
    v, f = R.box_mesh(ROOM_LO, ROOM_HI, (2, 2, 2))
    c2w = R.look_from([2.5, 2.0, 1.5], [4.0, 2.0, 1.5])
    with pytest.raises(_capi.NsrError, match="empty mesh"):
        raster.render_depth(v, f[:0], c2w, H, W, engine=E)
    with pytest.raises(_capi.NsrError, match="no views"):
        raster.render_depth(v, f, np.zeros((0, 4, 4)), H, W, engine=E)
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(_capi.NsrError, match="out of range"):
        raster.render_depth(v, bad, c2w, H, W, engine=E)
    with pytest.raises(_capi.NsrError, match="near"):
        raster.render_depth(v, f, c2w, H, W, near=0.0, engine=E)
    assert lib.nsr_raster_workspace_bytes(len(v), 0, 1, H, W) == -1
    assert lib.nsr_raster_workspace_bytes(len(v), len(f), 0, H, W) == -1
    assert lib.nsr_raster_workspace_bytes(len(v), len(f), 1, 2000, W) == -1
    vt = torch.from_numpy(v.astype(np.float32))
    ft = torch.from_numpy(f)
    w = torch.from_numpy(R.w2c_rows(c2w))
    ws = torch.zeros(int(lib.nsr_raster_workspace_bytes(len(v), len(f), 1, H, W)), dtype=torch.uint8)
    n = torch.zeros(1, dtype=torch.int64)
    call = lambda K, near, far, nf=len(f): lib.nsr_raster_bin(vt.data_ptr(), len(v), ft.data_ptr(), nf, w.data_ptr(), K, H, W, FX, FY,  # noqa: E731
                                                               CX, CY, near, far, ws.data_ptr(), n.data_ptr(), None)
    for args, msg in (((0, 0.1, 20.0), b"no views"), ((1, 0.0, 20.0), b"near"), ((1, -1.0, 20.0), b"near"), ((1, 0.5, 0.5), b"near"),
                      ((1, 0.1, 20.0, 0), b"empty mesh")):
        assert call(*args) != 0
        assert msg in lib.nsr_last_error()
    assert call(1, 0.1, 20.0) == 0 and int(n[0]) > 0
    assert lib.nsr_depth_error(None, None, 0, 10, None, None, None) != 0
    assert lib.nsr_view_unseen(None, 0, 0, None, 0, H, W, FX, FY, CX, CY, None, None) != 0


def test_cli(capsys):
    with pytest.raises(SystemExit) as e:
        recon.main(["depth", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for opt in ("--rec_mesh", "--gt_mesh", "--unseen", "--no_unseen", "--n_imgs", "--seed", "--no_align"):
        assert opt in out
    with pytest.raises(NotImplementedError, match="recon depth"):
        recon.main(["eval", "--rec_mesh", "a.ply", "--gt_mesh", "b.ply", "-2d"])
