"""CPU tests of the mesh-bound kernels (nice_slam_amd/csrc/nsr_bound.h) and of nice_slam_amd.bound, executed under the emulator
(tests/emu/) at small sizes: an analytic room ray-cast to 60 x 80 depth maps, every stage against the numpy restatement in
tests/bound_reference.py (touched units and touch bits exact, tsdf / weight and surface points bit for bit), the host
quickhull against scipy's Qhull, the point-in-hull test against a half-space test and Delaunay, and the C ABI's error paths."""
import ctypes as C

import numpy as np
import pytest
import torch

pytest.importorskip("scipy")
from scipy.spatial import ConvexHull, Delaunay  # noqa: E402

import bound_reference as R  # noqa: E402
import emu_harness  # noqa: E402
from nice_slam_amd import _capi, bound  # noqa: E402
from nice_slam_amd.engine import Engine  # noqa: E402

H, W, FX, FY, CX, CY = 60, 80, 40.0, 40.0, 39.5, 29.5
SCALE = 4.0                                    # voxel_length 1/32 m: the 5 x 4 x 3 m room is 10 x 8 x 6 units


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module", params=[3, 6])
def scene(request, E):
    kfs = R.room_keyframes(request.param, H, W, FX, FY, CX, CY, seed=request.param)
    depth = np.stack([k["depth"] for k in kfs])
    assert (depth == 0).any() and (depth > 0).any()              # frame 1 carries a block of invalid depth
    c2w, w2c, cams = R.poses(kfs)
    vl, tr = 4 * SCALE / 512, 0.04 * SCALE
    units, touch = R.touched(depth, c2w, FX, FY, CX, CY, vl, tr)
    ts, ws = R.integrate(units, touch, depth, w2c, FX, FY, CX, CY, vl, tr)
    pts = R.surface(units, ts, ws, vl)
    vol = bound.tsdf_fuse(kfs, H, W, FX, FY, CX, CY, SCALE, engine=E)
    return dict(kfs=kfs, cams=cams, vl=vl, units=units, touch=touch, tsdf=ts, weight=ws, surf=pts, vol=vol)


def test_touched_units_exact(scene):
    vol = scene["vol"]
    assert np.array_equal(vol.units.numpy(), scene["units"])
    assert np.array_equal(vol.touch.numpy().view(np.uint32), scene["touch"])
    K = len(scene["kfs"])
    assert scene["touch"].shape[1] == (K + 31) // 32
    # the per-(unit, frame) rule matters: some unit is touched by some frames and not by others
    bits = np.stack([(scene["touch"][:, 0] >> k) & 1 for k in range(K)], 1)
    assert (bits.sum(1) < K).any() and (bits.sum(1) > 0).all()


def test_integration_bit_for_bit(scene):
    vol = scene["vol"]
    assert np.array_equal(vol.weight.numpy(), scene["weight"])
    assert np.array_equal(vol.tsdf.numpy().view(np.uint32), scene["tsdf"].view(np.uint32))
    w = scene["weight"]
    assert (w > 0).sum() > 10000 and ((w > 1).any() or len(scene["kfs"]) < 6)


def test_surface_points_exact_in_order(scene):
    got = bound.surface_points(scene["vol"]).numpy()
    assert got.shape == scene["surf"].shape and len(got) > 1000
    assert np.array_equal(got, scene["surf"])
    # on the room's geometry: nearly every point lies within two voxels of a wall, the table or the sphere (a TSDF also has
    # zero crossings at the far edge of the truncation band behind thin geometry, as Open3D's does)
    lo, hi = R.ROOM_LO, R.ROOM_HI
    wall = np.min(np.minimum(np.abs(got - lo), np.abs(got - hi)), 1)
    tab = np.max(np.abs(got - R.TABLE_C) - R.TABLE_H, 1)
    c, r = R.SPHERES[0]
    sph = np.abs(np.linalg.norm(got - c, axis=1) - r)
    near = np.minimum(np.minimum(wall, np.abs(tab)), sph) < 2 * scene["vl"]
    assert near.mean() > 0.9, near.mean()


def test_bound_from_frames_matches_scipy(scene, E):
    b = bound.bound_from_frames(scene["kfs"], H, W, FX, FY, CX, CY, SCALE, 1.02, engine=E)
    pts = np.concatenate([scene["cams"], scene["surf"]])
    h = ConvexHull(pts)
    sv, _ = R.scipy_bound(pts, 1.02)
    assert len(b.vertices) == len(h.vertices)
    assert np.array_equal(np.sort(b.vertices, 0), np.sort(sv, 0))
    assert b.stats["prefiltered"] < b.stats["points"] and b.stats["hull_vertices"] == len(h.vertices)
    # outward faces: every vertex is behind (or on) every plane
    d = b.vertices @ b.planes[:, :3].T + b.planes[:, 3]
    assert d.max() <= 1e-9
    # contains: numpy in / numpy out, tensor in / tensor out; the half-space test exactly, Delaunay away from the boundary
    q = np.random.default_rng(1).uniform(R.ROOM_LO - 1, R.ROOM_HI + 1, (20000, 3))
    got = b.contains(q)
    assert isinstance(got, np.ndarray) and got.dtype == bool
    assert np.array_equal(got, R.halfspace_contains(b.planes, q))
    far = np.abs(q @ b.planes[:, :3].T + b.planes[:, 3]).min(1) > 1e-9
    assert np.array_equal(got[far], Delaunay(b.vertices).find_simplex(q[far]) >= 0)
    t = b(torch.from_numpy(q.astype(np.float32)))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.bool
    assert np.array_equal(t.numpy(), R.halfspace_contains(b.planes, q.astype(np.float32)))
    assert got.any() and not got.all()


def _vol(v, f):
    return abs(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)


def test_hull_general_position(E):
    rng = np.random.default_rng(3)
    for n in (4, 50, 2000):
        p = rng.normal(size=(n, 3))
        v, vi, f, pl = bound.convex_hull(p, 1.0, lib=E.lib)
        h = ConvexHull(p)
        assert np.array_equal(vi, np.sort(h.vertices))
        assert len(f) == 2 * len(v) - 4
        assert abs(_vol(v, f) - h.volume) <= 1e-12 * h.volume
        # deterministic
        v2, vi2, f2, pl2 = bound.convex_hull(p, 1.0, lib=E.lib)
        assert np.array_equal(f, f2) and np.array_equal(pl, pl2)


def test_hull_degenerate(E):
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    g = np.linspace(0, 1, 6)
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(4)
    walls = []
    for d in range(3):                                           # points ON the faces of a 5 x 4 x 3 box, and inside it
        for s in (0.0, 1.0):
            q = rng.uniform(size=(300, 3))
            q[:, d] = s
            walls.append(q)
    walls = np.concatenate(walls + [rng.uniform(size=(500, 3))]) * np.array([5.0, 4.0, 3.0])
    for P in (cube, np.concatenate([cube, cube, cube[:3]]), grid, walls, np.concatenate([walls, walls[:100]])):
        v, vi, f, pl = bound.convex_hull(P, 1.0, lib=E.lib)
        ref = ConvexHull(P).volume
        assert abs(_vol(v, f) - ref) <= 1e-12 * ref
        # no input point is outside its own hull by more than the quickhull tolerance (points ON a face may round either way)
        tol = bound.HULL_TOL_REL * np.abs(P).max(0).sum()
        assert (P @ pl[:, :3].T + pl[:, 3]).max() <= tol
    v, _, _, _ = bound.convex_hull(cube, 1.02, lib=E.lib)         # scaled about the mean of the vertices
    assert np.allclose(np.sort(v, 0)[[0, -1]], [[-0.01] * 3, [1.01] * 3], atol=1e-15)


def test_prefilter_keeps_every_hull_vertex(E):
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.normal(size=(5000, 3)), rng.uniform(-0.5, 0.5, (5000, 3))])
    kept = bound.prefilter(torch.from_numpy(p), E).numpy()
    h = ConvexHull(p)
    assert len(kept) < len(p)
    assert set(map(tuple, p[h.vertices])) <= set(map(tuple, kept))
    # survivors keep their input order
    idx = np.nonzero((p[:, None, :] == kept[None, :100, :]).all(2))[0]
    assert np.all(np.diff(idx) > 0)


def test_abi_errors(E):
    lib = E.lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    cnt = np.zeros(2, np.int64)
    buf = np.zeros((64, 4))
    vi = np.zeros(64, np.int64)
    fc = np.zeros((64, 3), np.int32)
    three = np.eye(3)
    assert lib.nsr_convex_hull(P(three), 3, 0.0, 1.0, P(cnt), P(buf), P(vi), P(fc), P(buf)) != 0
    assert b"no volume" in lib.nsr_last_error()
    plane = np.random.default_rng(0).uniform(size=(20, 3))
    plane[:, 2] = 0.5
    assert lib.nsr_convex_hull(P(plane), 20, 1e-12, 1.0, P(cnt), P(buf), P(vi), P(fc), P(buf)) != 0
    bad = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, np.nan]], np.float64)
    assert lib.nsr_convex_hull(P(bad), 4, 0.0, 1.0, P(cnt), P(buf), P(vi), P(fc), P(buf)) != 0
    assert lib.nsr_convex_hull(P(bad), 4, 0.0, 0.0, P(cnt), P(buf), P(vi), P(fc), P(buf)) != 0
    assert lib.nsr_tsdf_workspace_bytes((C.c_int32 * 6)(0, 0, 0, -1, 0, 0)) == -1
    assert lib.nsr_tsdf_workspace_bytes((C.c_int32 * 6)(0, 0, 0, 4095, 4095, 4095)) == -1       # 2^36 units
    assert lib.nsr_tsdf_workspace_bytes((C.c_int32 * 6)(-2, 0, 0, 1, 0, 0)) > 0
    d = np.zeros((1, 4, 4), np.float32)
    c2w = np.zeros((1, 12))
    box = np.zeros(6, np.int32)
    assert lib.nsr_tsdf_unit_box(P(d), 0, 4, 4, P(c2w), 1.0, 1.0, 0.0, 0.0, 0.01, 0.1, P(box), None) != 0
    assert lib.nsr_tsdf_unit_box(P(d), 1, 4, 4, P(c2w), 1.0, 1.0, 0.0, 0.0, -0.01, 0.1, P(box), None) != 0
    assert lib.nsr_tsdf_unit_box(P(d), 1, 4, 4, None, 1.0, 1.0, 0.0, 0.0, 0.01, 0.1, P(box), None) != 0
    assert lib.nsr_tsdf_integrate(P(d), 1, 4, 4, None, 1.0, 1.0, 0.0, 0.0, 0.01, 0.1, None, None, 1, None, None, None) != 0
    assert lib.nsr_tsdf_integrate(P(d), 1, 4, 4, None, 1.0, 1.0, 0.0, 0.0, 0.01, 0.1, None, None, -1, None, None, None) != 0
    pts = np.zeros((4, 3))
    keep = np.zeros(4, np.uint8)
    assert lib.nsr_hull_prefilter(P(pts), 4, (C.c_double * 260)(), 65, 0.0, P(keep), None) != 0
    assert lib.nsr_hull_prefilter(P(pts), 4, (C.c_double * 4)(), 1, -1.0, P(keep), None) != 0
    assert lib.nsr_hull_extremes(P(pts), 0, None, None, None) != 0
    assert lib.nsr_hull_contains(P(pts), -1, 1, None, 0, P(keep), None) != 0
    assert lib.nsr_hull_contains(P(pts), 4, 1, None, 3, P(keep), None) != 0
    # an empty hull test set: every point is inside
    assert lib.nsr_hull_contains(P(pts), 4, 1, None, 0, P(keep), None) == 0 and keep.all()
    # no valid depth anywhere: an empty volume, no surface
    kfs = [{"est_c2w": np.eye(4), "depth": np.zeros((H, W), np.float32)}]
    vol = bound.tsdf_fuse(kfs, H, W, FX, FY, CX, CY, SCALE, engine=E)
    assert vol.units.shape == (0, 3) and bound.surface_points(vol).shape == (0, 3)
    with pytest.raises(_capi.NsrError):
        bound.convex_hull(three, lib=lib)
