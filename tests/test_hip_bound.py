"""GPU tests of the mesh bound from keyframes (nice_slam_amd.bound, include/nsr.h "Mesh bound from keyframes"): a Replica-sized
room (680 x 1200, 50 keyframes) through every stage against the numpy restatement in tests/bound_reference.py and scipy's
hull, run-to-run determinism, Mesher.get_mesh(mesh_bound="frames") against the same call with a scipy-hull callable in both
branches that read the bound, and a 512^3 lattice through the point-in-hull test."""
import time

import numpy as np
import pytest
import torch

pytest.importorskip("scipy")
from scipy.spatial import ConvexHull, Delaunay  # noqa: E402

import bound_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W, FX, FY, CX, CY = 680, 1200, 600.0, 600.0, 599.5, 339.5      # Replica's camera
SCALE = 1.0


@pytest.fixture(scope="module")
def room():
    from nice_slam_amd import bound
    kfs = R.room_keyframes(50, H, W, FX, FY, CX, CY, seed=7)
    gpu_kfs = [{"est_c2w": torch.from_numpy(k["est_c2w"]).float().to(DEV), "depth": torch.from_numpy(k["depth"]).to(DEV)} for k in kfs]
    for k, g in zip(kfs, gpu_kfs):                                 # the product reads the fp32 pose the tracker would hold
        k["est_c2w"] = g["est_c2w"].cpu().double().numpy()
    vol = bound.tsdf_fuse(gpu_kfs, H, W, FX, FY, CX, CY, SCALE)
    surf = bound.surface_points(vol)
    torch.cuda.synchronize()
    return dict(kfs=kfs, gpu_kfs=gpu_kfs, vol=vol, surf=surf)


@pytest.fixture(scope="module")
def ref(room):
    kfs = room["kfs"]
    depth = np.stack([k["depth"] for k in kfs])
    c2w, w2c, cams = R.poses(kfs)
    vl, tr = 4 * SCALE / 512, 0.04 * SCALE
    units, touch = R.touched(depth, c2w, FX, FY, CX, CY, vl, tr)
    ts, ws = R.integrate(units, touch, depth, w2c, FX, FY, CX, CY, vl, tr)
    return dict(cams=cams, units=units, touch=touch, tsdf=ts, weight=ws, surf=R.surface(units, ts, ws, vl))


def test_stages_equal_the_restatement(room, ref):
    vol = room["vol"]
    assert np.array_equal(vol.units.cpu().numpy(), ref["units"])
    assert np.array_equal(vol.touch.cpu().numpy().view(np.uint32), ref["touch"])
    assert np.array_equal(vol.weight.cpu().numpy(), ref["weight"])
    assert np.array_equal(vol.tsdf.cpu().numpy().view(np.uint32), ref["tsdf"].view(np.uint32))
    assert np.array_equal(room["surf"].cpu().numpy(), ref["surf"])
    assert len(ref["units"]) > 1000 and len(ref["surf"]) > 100000


def test_two_runs_bit_identical(room):
    from nice_slam_amd import bound
    vol = bound.tsdf_fuse(room["gpu_kfs"], H, W, FX, FY, CX, CY, SCALE)
    surf = bound.surface_points(vol)
    for a, b in ((vol.units, room["vol"].units), (vol.touch, room["vol"].touch), (vol.tsdf, room["vol"].tsdf),
                 (vol.weight, room["vol"].weight), (surf, room["surf"])):
        assert torch.equal(a, b)
    b1 = bound.bound_from_frames(room["gpu_kfs"], H, W, FX, FY, CX, CY, SCALE, 1.02)
    b2 = bound.bound_from_frames(room["gpu_kfs"], H, W, FX, FY, CX, CY, SCALE, 1.02)
    assert np.array_equal(b1.vertices, b2.vertices) and np.array_equal(b1.faces, b2.faces) and np.array_equal(b1.planes, b2.planes)


def test_hull_against_scipy(room, ref):
    from nice_slam_amd import bound
    b = bound.bound_from_frames(room["gpu_kfs"], H, W, FX, FY, CX, CY, SCALE, 1.02)
    pts = np.concatenate([ref["cams"], ref["surf"]])
    h = ConvexHull(pts)
    sv, _ = R.scipy_bound(pts, 1.02)
    print("bound stats", b.stats, "scipy vertices", len(h.vertices))
    vol = ConvexHull(b.vertices).volume
    assert abs(vol - ConvexHull(sv).volume) <= 1e-9 * vol
    assert b.stats["prefiltered"] < b.stats["points"]
    q = np.random.default_rng(2).uniform(R.ROOM_LO - 0.5, R.ROOM_HI + 0.5, (200000, 3))
    got = b.contains(torch.from_numpy(q).to(DEV))
    assert got.device.type == "cuda" and got.dtype == torch.bool
    got = got.cpu().numpy()
    assert np.array_equal(got, R.halfspace_contains(b.planes, q))
    far = np.abs(q @ b.planes[:, :3].T + b.planes[:, 3]).min(1) > 1e-6
    assert np.array_equal(got[far], Delaunay(sv).find_simplex(q[far]) >= 0)


def _scipy_callable(kfs, H_, W_, fx, fy, cx, cy, scale, bound_scale):
    """the reference's bound restated with scipy: Qhull's hull of the camera centres and the TSDF surface points, scaled about
    the mean of its vertices, tested with its facet equations (inside: every signed distance <= 0)"""
    from nice_slam_amd import bound
    vol = bound.tsdf_fuse(kfs, H_, W_, fx, fy, cx, cy, scale)
    pts = np.concatenate([vol.cams, bound.surface_points(vol).cpu().numpy()])
    _, eq = R.scipy_bound(pts, bound_scale)
    return lambda p: R.halfspace_contains(eq, p)


@pytest.mark.parametrize("show_forecast", [False, True])
def test_get_mesh_frames_equals_scipy_bound(tmp_path, show_forecast):
    from test_hip_mesher import _setup
    sc, m, dec, grids, kfs, est = _setup(96, True, False)
    cb = _scipy_callable(kfs, m.H, m.W, m.fx, m.fy, m.cx, m.cy, m.scale, m.clean_mesh_bound_scale)
    got = m.get_mesh(str(tmp_path / "a.ply"), grids, dec, kfs, est, 1, DEV, show_forecast=show_forecast, mesh_bound="frames")
    want = m.get_mesh(str(tmp_path / "b.ply"), grids, dec, kfs, est, 1, DEV, show_forecast=show_forecast, mesh_bound=cb)
    free = m.get_mesh(str(tmp_path / "c.ply"), grids, dec, kfs, est, 1, DEV, show_forecast=show_forecast, mesh_bound=None)
    assert got is not None and want is not None
    for a, b in zip(got, want):
        assert (a is None and b is None) or torch.equal(a, b)
    assert open(tmp_path / "a.ply", "rb").read() == open(tmp_path / "b.ply", "rb").read()
    assert free is not None and free[1].shape != got[1].shape           # the bound changes the mesh
    # a ConvexBound passed directly is the same as "frames"
    hull = m.bound_from_frames(kfs, m.scale)
    again = m.get_mesh(str(tmp_path / "d.ply"), grids, dec, kfs, est, 1, DEV, show_forecast=show_forecast, mesh_bound=hull)
    assert all(torch.equal(a, b) for a, b in zip(got[:2], again[:2]))
    with pytest.raises(NotImplementedError, match="bound_from_frames"):
        m.get_bound_from_frames(kfs, 1.0)


def test_contains_512_lattice(room):
    from nice_slam_amd import bound
    from nice_slam_amd.mesher import Mesher  # noqa: F401
    b = bound.bound_from_frames(room["gpu_kfs"], H, W, FX, FY, CX, CY, SCALE, 1.02)
    ax = [torch.linspace(float(R.ROOM_LO[d]) - 0.3, float(R.ROOM_HI[d]) + 0.3, 512, dtype=torch.float64, device=DEV) for d in range(3)]
    yy, xx, zz = torch.meshgrid(ax[1], ax[0], ax[2], indexing="ij")
    pts = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 1).float()
    del xx, yy, zz
    b.contains(pts[:1000])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inside = b.contains(pts)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"contains 512^3: {dt * 1e3:.1f} ms over {b.planes.shape[0]} planes, {float(inside.float().mean()):.3f} inside")
    assert inside.shape == (512 ** 3,) and inside.any() and not inside.all()
    sel = torch.from_numpy(np.random.default_rng(3).integers(0, 512 ** 3, 200000)).to(DEV)
    assert np.array_equal(inside[sel].cpu().numpy(), R.halfspace_contains(b.planes, pts[sel].cpu().numpy()))
