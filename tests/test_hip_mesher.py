"""GPU tests of the mesh extraction (nice_slam_amd.mesher, include/nsr.h "Mesh extraction"): marching cubes bit for bit
against the numpy restatement (tests/mesh_reference.py), and Mesher.get_mesh end to end against a CPU pipeline built from
the GPU's own field, the masks restatement, numpy marching cubes, scipy components and the oracle's colour decode."""
import os
import time
import types

import numpy as np
import pytest
import torch

import mesh_reference as MR
from scene_util import build_product, make_scene, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lattice(n, shift=0.3):
    g = torch.arange(n, dtype=torch.float64) - n / 2 + shift
    return torch.meshgrid(g, g, g, indexing="ij")


def _sphere(n, r):
    X, Y, Z = _lattice(n)
    return (r - torch.sqrt(X ** 2 + Y ** 2 + Z ** 2)).float()


def _torus(n, R, r):
    X, Y, Z = _lattice(n)
    return (r - torch.sqrt((torch.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2)).float()


@pytest.mark.parametrize("name", ["sphere256", "torus256", "noise64"])
def test_marching_cubes_bit_exact_and_deterministic(name):
    from nice_slam_amd import marching_cubes
    if name == "sphere256":
        vol = _sphere(256, 100.0)
    elif name == "torus256":
        vol = _torus(256, 80.0, 30.0)
    else:
        vol = torch.from_numpy(np.random.default_rng(5).standard_normal((64, 64, 64)).astype(np.float32))
        vol[0] = vol[-1] = -5
        vol[:, 0] = vol[:, -1] = -5
        vol[:, :, 0] = vol[:, :, -1] = -5
    sp, org = (0.01, 0.02, 0.015), (-1.25, 0.5, 2.0)
    v1, f1 = marching_cubes(vol.to(DEV), 0.0, sp, org)
    v2, f2 = marching_cubes(vol.to(DEV), 0.0, sp, org)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)
    rv, rf = MR.marching_cubes(vol.numpy(), 0.0, sp, org)
    assert v1.dtype == torch.float64 and f1.dtype == torch.int32
    assert np.array_equal(v1.cpu().numpy(), rv) and np.array_equal(f1.cpu().numpy(), rf)
    if name == "noise64":
        assert set(MR.edge_use_counts(rf).tolist()) == {2}
    else:
        assert MR.euler_characteristic(rv, rf) == (2 if name == "sphere256" else 0)


# ---- get_mesh end to end ----

def _setup(res, depth_test, largest, seed=21):
    from nice_slam_amd import Mesher
    sc = make_scene(seed=seed, n_rays=16, small=True, fine_scale=1.0)
    renderer, dec, grids = build_product(sc, DEV)
    b = sc["bound"].numpy()
    H, W, fx, fy, cx, cy = sc["intr"]
    mc_bound = (b + np.array([[0.1, -0.1]])).tolist()
    cfg = {"coarse": True, "scale": 1.0, "occupancy": True,
           "meshing": {"resolution": res, "level_set": 0.0, "clean_mesh_bound_scale": 1.02, "remove_small_geometry_threshold": 0.002,
                       "color_mesh_extraction_method": "direct_point_query", "get_largest_components": largest, "depth_test": depth_test},
           "mapping": {"marching_cubes_bound": mc_bound}}
    slam = types.SimpleNamespace(renderer=renderer, bound=sc["bound"], nice=True, verbose=False, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy)
    m = Mesher(cfg, None, slam, points_batch_size=50000)
    c2 = sc["c2w"].clone()
    c2[:3, 3] += torch.tensor([0.3, -0.2, 0.25])
    kfs = [{"est_c2w": sc["c2w"], "depth": sc["depth_img"]}, {"est_c2w": c2, "depth": sc["depth_img"].flip(1)}]
    est = torch.stack([sc["c2w"], c2])
    # a level with surface inside the lattice: the median of the fine field
    z = m.eval_points(m.get_grid_uniform(res, DEV)["grid_points"], dec, grids, "fine", DEV)[:, 3]
    m.level_set = float(torch.quantile(z[z < 100].float()[:100000], 0.5))
    return sc, m, dec, grids, kfs, est


def _box(lo, hi):
    lo, hi = np.asarray(lo), np.asarray(hi)
    return lambda p: np.all((p > lo) & (p < hi), axis=1)


def _expected(sc, m, dec, grids, kfs, est, show_forecast, mesh_bound, use_all):
    """The CPU pipeline: GPU field values + restated masks + numpy marching cubes + scipy components."""
    from oracle import nice_oracle as orc
    H, W, fx, fy, cx, cy = sc["intr"]
    res = m.resolution
    pts, xyz = MR.grid_uniform(m.marching_cubes_bound.numpy(), res)
    assert np.array_equal(pts, m.get_grid_uniform(res)["grid_points"].numpy())
    if use_all:
        c2ws, depths, mode = [est[i].numpy() for i in range(len(est))], [], 0
    else:
        c2ws, depths, mode = [k["est_c2w"].numpy() for k in kfs], [k["depth"].numpy() for k in kfs], (2 if m.depth_test else 1)

    def masks(p):
        return MR.point_masks(p, c2ws, depths, H, W, fx, fy, cx, cy, mode, m.points_batch_size)

    def field(p, stage):
        return m.eval_points(torch.from_numpy(p).to(DEV), dec, grids, stage, DEV)[:, 3].cpu().numpy()

    if show_forecast:
        code = masks(pts)
        got_code = m._mask_codes(torch.from_numpy(pts).to(DEV), kfs, est, len(est) - 1, DEV, use_all).cpu().numpy()
        assert np.array_equal(got_code, code)
        z = np.full(len(pts), -100.0, np.float32)
        z[code == 2] = field(pts[code == 2], "coarse") + np.float32(0.2)
        z[code == 1] = field(pts[code == 1], "fine")
    else:
        z = field(pts, "fine")
        if mesh_bound is not None:
            z[~mesh_bound(pts)] = 100.0
    vol = z.reshape(res, res, res).transpose(1, 0, 2)
    verts, faces = MR.marching_cubes(vol, m.level_set, [a[2] - a[1] for a in xyz], [a[0] for a in xyz])
    if show_forecast:
        inside = mesh_bound(verts) if mesh_bound is not None else np.ones(len(verts), bool)
        faces = faces[~(~inside)[faces].all(1)]
    else:
        unseen = masks(verts.astype(np.float32)) != 1
        faces = faces[~unseen[faces].all(1)]
    comp = MR.face_adjacency_components(faces)
    area = MR.face_areas(verts, faces)
    ca = np.array([area[comp == c].sum() for c in range(comp.max() + 1)])
    if m.get_largest_components:
        keep = comp == np.argmax(ca)        # scipy labels components in order of their first face: argmax takes the first tie
    else:
        keep = ca[comp] > m.remove_small_geometry_threshold * m.scale ** 2
    faces = faces[keep]
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    verts, faces = verts[used], remap[faces].astype(np.int32)
    ref_col = orc.eval_points(torch.from_numpy(verts.astype(np.float32)).double(), sc["grids"], sc["params"],
                              orc.decoder_bounds(sc["bound"]), sc["bound"], "color")[:, :3].numpy()
    fore = masks(verts.astype(np.float32)) == 2 if show_forecast else None
    return verts, faces, ref_col, fore


CASES = [  # show_forecast, depth_test, largest, mesh_bound, get_mask_use_all_frames
    (False, True, False, False, False),
    (False, False, True, True, False),
    (True, True, False, False, False),
    (True, False, True, True, False),
    (False, True, False, True, True),
]


@pytest.mark.parametrize("show_forecast,depth_test,largest,bounded,use_all", CASES)
def test_get_mesh_end_to_end(tmp_path, show_forecast, depth_test, largest, bounded, use_all):
    from nice_slam_amd.ply import read_mesh
    sc, m, dec, grids, kfs, est = _setup(64, depth_test, largest)
    b = m.marching_cubes_bound.numpy()
    mesh_bound = _box(b[:, 0] + 0.15 * (b[:, 1] - b[:, 0]), b[:, 1] - 0.2 * (b[:, 1] - b[:, 0])) if bounded else None
    out = str(tmp_path / "mesh.ply")
    got = m.get_mesh(out, grids, dec, kfs, est, len(est) - 1, DEV, show_forecast=show_forecast, color=True, clean_mesh=True,
                     get_mask_use_all_frames=use_all, mesh_bound=mesh_bound)
    assert got is not None
    gv, gf, gc = got
    ev, ef, ecol, fore = _expected(sc, m, dec, grids, kfs, est, show_forecast, mesh_bound, use_all)
    assert len(ef) > 50
    assert np.array_equal(gv.cpu().numpy(), ev / m.scale) and np.array_equal(gf.cpu().numpy(), ef)
    col_f = m.eval_points(gv.float() * m.scale, dec, grids, "color", DEV)[:, :3]
    assert rel_err(col_f.cpu(), ecol) < 1e-4
    want = (col_f.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()
    if show_forecast:
        assert fore.any()
        want[fore] = [0, 255, 255]
    assert np.array_equal(gc.cpu().numpy(), want)
    rv, rf, rc = read_mesh(out, colors=True)
    assert np.array_equal(rv, (ev / m.scale).astype(np.float32)) and np.array_equal(rf, ef) and np.array_equal(rc[:, :3], want)


def test_get_mesh_without_surface(tmp_path, capsys):
    sc, m, dec, grids, kfs, est = _setup(32, True, False)
    m.level_set = 1e6
    out = str(tmp_path / "none.ply")
    assert m.get_mesh(out, grids, dec, kfs, est, 1, DEV) is None
    assert not os.path.exists(out) and "no surface" in capsys.readouterr().out
    with pytest.raises(NotImplementedError):
        m.get_bound_from_frames(kfs, 1.0)


def test_get_mesh_512_smoke(tmp_path):
    """512^3 lattice end to end (the reference's 'higher resolution geometry' setting): completes, reports V and F."""
    sc, m, dec, grids, kfs, est = _setup(128, True, False)
    m.resolution = 512
    m.points_batch_size = 500000
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    got = m.get_mesh(str(tmp_path / "m512.ply"), grids, dec, kfs, est, 1, DEV, show_forecast=False, clean_mesh=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert got is not None
    v, f, c = got
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print(f"512^3 get_mesh: V={v.shape[0]} F={f.shape[0]} in {dt:.2f} s, peak {peak:.2f} GiB")
    assert f.shape[0] > 1000 and peak < 16.0
    assert int(f.max()) < v.shape[0] and int(f.min()) >= 0
