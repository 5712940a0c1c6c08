"""GPU tests of the point-to-mesh distance (nice_slam_amd.recon.MeshIndex on libnsr.so) and of the estimator built on it: the
room of tests/recon_scenes.py meshed at 64^3 against 100 000 queries (surface samples with noise, uniform points of the box,
500 far points) -- bit for bit the kernel's expression at the returned face, a brute force over ALL faces on a subset, the
vertex bound, run-to-run identity and pruning -- then the oversize and degenerate cases and the estimator's properties of
tests/test_meshdist_emu.py on the device at 20 000 samples, and the error-coloured mesh."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import mesh_reference as MR
import meshdist_reference as R
import recon_scenes as RS
import test_meshdist_emu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_POINTS = 20000


@pytest.fixture(scope="module")
def E():
    from nice_slam_amd.engine import on
    return on(DEV)


@pytest.fixture(scope="module")
def room(E):
    """the mesh, the queries (and how many of them are surface samples), and the product's answer, computed once"""
    from nice_slam_amd import recon
    f, sp, org = RS.room_lattice(64)
    v, fc = MR.marching_cubes(f, 0.0, sp, org)
    rng = np.random.default_rng(21)
    n_surf = 60000
    surf = RS.room_surface_points(n_surf, 22) + rng.normal(scale=0.005, size=(n_surf, 3))
    uni = rng.uniform(RS.ROOM_LO - RS.MARGIN, RS.ROOM_HI + RS.MARGIN, (100000 - n_surf - 500, 3))
    far = rng.normal(size=(500, 3))
    far = (RS.ROOM_LO + RS.ROOM_HI) / 2 + 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)
    q = np.concatenate([surf, uni, far])
    idx = recon.MeshIndex(torch.from_numpy(v).to(DEV), torch.from_numpy(fc).to(DEV), E)
    out = idx.query(torch.from_numpy(q).to(DEV), with_candidates=True)
    torch.cuda.synchronize()
    return {"v": v, "f": fc, "q": q, "n_surf": n_surf, "idx": idx, "out": out}


def test_room_exact_at_returned_face(room):
    d, fi, x, _ = (t.cpu().numpy() for t in room["out"])
    assert len(room["q"]) == 100000 and fi.min() >= 0 and fi.max() < len(room["f"])
    rd, rx = R.at_face(room["q"], room["v"], room["f"], fi)
    assert np.array_equal(d, rd) and np.array_equal(x, rx)         # N evaluations of (a), bit for bit


def test_room_brute_force_subset(room):
    d, fi, x, _ = (t.cpu().numpy() for t in room["out"])
    rng = np.random.default_rng(23)
    n = len(room["q"])
    pick = np.concatenate([rng.choice(n - 500, 460, replace=False), n - 500 + rng.choice(500, 40, replace=False)])
    bd, bf, bx, d2 = R.brute(room["q"][pick], room["v"], room["f"], chunk=32, return_d2=True)
    assert np.array_equal(d[pick], bd)                              # the minimum over ALL faces
    differ = fi[pick] != bf
    k = np.nonzero(differ)[0]
    assert np.all(d2[k, fi[pick][k]] == d2[k, bf[k]]) and np.all(fi[pick][k] < bf[k])     # only at an exact tie, to the smaller index
    assert np.array_equal(x[pick][~differ], bx[~differ])


def test_room_vertex_bound_and_pruning(room):
    d, fi, x, nc = (t.cpu().numpy() for t in room["out"])
    used = np.unique(room["f"].reshape(-1))
    dv = cKDTree(room["v"][used]).query(room["q"])[0]
    assert np.all(d >= 0) and np.all(d <= dv + 1e-12)               # (i)
    F = len(room["f"])
    mean_surface = nc[:room["n_surf"]].astype(np.float64).mean()
    print(f"faces examined per surface query: mean {mean_surface:.1f}, max {nc[:room['n_surf']].max()} of {F}; all queries: "
          f"mean {nc.astype(np.float64).mean():.1f}, max {nc.max()}")
    assert mean_surface < F / 10                                    # only a search that does not prune breaks this


def test_room_deterministic(room):
    again = room["idx"].query(torch.from_numpy(room["q"]).to(DEV), with_candidates=True)
    for a, b in zip(room["out"], again):
        assert torch.equal(a, b)
    from nice_slam_amd import recon
    rebuilt = recon.MeshIndex(torch.from_numpy(room["v"]).to(DEV), torch.from_numpy(room["f"]).to(DEV))
    assert (rebuilt.npairs, rebuilt.nover) == (room["idx"].npairs, room["idx"].nover)
    for a, b in zip(room["out"], rebuilt.query(torch.from_numpy(room["q"]).to(DEV), with_candidates=True)):
        assert torch.equal(a, b)                                    # a second build gives the same table


@pytest.mark.parametrize("name", ["oversize", "degenerate_two_equal", "degenerate_three_equal", "degenerate_collinear",
                                  "degenerate_diagonal", "duplicates_and_fan", "far", "fp32", "zero_queries"])
def test_cases_on_device(E, name):
    q, v, f = T.CASES[name]
    idx, d, nc = T.check_mesh(E, q, v, f)
    if name == "oversize":
        assert idx.nover == 2


def test_rejects_on_device(E):
    from nice_slam_amd import recon
    v, f = R.box([0, 0, 0], [1, 1, 1])
    bad = v.copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError):
        recon.MeshIndex(torch.from_numpy(bad).to(DEV), f)
    with pytest.raises(ValueError):
        recon.MeshIndex(v, np.zeros((0, 3), np.int32))
    with pytest.raises(ValueError):
        recon.MeshIndex(v, f).query(torch.tensor([[0.0, float("inf"), 0.0]], device=DEV))


def test_properties_on_device(E, room):
    T.prop_tessellation(E, 2000)
    T.prop_below_point_estimator(E, R.box([0.01, 0, 0], [1, 0.8, 0.6], 3), R.box([0, 0, 0], [1, 0.8, 0.6], 4), N_POINTS)
    mesh = (torch.from_numpy(room["v"]).to(DEV), torch.from_numpy(room["f"]).to(DEV))
    m, p = T.prop_self(E, mesh, N_POINTS)                           # (iv)
    print("room against itself at", N_POINTS, "samples: mesh estimator", m["accuracy_cm"], "cm, point estimator", p["accuracy_cm"], "cm")
    T.prop_shift(E, N_POINTS)                                       # (v)
    T.prop_tilt(E, N_POINTS)                                        # (vi)
    T.prop_degenerate_pairs(E, N_POINTS)                            # (vii)


def test_default_metric_and_cli(E, monkeypatch, capsys, tmp_path):
    T.test_default_metric_unchanged(E)                              # (viii)
    T.test_cli(E, monkeypatch, capsys, tmp_path)                    # (ix)


def test_error_mesh(E, tmp_path):
    T.check_error_mesh(E, tmp_path)
