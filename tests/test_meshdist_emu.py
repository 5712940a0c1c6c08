"""CPU tests of the point-to-mesh distance (nice_slam_amd/csrc/nsr_meshdist.h) and of the estimator built on it
(nice_slam_amd.recon: MeshIndex, surface_metrics, error_mesh, ``eval -3d --surface mesh``), executed under the emulator
(tests/emu/) at small sizes.  Every case: distance and closest point bit for bit the brute force in the kernel's operation order
over ALL faces, the face its argmin, and the distance within 16 ulp of an independent formulation (tests/meshdist_reference.py).
The property checks take an engine, so tests/test_hip_meshdist.py runs them again on the GPU."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import emu_harness
import meshdist_reference as R
from nice_slam_amd import _capi, recon
from nice_slam_amd.engine import Engine
from nice_slam_amd.ply import read_mesh, write_ply

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "recon_eval.npz")


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


def check_mesh(E, q, v, f):
    """the product against (a) bit for bit and (b) within the gate; returns (index, distances, faces examined)"""
    idx = recon.MeshIndex(v, f, E)
    d, fi, x, nc = idx.query(q, with_candidates=True)
    d, fi, x = d.cpu().numpy(), fi.cpu().numpy(), x.cpu().numpy()
    assert d.dtype == np.float64 and fi.dtype == np.int64 and x.shape == (len(q), 3) and nc.dtype == torch.int32
    bd, bf, bx = R.brute(q, v, f)
    assert np.array_equal(d, bd)                                   # bit for bit, and never NaN
    assert np.array_equal(fi, bf)                                  # argmin: ties to the smallest index
    assert np.array_equal(x, bx)
    if len(q):
        q64, v64 = np.asarray(q, np.float64), np.asarray(v, np.float64)
        scale = np.maximum(np.abs(v64).max(), np.abs(q64).max(1))
        assert np.all(np.abs(d - R.independent_mesh(q64, v64, f)) <= R.gate(scale, d))
        assert np.all(d >= 0) and np.all(nc.cpu().numpy() >= 1)
    return idx, d, nc.cpu().numpy()


def one_face_queries():
    """a = (0,0,0), b = (2,0,0), c = (0,1,0): queries in all seven regions, above and in the plane, on the vertices and edges"""
    rng = np.random.default_rng(0)
    xy = np.array([[0.5, 0.25], [-1, -1], [3, -0.5], [-0.5, 2], [1, -1], [-1, 0.5], [2, 2],          # interior, a, b, c, ab, ca, bc
                   [0, 0], [2, 0], [0, 1], [1, 0], [0, 0.5], [1, 0.5], [0.3, 0.2]])
    grid = np.stack(np.meshgrid(np.linspace(-1.5, 3.5, 11), np.linspace(-1.5, 2.5, 9), indexing="ij"), -1).reshape(-1, 2)
    xy = np.concatenate([xy, grid, rng.uniform(-2, 4, (80, 2))])
    return np.concatenate([np.concatenate([xy, np.full((len(xy), 1), z)], 1) for z in (0.0, 0.7, -1.3)])


def rotated(v, seed):
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return v @ Q.T + rng.normal(size=3)


def cases():
    rng = np.random.default_rng(11)
    tri = (np.array([[0.0, 0, 0], [2, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]], np.int32))
    dv = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0.3, 0.3, 0.3], [0.3, 0.3, 0.3], [0.3, 0.3, 0.3], [0, 1, 0], [0, 2, 0], [0, 3.5, 0]], np.float64)
    df = np.arange(9, dtype=np.int32).reshape(3, 3)
    # the same three kinds along the diagonal (1, 2, -1), in dyadic coordinates: the cross products are exactly zero there too
    diag = np.array([1.0, 2.0, -1.0])
    diag_v = np.array([[0.5, 0.25, 1]] * 9) + np.array([0, 1, 1, 0.375, 0.375, 0.375, 0.25, 0.5, 0.875])[:, None] * diag
    dq = rng.uniform(-1, 4, (150, 3))
    dq[:6] = [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0.3, 0.3, 0.3], [0, 2.5, 0], [0, 5, 0]]
    cell = (0.3 + 1e-7 * rng.uniform(size=(90, 3)), np.arange(90, dtype=np.int32).reshape(30, 3))
    pv, pf = R.rectangle((-1, -1), (1, 1), 0.25, 9, 7)
    bv, bf = R.box([0, 0, 0], [1.0, 0.8, 0.6], 5)
    # duplicated faces, and a fan of 6 faces around the edge (0,0,0) - (0,0,1) with queries ON that edge
    fan_v = np.array([[0, 0, 0], [0, 0, 1]] + [[np.cos(a), np.sin(a), 0.5] for a in np.linspace(0, 2 * np.pi, 6, endpoint=False)])
    fan_f = np.array([[0, 1, 2 + k] for k in range(6)], np.int32)
    dup_f = np.concatenate([fan_f[::-1], fan_f, fan_f[2:4]])
    edge_q = np.stack([np.zeros(40), np.zeros(40), np.linspace(-0.5, 1.5, 40)], 1)
    fan_q = np.concatenate([edge_q, fan_v, rng.uniform(-1.2, 1.2, (80, 3))])
    ov, of = R.oversize_scene(seed=3)
    oq = np.concatenate([rng.uniform(-0.5, 5.5, (250, 3)), ov[::40] + 1e-4])
    far = rng.normal(size=(60, 3))
    far = 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)
    uv, uf = R.box([-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], 4)
    out = {
        "one_face": (one_face_queries(), *tri),
        "one_face_rotated": (rotated(one_face_queries(), 1), rotated(tri[0], 1), tri[1]),
        "degenerate_two_equal": (dq, dv, df[0:1]),
        "degenerate_three_equal": (dq, dv, df[1:2]),
        "degenerate_collinear": (dq, dv, df[2:3]),
        "degenerate_diagonal": (dq, diag_v, df),
        "one_cell": (np.concatenate([rng.uniform(0.2, 0.4, (80, 3)), cell[0][:20]]), *cell),
        "planar": (rng.uniform(-1.3, 1.3, (300, 3)), pv, pf),
        "planar_rotated": (rotated(rng.uniform(-1.3, 1.3, (300, 3)), 4), rotated(pv, 4), pf),
        "box": (np.concatenate([rng.uniform(0.05, 0.55, (200, 3)), rng.uniform(-0.6, 1.6, (300, 3)), bv[::5]]), bv, bf),
        "duplicates_and_fan": (fan_q, fan_v, dup_f),
        "oversize": (oq, ov, of),
        "far": (np.concatenate([far, rng.uniform(-1, 1, (40, 3))]), uv, uf),
        "zero_queries": (np.zeros((0, 3)), bv, bf),
        "fp32": (rng.uniform(-0.6, 1.6, (300, 3)).astype(np.float32), bv.astype(np.float32), bf),
        "fp32_queries_fp64_mesh": (rng.uniform(-0.6, 1.6, (100, 3)).astype(np.float32), rotated(bv, 5), bf),
    }
    # F and N on both sides of a wave (64) and of a block (256)
    for F, N in ((63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255)):
        v = rng.uniform(-1, 1, (F, 1, 3)) + rng.uniform(-0.15, 0.15, (F, 3, 3))
        out[f"sizes_F{F}_N{N}"] = (rng.uniform(-1.2, 1.2, (N, 3)), v.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3))
    # the box again, whose grid is ragged (test_grid_walk.py checks the plan): the first INSIDE queries sit at its empty middle,
    # the next len(far) far outside: these FAR_RAGGED come first, then queries around the box
    inside = np.array([0.5, 0.4, 0.3]) + rng.uniform(-0.02, 0.02, (INSIDE, 3))
    out["far_ragged"] = (np.concatenate([inside, far, rng.uniform(-0.2, 1.2, (40, 3))]), bv, bf)
    return out


INSIDE, FAR_RAGGED = 15, 75
CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_matches_brute_force(E, name):
    q, v, f = CASES[name]
    assert len(f) <= 2000 and len(q) <= 600
    idx, d, nc = check_mesh(E, q, v, f)
    if name == "oversize":
        assert idx.nover == 2 and idx.npairs <= _capi_cell_cap() * len(f)
    if name == "one_face":
        regions = R.pair_eval(np.asarray(q), v[0], v[1], v[2])[2]
        assert set(regions.tolist()) == {1, 2, 3, 4, 5, 6, 7}       # the walk's seven regions are all visited
    if name.startswith("degenerate"):
        assert (R.pair_eval(np.asarray(q)[:, None], *np.asarray(v)[f].transpose(1, 0, 2)[:, None])[2] == 0).all()


def _capi_cell_cap():
    import re
    txt = open(os.path.join(os.path.dirname(HERE), "include", "nsr.h")).read()
    return int(re.search(r"#define NSR_MESHDIST_CELL_CAP (\d+)", txt).group(1))


def test_references_agree():
    """(a) against (b) on random, tiny and far inputs, pair by pair: the measured distance between the two formulations"""
    rng = np.random.default_rng(12)
    worst = 0.0
    for size, radius in ((1.0, 2.0), (1e-3, 1.0), (1.0, 100.0)):
        tri = rng.uniform(-1, 1, (1, 600, 3, 3)) * size
        p = rng.normal(size=(500, 1, 3))
        p = radius * p / np.linalg.norm(p, axis=-1, keepdims=True) * rng.uniform(0.2, 1, (500, 1, 1))
        d2 = R.pair_eval(p, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])[0]
        di = R.independent(p, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])
        d = np.sqrt(d2)
        scale = np.maximum(np.maximum(np.abs(p).max(-1), np.abs(tri).max((-1, -2))), d)
        worst = max(worst, (np.abs(d - di) / (R.EPS * scale)).max())
    print("pair_eval against independent: worst", worst, "ulp of max(|coordinates|, distance)")
    assert worst <= 16.0


def test_rejects(E):
    v, f = R.box([0, 0, 0], [1, 1, 1])
    with pytest.raises(ValueError):
        recon.MeshIndex(v, np.zeros((0, 3), np.int32), E)
    bad = v.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        recon.MeshIndex(bad, f, E)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        recon.mesh_distance(np.zeros((2, 3)), bad, f, E)
    with pytest.raises(ValueError):
        recon.MeshIndex(v, f + len(v), E)                           # a face index outside the vertex array
    with pytest.raises(ValueError):
        recon.MeshIndex(v, f, E).query(np.array([[0.0, np.nan, 0.0]]))
    lib = E.lib
    assert lib.nsr_meshdist_plan(None, 0, None) != 0 and b"no faces" in lib.nsr_last_error()
    idx = recon.MeshIndex(v, f, E)
    assert lib.nsr_meshdist_workspace_bytes(idx.plan, len(f), 2 ** 31, 0) == -1        # int32 indexing
    assert lib.nsr_meshdist_workspace_bytes(idx.plan, len(f), _capi_cell_cap() * len(f) + 1, 0) == -1
    assert lib.nsr_meshdist_query(None, 5, 1, None, idx.plan, None, len(f), idx.npairs, 0, None, None, None, None, None) != 0
    assert lib.nsr_meshdist_query(None, 0, 1, None, idx.plan, None, len(f), idx.npairs, 0, None, None, None, None, None) == 0


def test_normals_and_stats(E):
    rng = np.random.default_rng(13)
    v = rng.normal(size=(40, 3))
    f = np.stack([rng.permutation(40)[:3] for _ in range(700)]).astype(np.int32)
    f[5] = [3, 3, 9]
    f[6] = [4, 4, 4]
    n = recon.face_normals(v, f, E).numpy()
    tri = v[f]
    ab, ac = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
    ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    with np.errstate(all="ignore"):
        ref = np.where(ln[:, None] > 0, cr / ln[:, None], 0.0)
    assert np.array_equal(n, ref) and not n[5].any() and not n[6].any()
    assert np.array_equal(recon.face_normals(v.astype(np.float32), f, E).numpy()[:5],
                          recon.face_normals(v.astype(np.float32).astype(np.float64), f, E).numpy()[:5])
    # the sum in the fixed order of nsr_dist_stats: trees of 256 inside blocks, then the blocks in order
    qn = rng.normal(size=(1000, 3))
    qn[17] = 0.0
    face = rng.integers(0, 700, 1000)
    face[:3] = [5, 6, 5]
    s, c = recon._normal_stats(E, torch.from_numpy(qn), torch.from_numpy(n), torch.from_numpy(face))
    m = n[face]
    term = np.abs((qn[:, 0] * m[:, 0] + qn[:, 1] * m[:, 1]) + qn[:, 2] * m[:, 2])
    valid = qn.any(1) & m.any(1)
    x = np.zeros(4 * 256)
    x[:1000] = np.where(valid, term, 0.0)
    blocks = x.reshape(4, 256)
    w = 128
    while w >= 1:
        blocks = blocks[:, :w] + blocks[:, w:2 * w]
        w //= 2
    acc = 0.0
    for b in blocks[:, 0]:
        acc += b
    assert s == acc and c == float(valid.sum()) and 900 < valid.sum() <= 996


# ---- properties, on the engine they are given (the GPU tests call them too) ---------------------------------------------
def prop_below_vertex_nn(E, q, v, f):
    """(i) the mesh is never farther than its nearest vertex"""
    d = recon.MeshIndex(v, f, E).query(q)[0].cpu().numpy()
    used = np.unique(np.asarray(f).reshape(-1))
    dv = cKDTree(np.asarray(v, np.float64)[used]).query(np.asarray(q, np.float64))[0]
    assert np.all(d >= 0) and np.all(d <= dv + 1e-12)
    return d


def prop_below_point_estimator(E, rec, gt, n_points):
    """(ii) for the metric's own samples the distance to the other mesh is at most the distance to the other cloud"""
    rp = recon.sample_surface(rec[0], rec[1], n_points, seed=0, engine=E)[0]
    gp = recon.sample_surface(gt[0], gt[1], n_points, seed=1, engine=E)[0]
    d_mesh = recon.MeshIndex(gt[0], gt[1], E).query(rp)[0]
    d_point = recon.nearest(rp, gp, E)[0]
    assert bool((d_mesh <= d_point + 1e-12).all())
    d_mesh = recon.MeshIndex(rec[0], rec[1], E).query(gp)[0]
    d_point = recon.nearest(gp, rp, E)[0]
    assert bool((d_mesh <= d_point + 1e-12).all())


def prop_tessellation(E, n_queries=400):
    """(iii) a rectangle as 2 triangles and as a 32 x 32 grid"""
    rng = np.random.default_rng(14)
    Q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    q = rng.uniform(-1.5, 1.5, (n_queries, 3)) @ Q.T
    v2, f2 = R.rectangle((-1, -0.7), (1, 0.7), 0.1, 1, 1)
    vg, fg = R.rectangle((-1, -0.7), (1, 0.7), 0.1, 32, 32)
    d2 = recon.mesh_distance(q, v2 @ Q.T, f2, E)[0].cpu().numpy()
    dg = recon.mesh_distance(q, vg @ Q.T, fg, E)[0].cpu().numpy()
    scale = np.maximum(np.abs(q).max(1), np.abs(v2).max())
    assert np.all(np.abs(d2 - dg) <= R.gate(scale, d2))


def prop_self(E, mesh, n_points):
    """(iv) a mesh scored against itself: the mesh estimator reads zero where the point estimator reads its sampling floor"""
    m = recon.calc_3d_metric(mesh, mesh, n_points=n_points, seed=2, engine=E, surface="mesh", thresholds=(0.05, 0.01))
    assert m["accuracy_cm"] < 1e-10 and m["completion_cm"] < 1e-10 and m["chamfer_cm"] < 1e-10      # 1e-12 m
    assert m["completion_ratio_pct"] == 100.0
    for t in (0.05, 0.01):
        assert m["precision_pct"][t] == 100.0 and m["recall_pct"][t] == 100.0 and m["fscore_pct"][t] == 100.0
    assert m["normal_consistency"] >= 1 - 1e-12 and m["normal_pairs"] == 2 * n_points
    p = recon.calc_3d_metric(mesh, mesh, n_points=n_points, seed=2, engine=E, surface="points")
    assert p["accuracy_cm"] > 0.1 and p["completion_cm"] > 0.1      # above 1 mm: the floor of the point estimator
    return m, p


def plane_and_patch(z=0.0, theta=0.0, flip=False):
    gt = R.rectangle((-2, -2), (2, 2), 0.0, 1, 1)
    pv, pf = R.rectangle((-0.5, -0.5), (0.5, 0.5), 0.0, 3, 3)
    pv = pv @ R.rotation_x(theta).T + [0, 0, z]
    return (pv, pf[:, ::-1].copy() if flip else pf), gt


def prop_shift(E, n_points):
    """(v) a patch 0.01 above a larger plane, exactly"""
    rec, gt = plane_and_patch(z=0.01)
    m = recon.surface_metrics(rec, gt, align=False, n_points=n_points, engine=E)
    assert abs(m["accuracy_cm"] - 1.0) <= 1e-12
    assert m["precision_pct"][0.05] == 100.0 and m["normal_consistency"] >= 1 - 1e-12
    m2 = recon.surface_metrics(rec, gt, align=False, n_points=n_points, thresholds=(0.005,), engine=E)
    assert m2["precision_pct"][0.005] == 0.0 and m2["fscore_pct"][0.005] == 0.0 and m2["recall_pct"][0.005] == 0.0


def prop_tilt(E, n_points, theta=0.3):
    """(vi) a patch tilted by theta about a line through its middle: |n . m| = cos(theta) in both directions, whatever the winding"""
    for flip in (False, True):
        rec, gt = plane_and_patch(theta=theta, flip=flip)
        m = recon.surface_metrics(rec, gt, align=False, n_points=n_points, engine=E)
        assert abs(m["normal_consistency"] - np.cos(theta)) <= 1e-12, flip
        assert m["normal_pairs"] == 2 * n_points


def prop_degenerate_pairs(E, n_points):
    """(vii) the pairs that hold a degenerate face are exactly the ones missing from normal_pairs"""
    rec, (gv, gf) = plane_and_patch(z=0.01)
    gv = np.concatenate([gv, [[-0.2, 0, 0.005], [0.2, 0, 0.005]]])
    gf = np.concatenate([gf, [[len(gv) - 2, len(gv) - 1, len(gv) - 1]]]).astype(np.int32)
    m = recon.surface_metrics(rec, (gv, gf), align=False, n_points=n_points, engine=E)
    rp = recon.sample_surface(rec[0], rec[1], n_points, seed=0, engine=E)[0].cpu().numpy()
    on_segment = int((R.brute(rp, gv, gf)[1] == len(gf) - 1).sum())
    assert on_segment > 0
    assert m["normal_pairs"] == 2 * n_points - on_segment
    assert m["normal_consistency"] >= 1 - 1e-12                    # the pairs that remain are plane against plane


def test_property_vertex_nn(E):
    rng = np.random.default_rng(15)
    v, f = R.box([0, 0, 0], [1, 0.8, 0.6], 5)
    prop_below_vertex_nn(E, rng.uniform(-0.5, 1.5, (500, 3)), v, f)


def test_property_point_estimator(E):
    prop_below_point_estimator(E, R.box([0.01, 0, 0], [1, 0.8, 0.6], 3), R.box([0, 0, 0], [1, 0.8, 0.6], 4), 1500)


def test_property_tessellation(E):
    prop_tessellation(E)


def test_property_self(E):
    prop_self(E, R.box([0, 0, 0], [1, 1, 1], 3), 2000)


def test_property_shift_tilt_degenerate(E):
    prop_shift(E, 2000)
    prop_tilt(E, 2000)
    prop_degenerate_pairs(E, 2000)


def test_default_metric_unchanged(E):
    """(viii) calc_3d_metric with defaults: today's dict from today's code path, and the golden clouds score as minted"""
    gold = np.load(GOLDEN)
    for name in gold["cloud_names"]:
        acc, comp, ratio = recon.recon_metrics(gold[f"{name}/gt"], gold[f"{name}/rec"], engine=E)
        assert acc == pytest.approx(float(gold[f"{name}/accuracy"]), rel=1e-12, abs=0)
        assert comp == pytest.approx(float(gold[f"{name}/completion"]), rel=1e-12, abs=0)
        assert ratio == float(gold[f"{name}/completion_ratio_0.05"])
    rec, gt = R.box([0.01, 0, 0], [1, 0.8, 0.6], 3), R.box([0, 0, 0], [1, 0.8, 0.6], 4)
    m = recon.calc_3d_metric(rec, gt, align=False, n_points=1500, seed=4, engine=E)
    assert list(m) == ["accuracy_cm", "completion_cm", "completion_ratio_pct"]
    rp = recon.sample_surface(rec[0], rec[1], 1500, seed=4, engine=E)[0]
    gp = recon.sample_surface(gt[0], gt[1], 1500, seed=5, engine=E)[0]
    acc, comp, ratio = recon.recon_metrics(gp, rp, 0.05, E)
    assert (m["accuracy_cm"], m["completion_cm"], m["completion_ratio_pct"]) == (acc * 100, comp * 100, ratio * 100)
    assert m == recon.calc_3d_metric(rec, gt, align=False, n_points=1500, seed=4, engine=E, surface="points")
    with pytest.raises(ValueError):
        recon.calc_3d_metric(rec, gt, engine=E, surface="voxels")


def run_cli(E, monkeypatch, capsys, argv):
    monkeypatch.setattr(recon, "gpu", lambda: E)
    assert recon.main(argv) == 0
    return capsys.readouterr().out.strip().splitlines()


def test_cli(E, monkeypatch, capsys, tmp_path):
    """(ix) without --surface the three lines of today; with it the extra lines and the coloured mesh"""
    v, f = R.box([0, 0, 0], [1, 0.8, 0.6], 3)
    a, b, out = str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply"), str(tmp_path / "err.ply")
    write_ply(a, v, f)
    write_ply(b, v, f)
    lines = run_cli(E, monkeypatch, capsys, ["eval", "--rec_mesh", a, "--gt_mesh", b, "-3d", "--n_points", "1500"])
    m = recon.calc_3d_metric(a, b, n_points=1500, engine=E)
    assert lines == [f"accuracy:  {m['accuracy_cm']}", f"completion:  {m['completion_cm']}", f"completion ratio:  {m['completion_ratio_pct']}"]
    lines = run_cli(E, monkeypatch, capsys, ["eval", "--rec_mesh", a, "--gt_mesh", b, "-3d", "--n_points", "1500", "--surface", "mesh", "--thresholds", "0.05", "0.01",
                                             "--error_mesh", out])
    heads = [ln.split(":")[0] for ln in lines]
    assert heads == ["accuracy", "completion", "completion ratio", "chamfer", "precision@0.05", "recall@0.05", "f-score@0.05",
                     "precision@0.01", "recall@0.01", "f-score@0.01", "normal consistency", "normal pairs", "error mesh"]
    assert float(lines[6].split()[-1]) == 100.0 and float(lines[0].split()[-1]) < 1e-10
    assert len(read_mesh(out, colors=True)[2]) == len(v)
    with pytest.raises(SystemExit):
        recon.main(["eval", "--rec_mesh", a, "--gt_mesh", b, "-3d", "--error_mesh", out])


def check_error_mesh(E, tmp_path):
    """vertices on the ground truth carry the first plasma entry, vertices at or beyond vmax the last"""
    gt = R.rectangle((-2, -2), (2, 2), 0.0, 1, 1)
    pv, pf = R.rectangle((-0.5, -0.5), (0.5, 0.5), 0.0, 4, 4)
    pv[:, 2] = np.where(pv[:, 0] > 0.2, 0.06, np.where(pv[:, 0] < -0.2, 0.0, 0.02))
    path = str(tmp_path / "error.ply")
    d = recon.error_mesh((pv, pf), gt, path, vmax=0.05, engine=E).cpu().numpy()
    assert np.array_equal(d, np.abs(pv[:, 2]))
    v, f, rgba = read_mesh(path, colors=True)
    assert np.array_equal(f, pf) and np.array_equal(v, pv.astype(np.float32).astype(np.float64))
    assert (rgba[d == 0.0, :3] == [12, 7, 134]).all() and (d == 0.0).sum() == 10
    assert (rgba[d >= 0.05, :3] == [239, 248, 33]).all() and (d >= 0.05).sum() == 10
    mid = rgba[(d > 0) & (d < 0.05), :3]
    assert len(mid) == 5 and not (mid == [12, 7, 134]).all(1).any() and not (mid == [239, 248, 33]).all(1).any()
    assert np.array_equal(recon.error_mesh((pv, pf), gt, engine=E).cpu().numpy(), d)       # without a path: distances only


def test_error_mesh(E, tmp_path):
    check_error_mesh(E, tmp_path)


def test_kernels_use_no_scratch():
    """the build's record of what the compiler made of the new kernels (nice_slam_amd/libnsr.resources.json)"""
    import json
    from nice_slam_amd import build
    res = json.load(open(build.RESOURCES))
    md = {k: v for k, v in res.items() if "md_" in k and "MdParams" in k or "MdNormalParams" in k}
    assert len(md) == 6
    # the kernels it shares with the point search (nsr_recon.h): the clear of the run tables, the normal statistic's reduction
    shared = {k: v for k, v in res.items() if "nn_clear_kernel" in k and "NnGrid" in k or "reduce_kernel" in k and "ILi3E" in k}
    assert len(shared) == 2
    md.update(shared)
    for k, v in md.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
