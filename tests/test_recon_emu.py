"""CPU tests of the reconstruction-evaluation kernels (nice_slam_amd/csrc/nsr_recon.h) and of nice_slam_amd.recon, executed
under the emulator (tests/emu/) at small sizes: nearest neighbour against a numpy brute force and scipy's cKDTree, the
surface sampler against a numpy restatement, the metrics and the frustum cull against a golden minted from the reference's
eval_recon.py / cull_mesh.py (tests/golden/make_golden_recon.py), the PLY reader, and the C ABI's error paths."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import emu_harness
from nice_slam_amd import _capi, recon
from nice_slam_amd.engine import Engine, w2c_rows
from nice_slam_amd.ply import write_ply

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "recon_eval.npz")


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def brute(q, ref):
    """distances in the kernel's operation order, and the first (smallest) index of the minimum"""
    q = np.asarray(q, np.float64)
    ref = np.asarray(ref, np.float64)
    d = q[:, None, :] - ref[None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    i = d2.argmin(1)
    return np.sqrt(d2[np.arange(len(q)), i]), i, d2


def check_nn(E, q, ref):
    d, i, nc = recon.NNIndex(ref, E).query(q, with_candidates=True)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    bd, bi, d2 = brute(q, ref)
    assert np.array_equal(d, bd)                                   # bit for bit
    unique = (d2 == d2[np.arange(len(q)), bi][:, None]).sum(1) == 1
    assert np.array_equal(i[unique], bi[unique])
    assert np.array_equal(i, bi)                                   # ties: the smallest index, like argmin
    if len(q):
        kd = cKDTree(np.asarray(ref, np.float64)).query(np.asarray(q, np.float64))[0]
        assert np.all(np.abs(d - kd) <= np.spacing(np.maximum(d, kd)))
    return nc.cpu().numpy()


def cases():
    rng = np.random.default_rng(5)
    line = np.stack([np.linspace(-1, 2, 700), np.full(700, 0.5), np.zeros(700)], 1)
    plane = np.concatenate([rng.uniform(-1, 1, (900, 2)), np.full((900, 1), 0.25)], 1)
    far = rng.normal(size=(25, 3))
    far = 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)
    one_cell = 0.3 + 1e-7 * rng.uniform(size=(200, 3))
    dup = np.repeat(rng.uniform(size=(60, 3)), 4, 0)
    out = {
        "one_point": (rng.normal(size=(50, 3)), np.array([[0.1, -0.2, 0.3]])),
        "zero_queries": (np.zeros((0, 3)), rng.uniform(size=(100, 3))),
        "one_cell": (np.concatenate([rng.uniform(0.2, 0.4, (80, 3)), one_cell[:20]]), one_cell),
        "duplicates": (np.concatenate([rng.uniform(size=(100, 3)), dup[::7]]), dup),
        "far": (np.concatenate([rng.uniform(-1, 1, (100, 3)), far]), rng.uniform(-1, 1, (2000, 3))),
        "line": (rng.uniform(-1.5, 2.5, (150, 3)), line),
        "plane": (rng.uniform(-1.2, 1.2, (150, 3)), plane),
        "uniform_fp32": (rng.uniform(-1, 1, (300, 3)).astype(np.float32), rng.uniform(-1, 1, (3000, 3)).astype(np.float32)),
    }
    # M and N on both sides of a wave (64) and of a block (256)
    for M, N in ((63, 65), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255)):
        out[f"sizes_M{M}_N{N}"] = (rng.uniform(-1.2, 1.2, (N, 3)), rng.uniform(-1, 1, (M, 3)))
    # points on the six sides of a box whose grid is ragged (test_grid_walk.py checks the plan); the first INSIDE queries sit
    # at its empty middle, the next len(far) far outside: these FAR_RAGGED come first, then queries around the box
    shell = rng.uniform(0, 1, (1500, 3))
    shell[np.arange(1500), rng.integers(0, 3, 1500)] = rng.integers(0, 2, 1500)
    inside = 0.5 + rng.uniform(-0.04, 0.04, (INSIDE, 3))
    out["far_ragged"] = (np.concatenate([inside, far, rng.uniform(-0.1, 1.1, (100, 3))]) * [1.0, 0.7, 0.45], shell * [1.0, 0.7, 0.45])
    return out


INSIDE, FAR_RAGGED = 15, 40


@pytest.mark.parametrize("name", list(cases()))
def test_nearest_matches_brute_force(E, name):
    q, ref = cases()[name]
    check_nn(E, q, ref)


def test_nearest_prunes(E, gold):
    gt, rec = gold["room/gt"], gold["room/rec"]
    nc = check_nn(E, rec, gt)
    assert nc.mean() < 0.1 * len(gt)                               # a brute force would examine every point


def test_nearest_rejects(E):
    with pytest.raises(ValueError):
        recon.nearest(np.zeros((3, 3)), np.zeros((0, 3)), engine=E)
    with pytest.raises(ValueError):
        recon.nearest(np.full((2, 3), np.nan), np.zeros((4, 3)), engine=E)
    with pytest.raises(_capi.NsrError):
        recon.nearest(np.zeros((2, 3)), np.array([[0.0, np.inf, 0.0], [1.0, 1.0, 1.0]]), engine=E)


# ---- the sampler -----------------------------------------------------------------------------------------------------
def sample_restated(verts, faces, u):
    """numpy restatement of nsr_sample_surface (trimesh's algorithm with this project's fixed-order scan)"""
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)]
    a, b = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cr = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    area = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2]) / 2.0
    T = 256
    nt = -(-len(area) // T)
    pad = np.zeros(nt * T)
    pad[:len(area)] = area
    local = np.cumsum(pad.reshape(nt, T), axis=1)                  # sequential inside a tile
    tot = local[:, -1]
    pre = np.zeros(nt)
    for t in range(1, nt):
        pre[t] = pre[t - 1] + tot[t - 1]
    cum = (pre[:, None] + local).reshape(-1)[:len(area)]
    fi = np.minimum(np.searchsorted(cum, u[:, 0] * cum[-1], side="left"), len(area) - 1)
    ab = u[:, 1:].copy()
    fold = ab.sum(1) > 1.0
    ab[fold] = np.abs(ab[fold] - 1.0)
    t = tri[fi]
    pts = ((t[:, 1] - t[:, 0]) * ab[:, :1] + (t[:, 2] - t[:, 0]) * ab[:, 1:]) + t[:, 0]
    return pts, fi


def small_mesh(rng, nv=300, nf=700):
    v = rng.normal(size=(nv, 3))
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    return v, f


def test_sampler_matches_restatement(E):
    rng = np.random.default_rng(1)
    v, f = small_mesh(rng)
    u = rng.uniform(size=(2000, 3))
    u[:5, 0] = [0.0, 1.0 - 2 ** -53, 0.5, 1e-300, 0.999]
    pts, fi = recon.sample_surface(v, f, 2000, uniforms=u, engine=E)
    rp, rfi = sample_restated(v, f, u)
    assert np.array_equal(fi.numpy(), rfi)
    assert np.array_equal(pts.numpy(), rp)


def test_sampler_philox_on_faces(E):
    rng = np.random.default_rng(2)
    v, f = small_mesh(rng, 50, 40)
    p1, fi1 = recon.sample_surface(v, f, 3000, seed=7, engine=E)
    p2, fi2 = recon.sample_surface(v, f, 3000, seed=7, engine=E)
    p3, _ = recon.sample_surface(v, f, 3000, seed=8, engine=E)
    assert np.array_equal(p1.numpy(), p2.numpy()) and np.array_equal(fi1.numpy(), fi2.numpy())
    assert not np.array_equal(p1.numpy(), p3.numpy())
    tri = v[f[fi1.numpy()]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    off = np.abs(((p1.numpy() - tri[:, 0]) * n).sum(1)) / np.linalg.norm(n, axis=1)
    assert off.max() < 1e-12 * (1 + np.abs(v).max())              # on the face's plane


# ---- metrics and ICP ------------------------------------------------------------------------------------------------
def test_metrics_match_golden(E, gold):
    for name in gold["cloud_names"]:
        gt, rec = gold[f"{name}/gt"], gold[f"{name}/rec"]
        acc = recon.accuracy(gt, rec, engine=E)
        comp = recon.completion(gt, rec, engine=E)
        assert acc == pytest.approx(float(gold[f"{name}/accuracy"]), rel=1e-12, abs=0), name
        assert comp == pytest.approx(float(gold[f"{name}/completion"]), rel=1e-12, abs=0), name
        for th in (0.05, 0.02):
            assert recon.completion_ratio(gt, rec, dist_th=th, engine=E) == float(gold[f"{name}/completion_ratio_{th}"]), name
        a2, c2, r2 = recon.recon_metrics(gt, rec, engine=E)
        assert (a2, c2, r2) == (acc, comp, float(gold[f"{name}/completion_ratio_0.05"]))


def test_dist_stats_fixed_order(E):
    rng = np.random.default_rng(3)
    d = torch.from_numpy(rng.uniform(size=1000) * 0.1)
    s, c = recon._dist_stats(E, d, 0.05)
    # the kernel's order: trees of 256 inside blocks (pairs at stride 128, 64, ...), then the blocks in order
    x = np.zeros(4 * 256)
    x[:1000] = d.numpy()
    blocks = x.reshape(4, 256)
    w = 128
    while w >= 1:
        blocks = blocks[:, :w] + blocks[:, w:2 * w]
        w //= 2
    ref = 0.0
    for b in blocks[:, 0]:
        ref += b
    assert s == ref
    assert c == float((d.numpy() < 0.05).sum())


def rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def icp_restated(src, tgt, threshold=0.1, max_iteration=30, rf=1e-6, rr=1e-6):
    """numpy + cKDTree restatement of Open3D's registration_icp (point to point) loop"""
    tree = cKDTree(tgt)
    pcd = src.copy()
    T = np.eye(4)

    def evaluate(p):
        d, i = tree.query(p)
        m = d < threshold
        if not m.any():
            return m, i, 0.0, 0.0
        return m, i, m.sum() / len(p), np.sqrt((d[m] ** 2).sum() / m.sum())

    m, i, fit, rmse = evaluate(pcd)
    it = 0
    while it < max_iteration:
        it += 1
        s, t = pcd[m], tgt[i[m]]
        ms, mt = s.mean(0), t.mean(0)
        U, _, Vt = np.linalg.svd((t - mt).T @ (s - ms) / len(s))
        S = np.eye(3)
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            S[2, 2] = -1
        R = U @ S @ Vt
        upd = np.eye(4)
        upd[:3, :3], upd[:3, 3] = R, mt - R @ ms
        T = upd @ T
        pcd = pcd @ R.T + upd[:3, 3]
        pf, pr = fit, rmse
        m, i, fit, rmse = evaluate(pcd)
        if abs(pf - fit) < rf and abs(pr - rmse) < rr:
            break
    return T, fit, rmse, it


def test_icp_recovers_motion(E, gold):
    tgt = gold["room/gt"]
    M = np.eye(4)
    M[:3, :3] = rot([0.3, 0.5, 1.0], 2.0)
    M[:3, 3] = [0.02, -0.015, 0.01]
    src = tgt @ np.linalg.inv(M)[:3, :3].T + np.linalg.inv(M)[:3, 3]
    T, fit, rmse, it = recon._icp(E, src, tgt)
    rT, rfit, rrmse, rit = icp_restated(src, tgt)
    assert it == rit
    assert np.abs(T - rT).max() < 1e-9
    assert fit == pytest.approx(rfit, abs=1e-12) and rmse == pytest.approx(rrmse, rel=1e-9, abs=1e-12)


def test_calc_3d_metric_identical_meshes(E):
    rng = np.random.default_rng(6)
    v, f = small_mesh(rng, 80, 150)
    T, fit, rmse = recon.align_icp(v, v, engine=E)
    assert np.abs(T - np.eye(4)).max() < 1e-12 and fit == 1.0 and rmse < 1e-12
    m = recon.calc_3d_metric((v, f), (v, f), align=True, n_points=3000, seed=3, engine=E)
    m0 = recon.calc_3d_metric((v, f), (v, f), align=False, n_points=3000, seed=3, engine=E)
    m1 = recon.calc_3d_metric((v, f), (v, f), align=False, n_points=3000, seed=3, engine=E)
    assert m0 == m1                                                 # seeded: reproducible
    for k in m:
        assert m[k] == pytest.approx(m0[k], rel=1e-9)
    assert set(m) == {"accuracy_cm", "completion_cm", "completion_ratio_pct"}


# ---- culling --------------------------------------------------------------------------------------------------------
def project64(verts, w2c, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5):
    """fp64 (u, v, z) of every vertex under every pose: to measure how close a vertex is to a mask boundary"""
    p = np.asarray(verts, np.float32).astype(np.float64)
    out = []
    for w in w2c.astype(np.float64).reshape(-1, 3, 4):
        cam = p @ w[:, :3].T + w[:, 3]
        X, Y, Z = -cam[:, 0], cam[:, 1], cam[:, 2]
        z = Z + 1e-5
        out.append(((fx * X + cx * Z) / z, (fy * Y + cy * Z) / z, z))
    return out


def write_traj(path, traj):
    with open(path, "w") as f:
        for row in traj:
            f.write(" ".join("%.17g" % x for x in row) + "\n")


def test_cull_matches_golden(E, gold, tmp_path):
    tp = str(tmp_path / "traj.txt")
    write_traj(tp, gold["cull/traj"])
    poses = recon.load_poses(tp)
    assert len(poses) == 20 and poses[0].dtype == torch.float32
    v, f = gold["cull/vertices"], gold["cull/faces"]
    seen, keep = recon.cull_masks(v, f, poses, engine=E)
    seen, keep = seen.numpy(), keep.numpy()
    # vertices within 1e-4 px (fp64) of a mask boundary are the only allowed exceptions: the fixture has none
    near = np.zeros(len(v), bool)
    for u, vv, z in project64(v, w2c_rows(poses, np.float32)):
        near |= (np.minimum.reduce([np.abs(u), np.abs(u - 1200), np.abs(vv), np.abs(vv - 680)]) < 1e-4) & (z <= 0)
    assert near.sum() == 0
    assert np.array_equal(seen, gold["cull/vertex_seen"])
    assert np.array_equal(keep, gold["cull/face_keep"])
    assert 0 < seen.sum() < len(v)
    vv, ff = recon.cull_mesh(v, f, poses, engine=E)
    assert vv.shape == v.shape and np.array_equal(ff.numpy(), f[gold["cull/face_keep"]])
    cv, cf = recon.cull_mesh(v, f, poses, compact=True, engine=E)
    assert np.array_equal(cv.numpy()[cf.numpy()], v[f[gold["cull/face_keep"]]])


def test_cull_many_poses_chunks(E, gold, tmp_path):
    # more poses than one LDS chunk (1024): the golden's 20 poses repeated give the golden's answer
    tp = str(tmp_path / "t.txt")
    write_traj(tp, np.concatenate([gold["cull/traj"]] * 60))
    poses = recon.load_poses(tp)
    assert len(poses) == 1200
    seen, keep = recon.cull_masks(gold["cull/vertices"][:300], gold["cull/faces"][:0], poses, engine=E)
    assert np.array_equal(seen.numpy(), gold["cull/vertex_seen"][:300]) and keep.shape == (0,)


# ---- PLY ------------------------------------------------------------------------------------------------------------
def test_read_mesh_roundtrip(tmp_path):
    rng = np.random.default_rng(7)
    v = rng.normal(size=(30, 3)).astype(np.float32)
    f = rng.integers(0, 30, (20, 3)).astype(np.int32)
    p = str(tmp_path / "a.ply")
    write_ply(p, v, f, colors=rng.integers(0, 255, (30, 3)))
    rv, rf = recon.read_mesh(p)
    assert rv.dtype == np.float64 and np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, f)
    write_ply(p, v, f)
    rv, rf = recon.read_mesh(p)
    assert np.array_equal(rv, v.astype(np.float64)) and np.array_equal(rf, f)


def test_read_mesh_ascii_and_extra_properties(tmp_path):
    p = tmp_path / "b.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment hand written\nelement vertex 4\nproperty float nx\nproperty double x\n"
                 "property double y\nproperty double z\nproperty uchar red\nproperty uchar alpha\n"
                 "element face 2\nproperty list uchar uint vertex_indices\nend_header\n"
                 "0 0.5 1 2 3 4\n0 1.25 0 0 3 4\n0 0 -2 0 3 4\n1 0 0 7.5 0 0\n3 0 1 2\n3 1 2 3\n")
    v, f = recon.read_mesh(str(p))
    assert np.array_equal(v, [[0.5, 1, 2], [1.25, 0, 0], [0, -2, 0], [0, 0, 7.5]]) and np.array_equal(f, [[0, 1, 2], [1, 2, 3]])
    # binary with normals + int-counted lists
    vb = np.zeros(3, dtype=[("x", "<f4"), ("nx", "<f4"), ("y", "<f4"), ("z", "<f4"), ("s", "<f8")])
    vb["x"], vb["y"], vb["z"] = [1, 2, 3], [4, 5, 6], [7, 8, 9]
    fb = np.zeros(1, dtype=[("n", "<i4"), ("i", "<u4", 3)])
    fb["n"], fb["i"] = 3, [2, 0, 1]
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float nx\nproperty float y\n"
           "property float z\nproperty double s\nelement face 1\nproperty list int uint vertex_indices\nend_header\n")
    q = tmp_path / "c.ply"
    q.write_bytes(hdr.encode() + vb.tobytes() + fb.tobytes())
    v, f = recon.read_mesh(str(q))
    assert np.array_equal(v, [[1, 4, 7], [2, 5, 8], [3, 6, 9]]) and np.array_equal(f, [[2, 0, 1]])


def test_read_mesh_rejects_quads(tmp_path):
    p = tmp_path / "q.ply"
    p.write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="4 vertices"):
        recon.read_mesh(str(p))


# ---- the C ABI's error paths ----------------------------------------------------------------------------------------
def test_abi_errors(E):
    lib = E.lib
    plan = (C.c_double * 16)()
    b = (C.c_double * 6)(0, 0, 0, 1, 1, 1)
    assert lib.nsr_nn_plan(b, 0, plan) != 0 and b"reference set" in lib.nsr_last_error()
    assert lib.nsr_nn_plan(b, 2 ** 31, plan) != 0
    bad = (C.c_double * 6)(0, float("nan"), 0, 1, 1, 1)
    assert lib.nsr_nn_plan(bad, 10, plan) != 0 and b"non-finite" in lib.nsr_last_error()
    assert lib.nsr_nn_plan(b, 1000, plan) == 0
    assert 0 < plan[13] <= 4 * 1000 + 64                            # cells: O(n_ref)
    assert lib.nsr_nn_workspace_bytes(plan, 1000) > 0
    assert lib.nsr_nn_workspace_bytes(plan, 10) == -1               # a plan for 1000 points is too big for 10
    broken = (C.c_double * 16)(*plan)
    broken[7] = 3.5
    assert lib.nsr_nn_workspace_bytes(broken, 1000) == -1
    assert lib.nsr_nn_bounds(None, 0, 1, None, None) != 0
    assert lib.nsr_nn_query(None, 5, 1, None, plan, None, 1000, None, None, None, None) != 0
    assert lib.nsr_nn_query(None, 0, 1, None, plan, None, 1000, None, None, None, None) == 0
    assert lib.nsr_sample_surface(None, 3, None, 0, 5, None, 0, None, None, None, None) != 0 and b"no faces" in lib.nsr_last_error()
    assert lib.nsr_sample_workspace_bytes(-1) == -1 and lib.nsr_recon_partial_doubles(-1) == -1
    assert lib.nsr_dist_stats(None, -1, 0.0, None, None, None) != 0
    assert lib.nsr_icp_stats(None, None, None, None, 4, 4, 0.1, None, None, None) != 0
    assert lib.nsr_transform_points(None, 3, None, None) != 0
    assert lib.nsr_cull_vertices(None, 3, 1, None, 1, 0, 10, 1., 1., 1., 1., None, 0, None, None, None) != 0
    assert b"empty image" in lib.nsr_last_error()


def test_cli_rejects_2d():
    with pytest.raises(NotImplementedError, match="rasterizer"):
        recon.main(["eval", "--rec_mesh", "a.ply", "--gt_mesh", "b.ply", "-2d"])
