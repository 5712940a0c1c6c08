"""GPU tests of reconstruction evaluation (nice_slam_amd.recon on libnsr.so): nearest neighbour at 200k x 200k against
cKDTree, pruning and run-to-run determinism, the surface sampler, ICP, the metrics and the cull against the golden minted from
the reference (tests/golden/make_golden_recon.py), a 2000-pose cull against a numpy restatement, an analytic room meshed and
scored end to end, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import mesh_reference as MR
import recon_scenes as RS
from test_recon_emu import icp_restated, sample_restated, write_traj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "recon_eval.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def clouds(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "surface":
        return RS.room_surface_points(n, seed) + rng.normal(scale=0.005, size=(n, 3))
    if kind == "uniform":
        return rng.uniform(-2, 2, (n, 3))
    centres = rng.uniform(-3, 3, (12, 3))
    return centres[rng.integers(0, 12, n)] + rng.normal(scale=0.05, size=(n, 3))


def check_exact(q, ref, d, i):
    """bit-exact against the kernel's operation order at the returned index, never farther than cKDTree's answer, and
    the same index wherever the nearest point is unique"""
    kd, ki = cKDTree(ref).query(q)
    def d2(idx):
        x = q - ref[idx]
        return (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    mine, theirs = d2(i), d2(ki)
    assert np.array_equal(d, np.sqrt(mine))
    assert np.all(mine <= theirs)
    assert np.all(np.abs(d - kd) <= np.spacing(np.maximum(d, kd)))
    differ = i != ki
    assert np.all(mine[differ] == theirs[differ])                  # a different index only at an exact tie
    assert np.all(i[differ] < ki[differ])                          # ... resolved to the smaller index


@pytest.mark.parametrize("kind", ["surface", "uniform", "clustered"])
def test_nearest_200k(kind):
    from nice_slam_amd import recon
    ref = clouds(kind, 200000, 1)
    q = clouds(kind, 200000, 2)
    idx = recon.NNIndex(torch.from_numpy(ref).to(DEV))
    d, i, nc = idx.query(torch.from_numpy(q).to(DEV), with_candidates=True)
    torch.cuda.synchronize()
    check_exact(q, ref, d.cpu().numpy(), i.cpu().numpy())
    d2, i2, nc2 = idx.query(torch.from_numpy(q).to(DEV), with_candidates=True)
    assert torch.equal(d, d2) and torch.equal(i, i2) and torch.equal(nc, nc2)     # bit-identical run to run
    if kind == "surface":
        assert nc.double().mean().item() < 100                    # the search prunes: 200k per query without it


def test_nearest_far_and_fp32():
    from nice_slam_amd import recon
    rng = np.random.default_rng(3)
    ref = clouds("surface", 50000, 4).astype(np.float32)
    far = rng.normal(size=(500, 3))
    q = np.concatenate([clouds("surface", 20000, 5), 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)]).astype(np.float32)
    d, i = recon.nearest(torch.from_numpy(q).to(DEV), torch.from_numpy(ref).to(DEV))
    check_exact(q.astype(np.float64), ref.astype(np.float64), d.cpu().numpy(), i.cpu().numpy())


def test_sampler():
    from nice_slam_amd import recon
    f, sp, org = RS.room_lattice(64)
    v, fc = MR.marching_cubes(f, 0.0, sp, org)
    rng = np.random.default_rng(6)
    u = rng.uniform(size=(300000, 3))
    p, fi = recon.sample_surface(torch.from_numpy(v).to(DEV), torch.from_numpy(fc).to(DEV), 300000, uniforms=torch.from_numpy(u).to(DEV))
    rp, rfi = sample_restated(v, fc, u)
    assert np.array_equal(fi.cpu().numpy(), rfi) and np.array_equal(p.cpu().numpy(), rp)
    # philox: points on their faces, faces drawn in proportion to their area (chi^2 over 24 faces of unequal areas)
    tv = rng.normal(size=(72, 3))
    tf = np.arange(72, dtype=np.int32).reshape(24, 3)
    n = 240000
    p, fi = recon.sample_surface(torch.from_numpy(tv).to(DEV), torch.from_numpy(tf).to(DEV), n, seed=11)
    p, fi = p.cpu().numpy(), fi.cpu().numpy()
    tri = tv[tf[fi]]
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.abs(((p - tri[:, 0]) * nrm).sum(1)) / np.linalg.norm(nrm, axis=1)).max() < 1e-12
    area = np.linalg.norm(np.cross(tv[tf[:, 1]] - tv[tf[:, 0]], tv[tf[:, 2]] - tv[tf[:, 0]]), axis=1) / 2
    expect = n * area / area.sum()
    chi2 = (((np.bincount(fi, minlength=24) - expect) ** 2) / expect).sum()
    assert chi2 < 49.7                                              # 23 dof, p = 0.001
    p2, _ = recon.sample_surface(torch.from_numpy(tv).to(DEV), torch.from_numpy(tf).to(DEV), n, seed=11)
    assert np.array_equal(p, p2.cpu().numpy())


def test_icp_recovers_motion():
    from nice_slam_amd import recon
    from nice_slam_amd.engine import gpu
    bf, bsp, borg = RS.bumpy_lattice(96)
    bv, _ = MR.marching_cubes(bf, 0.0, bsp, borg)
    M = RS.rigid([0.3, 0.5, 1.0], 5.0, [0.05, -0.03, 0.02])
    Mi = np.linalg.inv(M)
    src = bv @ Mi[:3, :3].T + Mi[:3, 3]
    T, fit, rmse, it = recon._icp(gpu(), torch.from_numpy(src).to(DEV), torch.from_numpy(bv).to(DEV))
    assert np.abs(T - M).max() < 1e-6 and fit == 1.0
    rT, rfit, rrmse, rit = icp_restated(src, bv)
    assert it == rit and np.abs(T - rT).max() < 1e-9
    T2, fit2, rmse2 = recon.align_icp(torch.from_numpy(src).to(DEV), torch.from_numpy(bv).to(DEV))
    assert np.array_equal(T, T2) and (fit, rmse) == (fit2, rmse2)


def test_metrics_match_golden(gold):
    from nice_slam_amd import recon
    for name in gold["cloud_names"]:
        gt = torch.from_numpy(gold[f"{name}/gt"]).to(DEV)
        rec = torch.from_numpy(gold[f"{name}/rec"]).to(DEV)
        acc, comp, ratio = recon.recon_metrics(gt, rec)
        assert acc == pytest.approx(float(gold[f"{name}/accuracy"]), rel=1e-12, abs=0), name
        assert comp == pytest.approx(float(gold[f"{name}/completion"]), rel=1e-12, abs=0), name
        assert ratio == float(gold[f"{name}/completion_ratio_0.05"]), name
        assert recon.completion_ratio(gt, rec, 0.02) == float(gold[f"{name}/completion_ratio_0.02"]), name
        assert recon.accuracy(gt, rec) == acc and recon.completion(gt, rec) == comp


def test_cull_matches_golden(gold, tmp_path):
    from nice_slam_amd import recon
    tp = str(tmp_path / "traj.txt")
    write_traj(tp, gold["cull/traj"])
    poses = recon.load_poses(tp)
    seen, keep = recon.cull_masks(torch.from_numpy(gold["cull/vertices"]).to(DEV), torch.from_numpy(gold["cull/faces"]).to(DEV), poses)
    assert np.array_equal(seen.cpu().numpy(), gold["cull/vertex_seen"])
    assert np.array_equal(keep.cpu().numpy(), gold["cull/face_keep"])


def cull_restated(verts, w2c, H=680, W=1200, fx=600., fy=600., cx=599.5, cy=339.5):
    """numpy fp32 restatement of the per-pose loop of cull_mesh.py:45-71 in the kernel's operation order"""
    p = verts.astype(np.float32)
    f32 = np.float32
    kf = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float64).astype(np.float32)
    seen = np.zeros(len(p), bool)
    for w in w2c.reshape(-1, 12):
        cam = [((w[4 * r] * p[:, 0] + w[4 * r + 1] * p[:, 1]) + w[4 * r + 2] * p[:, 2]) + w[4 * r + 3] * f32(1) for r in range(3)]
        X, Y, Z = cam[0] * f32(-1), cam[1], cam[2]
        uh = (kf[0] * X + kf[1] * Y) + kf[2] * Z
        vh = (kf[3] * X + kf[4] * Y) + kf[5] * Z
        z = ((kf[6] * X + kf[7] * Y) + kf[8] * Z) + f32(1e-5)
        u, v = uh / z, vh / z
        seen |= (f32(0) <= -z) & (u < f32(W)) & (u > f32(0)) & (v < f32(H)) & (v > f32(0))
    return seen


def test_cull_2000_poses():
    from nice_slam_amd import recon
    from nice_slam_amd.engine import w2c_rows
    rng = np.random.default_rng(8)
    verts = RS.room_surface_points(100000, 9)
    poses = []
    for k in range(2000):
        a = 2 * np.pi * k / 2000
        M = RS.rigid([0.2 * np.sin(3 * a), 1.0, 0.1], np.rad2deg(a), [2.5 + np.cos(a), 2.0 + np.sin(a), 1.5])
        poses.append(torch.from_numpy(M).float())
    seen, keep = recon.cull_masks(torch.from_numpy(verts).to(DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV), poses)
    ref = cull_restated(verts, w2c_rows(poses, np.float32))
    got = seen.cpu().numpy()
    assert 0 < ref.sum() < len(ref)
    assert np.array_equal(got, ref)


def test_room_end_to_end():
    """the analytic room meshed at 128^3 on the GPU, then scored against points on its exact surface.  Bounds from the CPU
    path on the same field (tests/mesh_reference.py marching cubes + cKDTree, 200k samples each): accuracy 1.158 cm,
    completion 1.160 cm, ratio 100 % -- the sampling spacing of 200k points on ~105 m^2 dominates (the voxel is 2.5-4.1 cm)."""
    from nice_slam_amd import marching_cubes, recon
    from nice_slam_amd.engine import gpu
    f, sp, org = RS.room_lattice(128)
    v, fc = marching_cubes(torch.from_numpy(f).to(DEV), 0.0, sp, org)
    gt = RS.room_surface_points(200000, 1)
    gtv = torch.from_numpy(gt).to(DEV)
    T = recon.align_icp(v, gtv)[0]
    assert np.abs(T - np.eye(4)).max() < 1e-4
    # the ground-truth "mesh" is a point set here: score the sampled reconstruction against the analytic samples
    rv = v.clone()
    gpu().transform(rv, T)
    rec = recon.sample_surface(rv, fc, 200000, seed=0)[0]
    acc, comp, ratio = recon.recon_metrics(gtv, rec)
    assert acc < 0.0135 and comp < 0.0135 and ratio == 1.0
    # calc_3d_metric on the device tensors marching_cubes / Mesher.get_mesh return (fp64 vertices, int32 faces)
    m = recon.calc_3d_metric((v, fc), (v, fc), align=True)
    assert m["completion_ratio_pct"] == 100.0 and m["accuracy_cm"] < 1.35 and m["completion_cm"] < 1.35


def test_cli(tmp_path, gold):
    from nice_slam_amd.ply import write_ply
    bf, bsp, borg = RS.bumpy_lattice(64)
    bv, bfc = MR.marching_cubes(bf, 0.0, bsp, borg)
    a, b = str(tmp_path / "rec.ply"), str(tmp_path / "gt.ply")
    write_ply(a, bv, bfc)
    write_ply(b, bv, bfc)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "nice_slam_amd.recon", "eval", "--rec_mesh", a, "--gt_mesh", b, "-3d"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines[-3:]] == ["accuracy", "completion", "completion ratio"]
    assert float(lines[-1].split()[-1]) == 100.0
    tp, out = str(tmp_path / "traj.txt"), str(tmp_path / "culled.ply")
    write_traj(tp, gold["cull/traj"])
    write_ply(str(tmp_path / "in.ply"), gold["cull/vertices"], gold["cull/faces"])
    r = subprocess.run([sys.executable, "-m", "nice_slam_amd.recon", "cull", "--input_mesh", str(tmp_path / "in.ply"), "--traj", tp,
                        "--output_mesh", out], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    from nice_slam_amd.ply import read_mesh
    cv, cf = read_mesh(out)
    assert len(cv) == len(gold["cull/vertices"]) and len(cf) > 0
