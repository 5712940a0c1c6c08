"""GPU: the trajectory evaluation (nice_slam_amd/csrc/nsr_trajeval.h) through the product, on the cases and under the gates of
tests/trajeval_reference.py (the ones tests/test_trajeval_emu.py runs on the emulator)."""
import numpy as np
import pytest
import torch

import trajeval_reference as R

pytestmark = pytest.mark.gpu

STATS = ("rmse", "mean", "median", "std", "min", "max")


@pytest.fixture(scope="module")
def E():
    from nice_slam_amd.engine import gpu
    return gpu()


def test_the_references_own_results(E):
    gold = R.golden()
    for name, (est, gt, last, scale) in R.golden_cases().items():
        rec, err, res = R.check_case(E, est, gt, [last], scale, name)
        d = res.dict()
        ext = max(1.0, R.evaluate(est, gt, last, scale)["extent"])
        assert d["compared_pose_pairs"] == int(gold[name + "/pairs"])
        for i, k in enumerate(STATS):
            assert abs(d["absolute_translational_error." + k] - gold[name + "/stats"][i]) <= R.GATE * ext, (name, k)
    for name, (est, gt, *_r) in R.ate_golden_cases().items():
        R.check_case(E, R.poses_of(est), R.poses_of(gt), [est.shape[1] - 1], 1.0, name)


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_sizes(E, scale):
    for n in R.SIZES:
        est, gt = R.sized_case(n)
        R.check_case(E, est, gt, [n - 1], scale, f"n {n}")


def test_three_problems_masked_frames_ties_and_two_runs(E):
    for n in (63, 65, 256, 257):
        est, gt = R.sized_case(n, masked=True)
        lasts = [n - 1, n // 2 + 3, 7]
        rec, err, _ = R.check_case(E, est, gt, lasts, 0.37, f"masked n {n}")
        again, err2, _ = R.run(E, est, gt, lasts, 0.37)
        assert again.tobytes() == rec.tobytes() and err2.tobytes() == err.tobytes()           # bit-identical run to run
        one, one_err, _ = R.run(E, est, gt, lasts[1:2], 0.37)
        assert one[0].tobytes() == rec[1].tobytes() and one_err[0].tobytes() == err[1].tobytes()
    est, gt = R.tied_case()
    for last in (63, 62, 61):                                                        # 62 pairs: the two middle errors tie
        rec, err, _ = R.check_case(E, est, gt, [last], 1.0, "tied")
        assert (err[0, 0:last:2] == err[0, 1:last + 1:2]).all()


def test_degenerate_inputs(E):
    from nice_slam_amd import trajeval
    est, gt = R.sized_case(65)
    est[9, 1, 3] = np.nan
    rec, err, res = R.run(E, est, gt, [64, 8, 65, -1, 0], 1.0)
    assert rec[0, 0] == 65 and rec[0, 2] == 1 and rec[0, 25] == 4 and np.isnan(rec[0, 3:25]).all()
    R.check_record(rec[1], R.evaluate(est, gt, 8, 1.0), err[1])
    for b in (2, 3):
        assert (rec[b, :3] == 0).all() and np.isnan(rec[b, 3:25]).all() and rec[b, 25] == 3 and np.isnan(err[b]).all()
        with pytest.raises(ValueError):
            res.dict(b)
    assert rec[4, 0] == 1 and rec[4, 25] == 1 and np.array_equal(rec[4, 9:18], np.eye(3).reshape(-1))
    with pytest.raises(ValueError):
        res.dict(4)
    one = trajeval.evaluate_ate(est[:1], gt[:1])                                     # n_frames = 1
    assert one.record[0, 0] == 1 and one.record[0, 25] == 1


def test_a_million_frames(E):
    """n_frames = 2^20: every thread's chunk is 4096 frames; against numpy on the kernel's own errors and the restatement"""
    n = 1 << 20
    g = torch.Generator(device="cpu").manual_seed(3)
    p = torch.cumsum(torch.randn((n, 3), generator=g, dtype=torch.float64) * 0.01, 0)
    est, gt = R.walk(3, 1)
    Rm = torch.from_numpy(est[0, :3, :3].astype(np.float64))
    q = p @ Rm.T + 0.5 + torch.randn((n, 3), generator=g, dtype=torch.float64) * 0.02
    gt = torch.eye(4, dtype=torch.float32).repeat(n, 1, 1)
    est = gt.clone()
    gt[:, :3, 3], est[:, :3, 3] = p.float(), q.float()
    gt[12345, 0, 0] = float("nan")
    est, gt = est.numpy(), gt.numpy()
    rec, err, _ = R.run(E, est, gt, [n - 1], 1.0)
    assert rec[0, 0] == n - 1 and rec[0, 1] == 1
    R.check_own_statistics(rec[0], err[0], "2^20")
    want = R.evaluate(est, gt, n - 1, 1.0)
    assert R.gap(want["model"].T, want["data"].T) >= R.MIN_GAP
    # the gate's n eps / gap, for this n: 2^20 * 1.1e-16 / 0.05 = 2.3e-9, with the derivation's margin of 5
    tol = 5 * n * 1.1e-16 / R.MIN_GAP
    assert np.abs(rec[0, 9:18].reshape(3, 3) - want["rot"]).max() <= tol and abs(rec[0, 3] - want["stats"]["rmse"]) <= tol * max(1.0, want["extent"])


def test_plot_bytes(E):
    for name, (est, gt, last, scale) in R.golden_cases().items():
        R.check_plot(E, est, gt, last, scale, name)
    est, gt = R.sized_case(3)
    est[1], gt[1] = est[0], gt[0]
    R.check_plot(E, est, gt, 2, 1.0, "repeated")


def test_host_inputs_come_back_on_the_host(E):
    import nice_slam_amd as nsa
    est, gt, last, scale = R.golden_cases()["masked65"]
    res = nsa.evaluate_ate(est, gt, last=last, scale=scale, errors=True)
    assert res.record.device.type == "cpu" and res.errors.device.type == "cpu" and res.last.device.type == "cpu"
    R.check_record(res.record[0].numpy(), R.evaluate(est, gt, last, scale), res.errors[0].numpy())
    img = nsa.plot_trajectories(est, gt, res)
    assert img.device.type == "cpu" and img.numpy().tobytes() == R.draw(res.record[0].numpy(), est, gt, last, scale).tobytes()
    curve = nsa.ate_curve(list(torch.from_numpy(est)), list(torch.from_numpy(gt)), [10, 30, 64], scale=scale)
    assert curve.rmse.device.type == "cpu" and curve.rmse[2] == res.rmse[0]


def test_trajectory_ate_in_a_captured_graph(E):
    """Trajectory.ate(out=...) alone in a graph on one stream; replayed at two values of idx, each replay is the eager call bit for bit"""
    from nice_slam_amd import trajeval
    from nice_slam_amd.poses import Trajectory
    est, gt = R.sized_case(65, masked=True)
    T = Trajectory(65, engine=E)
    T.est.copy_(torch.from_numpy(est))
    T.gt.copy_(torch.from_numpy(gt))
    out = torch.zeros(32, dtype=torch.float64, device=E.device)
    T.set_index(64)
    T.ate(out=out, scale=0.37)                                                       # (loads the kernel before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.ate(out=out, scale=0.37)
    for idx in (40, 64):
        T.set_index(idx)
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy().copy()
        eager = T.ate(scale=0.37).cpu().numpy()
        want = trajeval.evaluate_ate(T.est, T.gt, last=idx, scale=0.37).record[0].cpu().numpy()
        assert got.tobytes() == eager.tobytes() == want.tobytes()
        R.check_record(got, R.evaluate(est, gt, idx, 0.37))
