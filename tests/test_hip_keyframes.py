"""GPU: overlap keyframe selection (nice_slam_amd.KeyframeSelector, nsr_keyframe_overlap) against the unmodified reference
(tests/golden/keyframe_overlap.npz), the numpy restatement (tests/keyframe_reference.py) and the recorded optimize_map calls
(tests/golden/caller_steps.npz)."""
import os

import numpy as np
import pytest
import torch

import keyframe_reference as kr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_overlap.npz")
CALLERS = os.path.join(ROOT, "tests", "golden", "caller_steps.npz")


def _sel(intr):
    import nice_slam_amd as nsa
    return nsa.KeyframeSelector(*intr)


def _intr(g):
    H, W, fx, fy, cx, cy = (float(v) for v in g["intr"])
    return int(H), int(W), fx, fy, cx, cy


def _set_state(g, p):
    np.random.set_state(("MT19937", g[p + "rng_keys"], int(g[p + "rng_pos"]), int(g[p + "rng_has_gauss"]), float(g[p + "rng_gauss"])))


def test_fixture_counts_and_selection(monkeypatch):
    g = np.load(GOLD)
    intr = _intr(g)
    sel = _sel(intr)
    depth = torch.from_numpy(g["depth"]).to(DEV)
    real_randint = torch.randint
    for case in g["cases"]:
        p = case + "/"
        n, N, k = int(g[p + "pixels"]), int(g[p + "n_samples"]), int(g[p + "k"])
        est = [torch.from_numpy(m).to(DEV) for m in g[p + "est_c2w"]]
        c2w = torch.from_numpy(g[p + "c2w"]).to(DEV)
        counts = sel.overlap(c2w, depth, est, N_samples=N, pixels=n, indices=torch.from_numpy(g[p + "indices"]))
        assert counts.dtype == torch.int32 and counts.device.type == "cuda" and counts.shape == (len(est),)
        want = np.rint(g[p + "percent"] * (n * N)).astype(np.int64)
        assert np.array_equal(counts.cpu().numpy().astype(np.int64), want), case
        # the drop-in, with its pixel draw teacher-forced to the recorded one
        drawn = []

        def forced(high, size, device=None, **kw):
            assert high == intr[0] * intr[1] and tuple(size) == (n,)
            drawn.append(1)
            return torch.from_numpy(g[p + "indices"]).to(device)

        monkeypatch.setattr(torch, "randint", forced)
        _set_state(g, p)
        kfd = [{"est_c2w": e, "idx": 50 * i} for i, e in enumerate(est)]
        out = sel.keyframe_selection_overlap(None, depth, c2w, kfd, k, N_samples=N, pixels=n)
        after = np.random.random(4)
        monkeypatch.setattr(torch, "randint", real_randint)
        assert drawn == [1]
        assert out == g[p + "out"].tolist() and all(type(v) is np.int64 for v in out), case
        assert np.array_equal(after, g[p + "after"]), case


@pytest.mark.parametrize("K", [1, 7, 40, 255, 256, 257, 1000])
def test_random_scenes_match_restatement(K):
    rng = np.random.default_rng(K)
    H, W, fx, fy, cx, cy = 120, 160, 130.0, 131.5, 79.5, 60.0
    for n_rays, N in ((100, 16), (150, 24), (33, 64), (64, 1)):
        depth, c2w, est, idx = kr.random_scene(rng, H, W, K, n_rays)
        sel = _sel((H, W, fx, fy, cx, cy))
        got = sel.overlap(torch.from_numpy(c2w).to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(est).to(DEV),
                          N_samples=N, pixels=n_rays, indices=torch.from_numpy(idx))
        want = kr.counts(idx, depth, c2w, est, fx, fy, cx, cy, N)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (K, n_rays, N)


@pytest.mark.parametrize("seed", [0, 3])
def test_drop_in_draw_and_rng_state(seed):
    """without indices the drop-in draws one torch.randint(H*W, (pixels,)) on the depth's device: its output equals the
    restatement fed with that draw, and the CUDA generator ends where that one draw leaves it"""
    rng = np.random.default_rng(100 + seed)
    H, W, fx, fy, cx, cy = 120, 160, 130.0, 131.5, 79.5, 60.0
    depth, c2w, est, _ = kr.random_scene(rng, H, W, 60, 1)
    sel = _sel((H, W, fx, fy, cx, cy))
    d_dev = torch.from_numpy(depth).to(DEV)
    kfd = [{"est_c2w": torch.from_numpy(m).to(DEV)} for m in est]
    torch.cuda.manual_seed(seed)
    np.random.seed(seed)
    out = sel.keyframe_selection_overlap(None, d_dev, torch.from_numpy(c2w).to(DEV), kfd, 5)
    st_got = torch.cuda.get_rng_state()
    np_after = np.random.random(3)
    torch.cuda.manual_seed(seed)
    idx = torch.randint(H * W, (100,), device=DEV)
    st_want = torch.cuda.get_rng_state()
    np.random.seed(seed)
    want = kr.select(kr.counts(idx.cpu().numpy(), depth, c2w, est, fx, fy, cx, cy, 16), 1600, 5)
    assert out == want and len(out) == 5
    assert torch.equal(st_got, st_want)
    assert np.array_equal(np_after, np.random.random(3))


def test_pose_sources_and_cache():
    """est_c2w on the CPU and on the device give the same counts; a BA-style replacement of one pose tensor, or an in-place
    edit of one, is seen by the next call although the inverses are cached"""
    rng = np.random.default_rng(9)
    H, W, fx, fy, cx, cy = 120, 160, 130.0, 131.5, 79.5, 60.0
    depth, c2w, est, idx = kr.random_scene(rng, H, W, 12, 100)
    sel = _sel((H, W, fx, fy, cx, cy))
    d_dev, c_dev, i_t = torch.from_numpy(depth).to(DEV), torch.from_numpy(c2w).to(DEV), torch.from_numpy(idx)
    dev_poses = [torch.from_numpy(m).to(DEV) for m in est]
    cpu_poses = [torch.from_numpy(m.copy()) for m in est]
    want = kr.counts(idx, depth, c2w, est, fx, fy, cx, cy, 16)
    for poses in (dev_poses, cpu_poses, dev_poses, list(est)):
        assert np.array_equal(sel.overlap(c_dev, d_dev, poses, indices=i_t).cpu().numpy(), want)
    assert len(sel._inv) == 0                                          # numpy poses are never cached
    sel.overlap(c_dev, d_dev, dev_poses, indices=i_t)
    assert len(sel._inv) == 12
    j = int(np.argmax(want))
    away = est.copy()
    away[j] = c2w.copy()
    away[j][:3, :3] = -away[j][:3, :3] * np.array([1, -1, 1], np.float32)[None, :]   # turned by pi about its y axis
    want2 = kr.counts(idx, depth, c2w, away, fx, fy, cx, cy, 16)
    assert want2[j] != want[j]
    dev_poses[j] = torch.from_numpy(away[j]).to(DEV)                  # replaced tensor (Mapper.py: est_c2w = c2w.clone())
    assert np.array_equal(sel.overlap(c_dev, d_dev, dev_poses, indices=i_t).cpu().numpy(), want2)
    dev_poses[j] = torch.from_numpy(est[j]).to(DEV)
    assert np.array_equal(sel.overlap(c_dev, d_dev, dev_poses, indices=i_t).cpu().numpy(), want)
    dev_poses[j].copy_(torch.from_numpy(away[j]))                     # edited in place: _version moves
    assert np.array_equal(sel.overlap(c_dev, d_dev, dev_poses, indices=i_t).cpu().numpy(), want2)
    assert sel.overlap(c_dev, d_dev, [], indices=i_t).shape == (0,)


def test_caller_fixture_window(monkeypatch):
    """the drop-in, on the first recorded draw of optimize_map (its pixel draw teacher-forced) and under the numpy seed the
    recording set, picks the window the real optimize_map picked, in its order"""
    g = np.load(CALLERS)
    intr = _intr(g)
    sel = _sel(intr)
    depth = torch.from_numpy(g["frame/0/depth"]).to(DEV)
    color = torch.from_numpy(g["frame/0/color"]).to(DEV)
    for pre in ("map/", "ba/"):
        n_kf = 0
        while f"{pre}kf/{n_kf}/frame" in g:
            n_kf += 1
        kfd = [{"est_c2w": torch.from_numpy(g[f"{pre}kf/{i}/est_c2w_in"]).to(DEV)} for i in range(n_kf)]
        order = [int(v) for v in g[pre + "draw_frames"]]
        per_iter = (len(order) - 1) // int(g[pre + "n_iters"])
        frames = [int(g[f"{pre}kf/{i}/frame"]) for i in range(n_kf)]
        want = [frames.index(f) for f in order[1:1 + per_iter][:-2]]
        drawn = []

        def forced(high, size, device=None, **kw):
            assert high == intr[0] * intr[1] and tuple(size) == (100,)
            drawn.append(1)
            return torch.from_numpy(g[pre + "draw/0"]).to(device)

        monkeypatch.setattr(torch, "randint", forced)
        np.random.seed(11)
        got = sel.keyframe_selection_overlap(color, depth, torch.from_numpy(g[pre + "cur_c2w"]).to(DEV), kfd[:-1], 3)
        monkeypatch.undo()
        assert drawn == [1] and got == want, pre
