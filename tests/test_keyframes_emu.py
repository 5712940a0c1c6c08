"""CPU: the overlap keyframe selection kernel (``nsr_keyframe_overlap``) executed under the fiber emulator, against the
unmodified reference (tests/golden/keyframe_overlap.npz, minted by make_golden_keyframes.py) and against the numpy
restatement in tests/keyframe_reference.py; the host half of ``KeyframeSelector.keyframe_selection_overlap`` on the
emulator's counts; argument rejection of the real libnsr.so (no device work is reached)."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import keyframe_reference as kr
from conftest import ROOT
from emu_harness import emu_lib, ptr

GOLD = os.path.join(ROOT, "tests", "golden", "keyframe_overlap.npz")
CALLERS = os.path.join(ROOT, "tests", "golden", "caller_steps.npz")


def run_counts(lib, indices, depth, c2w, w2c, N, intr, edge=20, c2w_stride=4):
    H, W, fx, fy, cx, cy = intr
    K = w2c.shape[0]
    idx = np.ascontiguousarray(indices, dtype=np.int64)
    c2w = np.ascontiguousarray(c2w, dtype=np.float32)
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    w2c = np.ascontiguousarray(w2c, dtype=np.float32)
    cnt = np.full(K + 1, -7, dtype=np.int32)                   # one guard word behind the K counts
    tv = kr.t_vals(N)
    lib.check(lib.nsr_keyframe_overlap(ptr(idx), idx.shape[0], N, tv.ctypes.data_as(C.POINTER(C.c_float)), int(H), int(W),
                                       fx, fy, cx, cy, edge, ptr(c2w), c2w_stride, ptr(depth), ptr(w2c), K, ptr(cnt), None),
              "nsr_keyframe_overlap")
    assert cnt[K] == -7
    return cnt[:K].astype(np.int64)


def set_state(g, p):
    np.random.set_state(("MT19937", g[p + "rng_keys"], int(g[p + "rng_pos"]), int(g[p + "rng_has_gauss"]), float(g[p + "rng_gauss"])))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _intr(g):
    H, W, fx, fy, cx, cy = (float(v) for v in g["intr"])
    return int(H), int(W), fx, fy, cx, cy


def test_fixture_counts_match_reference_exactly(gold):
    lib = emu_lib()
    intr = _intr(gold)
    H, W, fx, fy, cx, cy = intr
    flips = []
    for case in gold["cases"]:
        p = case + "/"
        est = gold[p + "est_c2w"]
        n, N = int(gold[p + "pixels"]), int(gold[p + "n_samples"])
        got = run_counts(lib, gold[p + "indices"], gold["depth"], gold[p + "c2w"], kr.w2c_rows(est), N, intr)
        want = np.rint(gold[p + "percent"] * (n * N)).astype(np.int64)
        assert got.shape == want.shape
        # the kernel is the restatement, exactly
        assert np.array_equal(got, kr.counts(gold[p + "indices"], gold["depth"], gold[p + "c2w"], est, fx, fy, cx, cy, N)), case
        if np.array_equal(got, want):
            continue
        # the one excused deviation: numpy's BLAS summing w2c @ p (or K @ cam) in another order than left to right
        pts = kr.points(gold[p + "indices"], gold["depth"], gold[p + "c2w"], fx, fy, cx, cy, N)
        seq, u, v, zc = kr.inside(pts, kr.w2c_rows(est), H, W, fx, fy, cx, cy)
        mm = kr.inside_matmul(pts, est, H, W, fx, fy, cx, cy)[0]
        assert np.array_equal(mm.sum(1), want), (case, "the reference's counts are not the matmul restatement's")
        for kk, i in zip(*np.nonzero(seq != mm)):
            assert kr.near_boundary(u[kk, i], v[kk, i], zc[kk, i], H, W), (case, kk, i, u[kk, i], v[kk, i], zc[kk, i])
            flips.append((str(case), int(kk), int(i), float(u[kk, i]), float(v[kk, i]), float(zc[kk, i])))
    print("summation-order flips (case, keyframe, point, u, v, z):", flips)


def test_fixture_selection_and_rng_state(gold):
    from nice_slam_amd.keyframes import select_overlapping
    lib = emu_lib()
    intr = _intr(gold)
    for case in gold["cases"]:
        p = case + "/"
        est = gold[p + "est_c2w"]
        n, N, k = int(gold[p + "pixels"]), int(gold[p + "n_samples"]), int(gold[p + "k"])
        counts = run_counts(lib, gold[p + "indices"], gold["depth"], gold[p + "c2w"], kr.w2c_rows(est), N, intr)
        set_state(gold, p)
        sel = select_overlapping(counts, n * N, k)
        after = np.random.random(4)
        assert sel == gold[p + "out"].tolist(), case
        assert [type(v).__name__ for v in sel] == gold[p + "out_types"].tolist() and all(type(v) is np.int64 for v in sel)
        assert np.array_equal(after, gold[p + "after"]), case          # the permutation used up the same draws
        if len(est):
            order = sorted(range(len(est)), key=lambda i: counts[i] / (n * N), reverse=True)
            assert order == gold[p + "sorted_ids"].tolist(), case
    assert {str(c) for c in gold["cases"]} >= {"k0", "k1", "k7", "k40", "k150"}


def test_caller_fixture_window():
    """The first draw of the recorded optimize_map calls is the selection's (Mapper.py:185, before the iterations): the
    selection on it, under numpy seed 11, names the keyframes the real optimize_map put into its window, in its order."""
    from nice_slam_amd.keyframes import select_overlapping
    g = np.load(CALLERS)
    H, W, fx, fy, cx, cy = (float(v) for v in g["intr"])
    intr = (int(H), int(W), fx, fy, cx, cy)
    lib = emu_lib()
    for pre in ("map/", "ba/"):
        n_kf = 0
        while f"{pre}kf/{n_kf}/frame" in g:
            n_kf += 1
        est = [g[f"{pre}kf/{i}/est_c2w_in"] for i in range(n_kf - 1)]          # keyframe_dict[:-1] (Mapper.py:264-265)
        order = [int(v) for v in g[pre + "draw_frames"]]
        per_iter = (len(order) - 1) // int(g[pre + "n_iters"])
        window = order[1:1 + per_iter]                                          # selected..., last keyframe, current (0)
        want = [int(g[f"{pre}kf/{i}/frame"]) for i in range(n_kf)]
        want = [want.index(f) for f in window[:-2]]
        counts = run_counts(lib, g[pre + "draw/0"], g["frame/0/depth"], g[pre + "cur_c2w"], kr.w2c_rows(est), 16, intr)
        np.random.seed(11)
        assert select_overlapping(counts, 100 * 16, 3) == want, pre


@pytest.mark.parametrize("K,n_rays,N", [(300, 100, 16), (5, 150, 24), (3, 40, 64), (20, 100, 1), (1, 1, 1), (270, 37, 64)])
def test_random_scenes_match_restatement(K, n_rays, N):
    """more keyframes than blocks in the grid (256), more points than one LDS chunk (2048), N_samples 1 and 64"""
    rng = np.random.default_rng(K * 1000 + n_rays * 7 + N)
    H, W, fx, fy, cx, cy = 60, 80, 70.0, 69.0, 39.5, 30.25
    depth, c2w, est, idx = kr.random_scene(rng, H, W, K, n_rays)
    got = run_counts(emu_lib(), idx, depth, c2w, kr.w2c_rows(est), N, (H, W, fx, fy, cx, cy))
    want = kr.counts(idx, depth, c2w, est, fx, fy, cx, cy, N)
    assert np.array_equal(got, want)
    assert (want > 0).any() and (want == 0).any() or K < 5


def test_pose_stride_and_k0():
    """a 3x4 current pose (row stride 4) or a 4x4 one give the same counts; K = 0 writes nothing and succeeds"""
    rng = np.random.default_rng(5)
    H, W, fx, fy, cx, cy = 60, 80, 70.0, 69.0, 39.5, 30.25
    depth, c2w, est, idx = kr.random_scene(rng, H, W, 9, 50)
    lib = emu_lib()
    a = run_counts(lib, idx, depth, c2w, kr.w2c_rows(est), 16, (H, W, fx, fy, cx, cy))
    b = run_counts(lib, idx, depth, c2w[:3], kr.w2c_rows(est), 16, (H, W, fx, fy, cx, cy))
    wide = np.zeros((3, 6), np.float32)
    wide[:, :4] = c2w[:3]
    c = run_counts(lib, idx, depth, wide, kr.w2c_rows(est), 16, (H, W, fx, fy, cx, cy), c2w_stride=6)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert run_counts(lib, idx, depth, c2w, np.zeros((0, 12), np.float32), 16, (H, W, fx, fy, cx, cy)).shape == (0,)


@pytest.fixture(scope="module")
def real_lib():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from nice_slam_amd import _capi, build
    build.build_lib()
    return _capi.Lib(_capi.LIB_PATH)


def test_argument_rejection_without_device_work(real_lib):
    lib = real_lib
    idx = np.zeros(4, np.int64)
    tv = kr.t_vals(16)
    c2w = np.eye(4, dtype=np.float32)
    depth = np.ones((60, 80), np.float32)
    w2c = np.zeros((2, 12), np.float32)
    cnt = np.zeros(2, np.int32)
    tvp = tv.ctypes.data_as(C.POINTER(C.c_float))
    base = dict(indices=ptr(idx), n_rays=4, n_samples=16, t=tvp, H=60, W=80, edge=20, c2w=ptr(c2w), stride=4,
                depth=ptr(depth), w2c=ptr(w2c), K=2, counts=ptr(cnt))

    def call(**kw):
        a = dict(base, **kw)
        return lib.nsr_keyframe_overlap(a["indices"], a["n_rays"], a["n_samples"], a["t"], a["H"], a["W"], 70.0, 69.0, 39.5, 30.0,
                                        a["edge"], a["c2w"], a["stride"], a["depth"], a["w2c"], a["K"], a["counts"], None)

    bad = [dict(indices=None), dict(t=None), dict(c2w=None), dict(depth=None), dict(w2c=None), dict(counts=None), dict(K=-1),
           dict(n_rays=0), dict(n_rays=-3), dict(n_samples=0), dict(n_samples=65), dict(edge=40), dict(edge=30, H=60),
           dict(edge=-1), dict(stride=3), dict(H=0)]
    for kw in bad:
        assert call(**kw) != 0, kw
        msg = lib.nsr_last_error()
        assert msg and msg.startswith(b"nsr_keyframe_overlap"), (kw, msg)
    assert call(K=0, w2c=None, counts=None) == 0              # K = 0: valid, launches nothing
