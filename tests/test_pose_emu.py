"""CPU tests of the pose kernels (nice_slam_amd/csrc/nsr_pose.h, nice_slam_amd/poses.py): the kernel sources run on the emulator
against the fp64 restatement of tests/pose_reference.py under the gate derived there."""
import os
import sys

import numpy as np
import pytest
import torch

import emu_harness
import pose_reference as R
from conftest import ROOT
from nice_slam_amd import _capi
from nice_slam_amd.engine import Engine
from nice_slam_amd.poses import Trajectory, get_tensor_from_camera


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


def test_named_cases_sit_in_their_branches_away_from_ties():
    seen = set()
    for name, (m, branch) in R.named_poses().items():
        b, margin = R.branch_and_margin(m)
        assert b == branch and margin >= R.TIE_MARGIN, (name, b, margin)
        seen.add(b)
    assert seen == {0, 1, 2, 3}
    rnd = R.random_poses()
    assert len(rnd) == 64
    info = [R.branch_and_margin(m) for m in rnd]
    assert min(mg for _, mg in info) >= R.TIE_MARGIN              # so the reference's branch is the kernel's
    assert {b for b, _ in info} == {0, 1, 2, 3}


@pytest.mark.parametrize("rows", [12, 16])
@pytest.mark.parametrize("name", list(R.named_poses()))
def test_tensor_from_camera_named(E, name, rows):
    R.check_tensor_from_camera(E, R.named_poses()[name][0], rows)


@pytest.mark.parametrize("rows", [12, 16])
def test_tensor_from_camera_random_and_counts(E, rows):
    rnd = R.random_poses()
    got = R.check_tensor_from_camera(E, rnd, rows)                # n = 64
    one = R.check_tensor_from_camera(E, rnd[:1], rows)            # n = 1
    more = R.check_tensor_from_camera(E, np.concatenate([rnd, rnd[:1]]), rows)      # n = 65: past one round of the block's lanes
    assert one.tobytes() == got[:1].tobytes() and more[:64].tobytes() == got.tobytes() and more[64].tobytes() == got[0].tobytes()
    empty = get_tensor_from_camera(torch.zeros((0, rows // 4, 4)), engine=E)        # n = 0
    assert empty.shape == (0, 7)


def test_tensor_from_camera_equals_the_tools_restatement_and_round_trips(E):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import slam_synthetic as ss
    poses = np.concatenate([np.stack([m for m, _ in R.named_poses().values()]), R.random_poses()])
    got = R.check_tensor_from_camera(E, poses, 16)
    for k, m in enumerate(poses):
        R.gate(got[k], ss._cam_np(m).numpy(), f"_cam_np {k}")
    back = R.camera_from_tensor(E, got)
    assert np.abs(back.astype(np.float64) - poses[:, :3].astype(np.float64)).max() <= 4e-7


def test_drop_in_shapes_devices_and_order(E):
    m = R.named_poses()["branch2"][0]
    ref = R.cam_ref(m)
    for src in (m, m[:3], torch.from_numpy(m), torch.from_numpy(m[:3].copy())):
        got = get_tensor_from_camera(src, engine=E)
        assert got.shape == (7,) and got.dtype == torch.float32 and got.device.type == "cpu"
        R.gate(got.numpy(), ref)
    tq = get_tensor_from_camera(m, Tquad=True, engine=E)
    R.gate(tq.numpy(), np.concatenate([ref[4:], ref[:4]]))
    with pytest.raises(_capi.NsrError):
        get_tensor_from_camera(np.zeros((3, 3), np.float32), engine=E)
    lib = E.lib
    assert lib.nsr_tensor_from_camera(None, 1, 12, None, None) != 0 and b"null" in lib.nsr_last_error()
    assert lib.nsr_tensor_from_camera(None, 1, 9, None, None) != 0 and b"row_floats" in lib.nsr_last_error()


@pytest.mark.parametrize("const_speed", [False, True])
@pytest.mark.parametrize("idx", [1, 2, 5])
def test_predict(E, idx, const_speed):
    R.check_predict(E, idx, const_speed)


def test_predict_and_commit_ignore_an_index_outside_the_trajectory(E):
    traj = R.walk()
    T = Trajectory(len(traj), engine=E)
    T.est.copy_(torch.from_numpy(traj))
    cam = torch.full((7,), -3.0)
    hist = torch.from_numpy(R.commit_cases()["minimum_last"][0])
    for bad in (0, len(traj), -1):
        T.idx.fill_(bad)
        T.predict(cam)
        if bad != 0:                                               # frame 0 has no prediction, but it can be committed
            T.commit(hist)
    assert (cam == -3.0).all() and T.est.numpy().tobytes() == traj.tobytes()
    with pytest.raises(IndexError):
        T.set_index(len(traj))


@pytest.mark.parametrize("name", list(R.commit_cases()))
def test_commit(E, name):
    R.check_commit(E, name)


def test_commit_after_predict_keeps_the_prediction_when_no_row_is_taken(E):
    traj = R.walk()
    T = Trajectory(len(traj), engine=E)
    T.est.copy_(torch.from_numpy(traj))
    T.set_index(3)
    cam = torch.zeros(7)
    T.predict(cam)
    T.commit(torch.from_numpy(R.commit_cases()["all_nan_or_huge"][0]))
    R.gate(T.est[3].numpy(), R.predict_ref(traj, 3, True)[1])


@pytest.mark.parametrize("m", [0, 1, 5])
def test_store(E, m):
    R.check_store(E, m)
