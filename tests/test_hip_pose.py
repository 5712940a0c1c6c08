"""GPU: the pose kernels (nice_slam_amd/csrc/nsr_pose.h) through the product, on the cases and under the gate of
tests/pose_reference.py (the same ones tests/test_pose_emu.py runs on the emulator)."""
import numpy as np
import pytest
import torch

import pose_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from nice_slam_amd.engine import gpu
    return gpu()


@pytest.mark.parametrize("rows", [12, 16])
def test_tensor_from_camera(E, rows):
    named = np.stack([m for m, _ in R.named_poses().values()])
    rnd = R.random_poses()
    R.check_tensor_from_camera(E, named, rows)
    got = R.check_tensor_from_camera(E, np.concatenate([rnd, rnd[:1]]), rows)        # n = 65
    one = R.check_tensor_from_camera(E, rnd[:1], rows)
    assert one.tobytes() == got[:1].tobytes() and got[64].tobytes() == got[0].tobytes()
    import nice_slam_amd as nsa
    assert nsa.get_tensor_from_camera(torch.zeros((0, rows // 4, 4), device=E.device)).shape == (0, 7)
    back = nsa.get_camera_from_tensor(torch.from_numpy(got[:64]).to(E.device)).cpu().numpy()
    assert np.abs(back.astype(np.float64) - rnd[:, :3].astype(np.float64)).max() <= 4e-7
    host = nsa.get_tensor_from_camera(rnd[0], Tquad=True)                              # host input: the result comes back to the host
    assert host.device.type == "cpu"
    R.gate(host.numpy(), np.concatenate([R.cam_ref(rnd[0])[4:], R.cam_ref(rnd[0])[:4]]))


@pytest.mark.parametrize("const_speed", [False, True])
@pytest.mark.parametrize("idx", [1, 2, 5])
def test_predict(E, idx, const_speed):
    R.check_predict(E, idx, const_speed)


@pytest.mark.parametrize("name", list(R.commit_cases()))
def test_commit(E, name):
    R.check_commit(E, name)


@pytest.mark.parametrize("m", [0, 1, 5])
def test_store(E, m):
    R.check_store(E, m)
