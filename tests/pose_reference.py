"""TEST INFRASTRUCTURE: fp64 numpy restatement of the pose kernels (nice_slam_amd/csrc/nsr_pose.h), their cases, and the checks
that tests/test_pose_emu.py runs on the emulator and tests/test_hip_pose.py on the GPU, both through an ``Engine``.

Gate of every comparison: |got - ref| <= 2^-23 |ref| + 1e-12 per element.  The kernels compute in fp64 and round to fp32 once: that
is half an fp32 ulp, 2^-24 |ref|; the gate allows it twice over.  The additive term stands for the fp64 error of the chain
itself -- at most a few hundred fp64 ulps (1e-14) through the 4x4 inverse of a pose with translations up to 10 m.
"""
import math

import numpy as np
import torch

from nice_slam_amd.poses import Trajectory, get_tensor_from_camera

TIE_MARGIN = 1e-3


def gate(got, ref, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    tol = 2.0 ** -23 * np.abs(ref) + 1e-12
    assert (err <= tol).all(), (what, float((err - tol).max()), np.argwhere(err > tol)[:4].tolist())


# --------------------------------------------------------------------------------------------------
# restatement
# --------------------------------------------------------------------------------------------------
def branch_and_margin(m):
    """(Shepperd branch 0..3 of the rotation, distance of the deciding comparisons from a tie)"""
    r00, r11, r22 = float(m[0, 0]), float(m[1, 1]), float(m[2, 2])
    t = r00 + r11 + r22
    if t > 0.0:
        return 0, abs(t)
    if r00 > r11 and r00 > r22:
        return 1, min(abs(t), r00 - r11, r00 - r22)
    if r11 > r22:
        return 2, min(abs(t), max(r11 - r00, r22 - r00), r11 - r22)
    return 3, min(abs(t), max(r11 - r00, r22 - r00), r22 - r11)


def cam_ref(m):
    """3x4 / 4x4 (values as stored, fp32) -> [w, x, y, z | T] in fp64"""
    m = np.asarray(m, np.float64)
    r00, r11, r22 = m[0, 0], m[1, 1], m[2, 2]
    t = r00 + r11 + r22
    if t > 0.0:
        s = 2.0 * math.sqrt(t + 1.0)
        q = [0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s]
    elif r00 > r11 and r00 > r22:
        s = 2.0 * math.sqrt(1.0 + r00 - r11 - r22)
        q = [(m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s]
    elif r11 > r22:
        s = 2.0 * math.sqrt(1.0 + r11 - r00 - r22)
        q = [(m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s]
    else:
        s = 2.0 * math.sqrt(1.0 + r22 - r00 - r11)
        q = [(m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s]
    q = np.array(q, np.float64)
    return np.concatenate([q / math.sqrt(float(q @ q)), m[:3, 3]])


def pose_ref(c):
    """[w, x, y, z | T] -> 4x4 in fp64 (quad2rotation, src/common.py:137-176)"""
    c = np.asarray(c, np.float64)
    w, x, y, z = c[:4]
    s = 2.0 / (w * w + x * x + y * y + z * z)
    m = np.eye(4)
    m[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    m[:3, 3] = c[4:7]
    return m


def predict_ref(traj, idx, const_speed):
    """(cam fp64 [7], its 4x4) of frame idx (src/Tracker.py:192-201)"""
    t = np.asarray(traj, np.float64)
    pre = t[idx - 1]
    init = pre @ np.linalg.inv(t[idx - 2]) @ pre if (const_speed and idx >= 2) else pre
    cam = cam_ref(init)
    return cam, pose_ref(cam)


def commit_ref(hist):
    """row taken by src/Tracker.py:224,245-247, or None"""
    low, taken = 1e10, None
    for i, row in enumerate(np.asarray(hist, np.float64)):
        if row[0] < low:
            low, taken = row[0], i
    return taken


# --------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------
def axis_angle(axis, deg):
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    a = np.deg2rad(deg)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def pose44(R, t):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3], m[:3, 3] = R, t
    return m


def named_poses():
    """name -> (4x4 fp32, expected branch)"""
    out = {"identity": (pose44(np.eye(3), [0, 0, 0]), 0),
           "branch0": (pose44(axis_angle([0.3, -0.5, 0.8], 40.0), [1.5, -0.25, 3.0]), 0),
           "branch1": (pose44(axis_angle([0.9, 0.3, -0.2], 170.0), [-2.0, 0.5, 0.125]), 1),
           "branch2": (pose44(axis_angle([0.2, -0.9, 0.3], 165.0), [0.0, 7.5, -1.0]), 2),
           "branch3": (pose44(axis_angle([-0.3, 0.2, 0.9], 175.0), [9.5, -9.5, 4.0]), 3),
           "turn_x": (pose44(np.diag([1.0, -1.0, -1.0]), [1, 2, 3]), 1),
           "turn_y": (pose44(np.diag([-1.0, 1.0, -1.0]), [1, 2, 3]), 2),
           "turn_z": (pose44(np.diag([-1.0, -1.0, 1.0]), [1, 2, 3]), 3)}
    return out


def random_poses(n=64, seed=7):
    """n random rotations (uniform quaternions) with translations up to 10 m, each at least TIE_MARGIN from a branch tie"""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        q = rng.normal(size=4)
        m = pose44(pose_ref(np.concatenate([q, [0, 0, 0]]))[:3, :3], rng.uniform(-10, 10, 3))
        if branch_and_margin(m)[1] >= TIE_MARGIN:
            out.append(m)
    return np.stack(out)


def walk(n=6, seed=3):
    """a smooth trajectory [n,4,4] fp32 a few metres from the origin"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        R = axis_angle([0.2, 1.0, 0.1], 25.0 + 3.0 * k + rng.uniform(-0.3, 0.3))
        out.append(pose44(R, [3.0 + 0.05 * k, -2.5 + 0.01 * k * k, 4.0 - 0.03 * k] + rng.uniform(-0.005, 0.005, 3)))
    return np.stack(out)


# --------------------------------------------------------------------------------------------------
# checks through an engine
# --------------------------------------------------------------------------------------------------
def camera_from_tensor(E, cam):
    """nsr_camera_from_tensor on the engine: [B,7] fp32 -> [B,3,4] numpy"""
    c = torch.as_tensor(np.asarray(cam, np.float32)).reshape(-1, 7).contiguous().to(E.device)
    rt = torch.empty((c.shape[0], 3, 4), dtype=torch.float32, device=E.device)
    with E.guard():
        E.lib.check(E.lib.nsr_camera_from_tensor(c.data_ptr(), c.shape[0], rt.data_ptr(), None, None, E.stream()), "nsr_camera_from_tensor")
    return rt.cpu().numpy()


def check_tensor_from_camera(E, poses, rows):
    """poses [n,4,4] fp32 through 3x4 (rows = 12) or 4x4 (16) input"""
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    src = poses if rows == 16 else np.ascontiguousarray(poses[:, :3])
    got = get_tensor_from_camera(torch.from_numpy(src).to(E.device), engine=E)
    assert got.shape == (poses.shape[0], 7) and got.dtype == torch.float32 and got.device == E.device
    got = got.cpu().numpy()
    for k, m in enumerate(poses):
        gate(got[k], cam_ref(m), f"pose {k}")
    return got


def check_predict(E, idx, const_speed):
    traj = walk()
    T = Trajectory(len(traj), engine=E)
    T.est.copy_(torch.from_numpy(traj))
    T.est[idx:] = float("nan")                          # nothing behind idx - 1 is read
    T.set_index(idx)
    cam = torch.full((7,), float("nan"), device=E.device)
    T.predict(cam, const_speed=const_speed)
    cam_r, m_r = predict_ref(traj, idx, const_speed)
    est = T.est.cpu().numpy()
    gate(cam.cpu().numpy(), cam_r, "cam")
    gate(est[idx], m_r, "traj[idx]")
    assert np.array_equal(est[:idx], traj[:idx]) and np.isnan(est[idx + 1:]).all()
    # ... and traj[idx] is the pose of the 7-vector as returned in fp32: an fp32 rounding of each quaternion component moves an
    # entry of the rotation by at most 4 * 2^-24 * 2 < 4e-7
    assert np.abs(est[idx] - pose_ref(cam.cpu().numpy())).max() <= 4e-7
    if not (const_speed and idx >= 2):
        gate(cam.cpu().numpy(), cam_ref(traj[idx - 1]), "copy of the previous pose")


def commit_cases():
    rng = np.random.RandomState(11)

    def hist(losses):
        h = rng.normal(size=(len(losses), 8)).astype(np.float32)
        h[:, 5:] *= 3.0
        h[:, 0] = losses
        return h
    nan = float("nan")
    return {"one_iteration": (hist([2.5]), 0),
            "tie_first_wins": (hist([5.0, 3.0, 4.0, 3.0, 3.5]), 1),
            "nan_in_the_middle": (hist([7.0, 6.0, nan, 5.5, 6.5]), 3),
            "all_nan_or_huge": (hist([nan, 1e10, 2e10, nan]), None),
            "minimum_last": (hist([4.0, 3.0, 2.0, 1.0]), 3)}


def check_commit(E, name):
    hist, expect = commit_cases()[name]
    assert commit_ref(hist) == expect
    traj = walk()
    idx = 4
    T = Trajectory(len(traj), engine=E)
    T.est.copy_(torch.from_numpy(traj))
    T.set_index(idx)
    best = torch.full((8,), -7.0, device=E.device)
    T.commit(torch.from_numpy(hist).to(E.device), best)
    est = T.est.cpu().numpy()
    keep = np.arange(len(traj)) != idx
    assert np.array_equal(est[keep], traj[keep])
    if expect is None:
        assert np.array_equal(est[idx], traj[idx]) and (best.cpu().numpy() == -7.0).all()
    else:
        gate(est[idx], pose_ref(hist[expect, 1:]), "traj[idx]")
        assert best.cpu().numpy().tobytes() == hist[expect].tobytes()
    return est[idx]


def check_store(E, m):
    rng = np.random.RandomState(5)
    cams = rng.normal(size=(m, 7)).astype(np.float32)
    index = np.array([6, 0, 3, 7, 2][:m], dtype=np.int64)              # not in order
    table = rng.normal(size=(8, 4, 4)).astype(np.float32)
    T = Trajectory(8, engine=E)
    dst = torch.from_numpy(table.copy()).to(E.device)
    T.store(torch.from_numpy(cams).to(E.device), torch.from_numpy(index).to(E.device), dst)
    got = dst.cpu().numpy()
    for r in range(8):
        if r in index:
            gate(got[r], pose_ref(cams[list(index).index(r)]), f"row {r}")
        else:
            assert np.array_equal(got[r], table[r])
    T.est.copy_(torch.from_numpy(table))                               # default table: the trajectory
    T.store(torch.from_numpy(cams).to(E.device), torch.from_numpy(index).to(E.device))
    assert T.est.cpu().numpy().tobytes() == got.tobytes()
