"""TEST INFRASTRUCTURE: numpy / fp64 restatement of src/tools/eval_ate.py as nice_slam_amd/csrc/nsr_trajeval.h computes it -- the mask
and scale of convert_poses (:239-256), align (:44-78, LAPACK's SVD as there), the statistics (:215-223), matplotlib's data -> display
transform of the figure (:196-204, :213) and the kernel's pixel rule -- and the cases the trajectory tests share.

Gate (tests/test_trajeval_emu.py, tests/test_hip_trajeval.py): 1e-10 on rot, 1e-10 max(1, extent) on trans, the errors, the
statistics and the limits.  The alignment's rounding error is at most about n eps / gap with gap = (s2 +- s3) / s1 of the singular
values of W (+ for det > 0, - for the mirrored case): at n = 4096 and gap = 0.05 that is 1.8e-11, and the gate takes a margin of
5 over it.  Every case must therefore have gap >= MIN_GAP, which the tests assert."""
import os

import numpy as np
import torch

GATE = 1e-10
MIN_GAP = 0.05
PLOT_H, PLOT_W = 432, 576
HW_TRAJ, HW_FRAME = 0.9375, 0.5                  # 1.5 pt at 90 dpi = 1.875 px wide; the axes box 1 px
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# --------------------------------------------------------------------------------------------------
# eval_ate.py
# --------------------------------------------------------------------------------------------------
def used_mask(gt: np.ndarray, last: int) -> np.ndarray:
    """convert_poses :247-252: frame i <= last is used iff gt[i] has no inf and no nan"""
    return np.isfinite(gt[:last + 1].reshape(last + 1, 16)).all(1)


def positions(c2w: np.ndarray, scale: float) -> np.ndarray:
    """[n, 3] fp64 of fp32 poses: ``c2w[:3, 3] /= scale`` on fp32 tensors (:253), then ``float(value)`` (:146-148)"""
    t = torch.from_numpy(np.ascontiguousarray(c2w[:, :3, 3], dtype=np.float32)).clone()
    t /= scale
    return t.numpy().astype(np.float64)


def align(model: np.ndarray, data: np.ndarray):
    """eval_ate.py:44-78 on (3, n) arrays -> rot (3, 3), trans (3,), the error per point"""
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    if model.shape[1] <= 4096:
        W = np.zeros((3, 3))
        for k in range(model.shape[1]):
            W += np.outer(mz[:, k], dz[:, k])
    else:                                            # (the same sum in another order: the loop takes seconds at 2^20 points)
        W = mz @ dz.T
    U, _, Vh = np.linalg.svd(W.transpose())
    S = np.identity(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    trans = data.mean(1) - rot @ model.mean(1)
    diff = rot @ model + trans[:, None] - data
    return rot, trans, np.sqrt((diff * diff).sum(0))


def gap(model: np.ndarray, data: np.ndarray) -> float:
    """(s2 +- s3) / s1 of W: what the rotation's conditioning hangs on"""
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    W = mz @ dz.T
    s = np.linalg.svd(W, compute_uv=False)
    return float((s[1] + (s[2] if np.linalg.det(W) > 0 else -s[2])) / s[0])


def stats(e: np.ndarray) -> dict:
    """:215-223"""
    return {"rmse": np.sqrt(np.dot(e, e) / len(e)), "mean": np.mean(e), "median": np.median(e), "std": np.std(e), "min": np.min(e),
            "max": np.max(e)}


def apply(rot, trans, m):
    """rot m + trans of [n, 3] points in the kernel's association"""
    return np.stack([((rot[r, 0] * m[:, 0] + rot[r, 1] * m[:, 1]) + rot[r, 2] * m[:, 2]) + trans[r] for r in range(3)], 1)


def evaluate(est: np.ndarray, gt: np.ndarray, last: int, scale: float) -> dict:
    """What a record and an error row must hold for fp32 pose lists [n, 4, 4]"""
    use = used_mask(gt, last)
    m, d = positions(est[:last + 1][use], scale), positions(gt[:last + 1][use], scale)
    out = {"pairs": int(use.sum()), "dropped": int((~use).sum()), "model": m, "data": d}
    if out["pairs"] >= 1:
        rot, trans, e = align(m.T, d.T)
        a = apply(rot, trans, m)
        out.update(rot=rot, trans=trans, err=e, stats=stats(e), extent=float(max(np.abs(m).max(), np.abs(d).max())),
                   gap=gap(m.T, d.T) if out["pairs"] >= 3 else 0.0,
                   limits=np.array([min(a[:, 0].min(), d[:, 0].min()), max(a[:, 0].max(), d[:, 0].max()),
                                    min(a[:, 1].min(), d[:, 1].min()), max(a[:, 1].max(), d[:, 1].max())]))
    return out


def check_record(rec: np.ndarray, want: dict, err=None, what=""):
    """A record (and its error row) against ``evaluate``'s dict under the gate of the module's docstring; the case must be one the
    gate was derived for"""
    assert want["pairs"] >= 3 and want["gap"] >= MIN_GAP, (what, want["pairs"], want.get("gap"))
    assert rec[0] == want["pairs"] and rec[1] == want["dropped"] and rec[2] == 0, (what, rec[:3], want["pairs"], want["dropped"])
    assert rec[25] == (1.0 if want["pairs"] < 2 else 0.0) and (rec[26:] == 0).all(), (what, rec[25:])
    tol = GATE * max(1.0, want["extent"])
    assert np.abs(rec[9:18].reshape(3, 3) - want["rot"]).max() <= GATE, (what, "rot", np.abs(rec[9:18].reshape(3, 3) - want["rot"]).max())
    assert np.abs(rec[18:21] - want["trans"]).max() <= tol, (what, "trans", np.abs(rec[18:21] - want["trans"]).max())
    for i, k in enumerate(("rmse", "mean", "median", "std", "min", "max")):
        assert abs(rec[3 + i] - want["stats"][k]) <= tol, (what, k, rec[3 + i], want["stats"][k])
    assert np.abs(rec[21:25] - want["limits"]).max() <= tol, (what, "limits", rec[21:25], want["limits"])
    if err is not None:
        assert np.abs(err[:want["pairs"]] - want["err"]).max() <= tol, (what, "errors")
        assert np.isnan(err[want["pairs"]:]).all(), (what, "the row behind the pairs")


def check_own_statistics(rec: np.ndarray, err: np.ndarray, what=""):
    """The record's statistics against numpy's of the kernel's OWN error vector: min, max and median bit for bit, the sums to
    n eps relative"""
    n = int(rec[0])
    e = err[:n]
    s = stats(e)
    for i, k in ((2, "median"), (4, "min"), (5, "max")):
        assert np.float64(rec[3 + i]).tobytes() == np.float64(s[k]).tobytes(), (what, k, rec[3 + i], s[k])
    for i, k in ((0, "rmse"), (1, "mean"), (3, "std")):
        assert abs(rec[3 + i] - s[k]) <= n * 2.2e-16 * abs(s[k]), (what, k, rec[3 + i], s[k])


def run(E, est, gt, lasts, scale):
    """evaluate_ate on the engine's device with the error rows -> (records [B, 32], error rows [B, n], the result)"""
    from nice_slam_amd import trajeval
    res = trajeval.evaluate_ate(torch.from_numpy(est).to(E.device), torch.from_numpy(gt).to(E.device), last=lasts, scale=scale, errors=True, engine=E)
    assert res.record.device == E.device and res.errors.device == E.device and res.record.dtype == torch.float64
    return res.record.cpu().numpy(), res.errors.cpu().numpy(), res


def check_case(E, est, gt, lasts, scale, what=""):
    """Every problem of ``lasts`` under both checks"""
    rec, err, res = run(E, est, gt, lasts, scale)
    assert rec.shape == (len(lasts), 32)
    for b, last in enumerate(lasts):
        want = evaluate(est, gt, last, scale)
        check_record(rec[b], want, err[b], f"{what} last {last}")
        check_own_statistics(rec[b], err[b], f"{what} last {last}")
    return rec, err, res


def check_plot(E, est, gt, last, scale, what=""):
    """The kernel's figure is, byte for byte, the restatement's of the kernel's record"""
    from nice_slam_amd import trajeval
    e, g = torch.from_numpy(est).to(E.device), torch.from_numpy(gt).to(E.device)
    res = trajeval.evaluate_ate(e, g, last=last, scale=scale, engine=E)
    img = trajeval.plot_trajectories(e, g, res)
    assert img.device == E.device and img.dtype == torch.uint8 and tuple(img.shape) == (PLOT_H, PLOT_W, 3)
    img = img.cpu().numpy()
    want = draw(res.record[0].cpu().numpy(), est, gt, last, scale)
    assert img.tobytes() == want.tobytes(), (what, int((img != want).sum()))
    return img


# --------------------------------------------------------------------------------------------------
# the figure
# --------------------------------------------------------------------------------------------------
def view_limits(lo: float, hi: float):
    """matplotlib's autoscale of the data limits: nonsingular(expander 0.05), then 5 % of the range on each side"""
    lo, hi = np.float64(lo), np.float64(hi)
    if hi == lo:
        if lo == 0.0:
            lo, hi = np.float64(-0.05), np.float64(0.05)
        else:
            lo, hi = lo - 0.05 * abs(lo), hi + 0.05 * abs(hi)
    d = (hi - lo) * 0.05
    return lo - d, hi + d


def display(x, y, limits, H=PLOT_H, W=PLOT_W):
    """data -> pixels, x right and y DOWN (row = H - matplotlib's y), of the axes box [0.125, 0.9] x [0.11, 0.88]"""
    W, H = np.float64(W), np.float64(H)
    ax0, ax1, ay0, ay1 = 0.125 * W, 0.9 * W, 0.11 * H, 0.88 * H
    xl, yl = view_limits(limits[0], limits[1]), view_limits(limits[2], limits[3])
    with np.errstate(all="ignore"):
        kx, ky = (ax1 - ax0) / (xl[1] - xl[0]), (ay1 - ay0) / (yl[1] - yl[0])
        return ax0 + (x - xl[0]) * kx, H - (ay0 + (y - yl[0]) * ky)


def on_segment(px, py, ax, ay, bx, by, hw2):
    """the pixel rule of nsr_trajeval.h on arrays of pixel centres"""
    with np.errstate(all="ignore"):
        sx, sy, ux, uy = bx - ax, by - ay, px - ax, py - ay
        dot, len2 = ux * sx + uy * sy, sx * sx + sy * sy
        vx, vy = px - bx, py - by
        cr = ux * sy - uy * sx
        return np.where(dot <= 0.0, ux * ux + uy * uy <= hw2, np.where(dot >= len2, vx * vx + vy * vy <= hw2, cr * cr <= hw2 * len2))


def draw(rec: np.ndarray, est: np.ndarray, gt: np.ndarray, last: int, scale: float, H=PLOT_H, W=PLOT_W) -> np.ndarray:
    """u8 [H, W, 3] of a record (its rot, trans and limits) and the pose lists"""
    py, px = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing="ij")
    Wd, Hd = np.float64(W), np.float64(H)
    ax0, ax1, top, bot = 0.125 * Wd, 0.9 * Wd, Hd - 0.88 * Hd, Hd - 0.11 * Hd
    black = np.zeros((H, W), bool)
    blue = np.zeros((H, W), bool)
    for a, b in (((ax0, bot), (ax1, bot)), ((ax1, bot), (ax1, top)), ((ax1, top), (ax0, top)), ((ax0, top), (ax0, bot))):
        black |= on_segment(px, py, a[0], a[1], b[0], b[1], HW_FRAME * HW_FRAME)
    if 0 <= last < len(gt):
        use = used_mask(gt, last)
        m, d = positions(est[:last + 1][use], scale), positions(gt[:last + 1][use], scale)
        a = apply(rec[9:18].reshape(3, 3), rec[18:21], m)
        gx, gy = display(d[:, 0], d[:, 1], rec[21:25], H, W)
        ex, ey = display(a[:, 0], a[:, 1], rec[21:25], H, W)
        for k in range(1, len(m)):
            black |= on_segment(px, py, gx[k - 1], gy[k - 1], gx[k], gy[k], HW_TRAJ * HW_TRAJ)
            blue |= on_segment(px, py, ex[k - 1], ey[k - 1], ex[k], ey[k], HW_TRAJ * HW_TRAJ)
    img = np.full((H, W, 3), 255, np.uint8)
    img[black] = 0
    img[blue] = (0, 0, 255)
    return img


# --------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------
def rotation(rng) -> np.ndarray:
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] *= -1.0
    return q


def walk(n: int, seed: int, noise: float = 0.02, mirror: bool = False):
    """(est, gt) fp32 [n, 4, 4]: a random walk and a rotated, shifted, noisy copy of it (``mirror``: reflected as well, so that
    the alignment takes the det < 0 branch)"""
    rng = np.random.RandomState(seed)
    p = np.cumsum(rng.randn(n, 3) * 0.25, 0) + rng.randn(3)
    R = rotation(rng)
    q = p @ R.T + rng.randn(3) + rng.randn(n, 3) * noise
    if mirror:
        q[:, 2] *= -1.0
    est = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    gt = est.copy()
    for i in range(n):
        gt[i, :3, :3] = rotation(rng)
        est[i, :3, :3] = gt[i, :3, :3]
    gt[:, :3, 3] = p
    est[:, :3, 3] = q
    return est, gt


SIZES = (3, 5, 63, 64, 65, 255, 256, 257, 1000)


def sized_case(n: int, masked: bool = False):
    """(est, gt) of n frames; ``masked``: the first, the last and an interior ground-truth pose are inf / nan (n >= 6)"""
    est, gt = walk(n, 1000 + n)
    if masked:
        gt[0, 1, 2] = np.inf
        gt[n - 1, 3, 3] = np.nan
        gt[n // 2, 0, 3] = -np.inf
    return est, gt


def tied_case(n: int = 64):
    """every second frame repeats the one before it, in both lists: the errors come in exactly equal pairs"""
    est, gt = walk(n, 77)
    est[1::2], gt[1::2] = est[0::2], gt[0::2]
    return est, gt


def golden_cases():
    """The three pose sets of tests/golden/trajeval.npz: name -> (est, gt, last, scale)"""
    a = walk(12, 5)
    b = walk(65, 6)
    b[1][0, 0, 0] = np.inf
    b[1][17, 2, 3] = np.nan
    b[1][64, 1, 1] = -np.inf
    c = walk(60, 8, noise=0.3, mirror=True)
    return {"plain12": (a[0], a[1], 11, 1.0), "masked65": (b[0], b[1], 64, 0.37), "mirror60": (c[0], c[1], 59, 1.0)}


def golden():
    z = np.load(os.path.join(GOLDEN, "trajeval.npz"))
    return {k: z[k] for k in z.files}


def ate_golden_cases():
    """The committed tests/golden/ate_golden.npz (the reference's own align on fp64 points): name -> (est (3, n), gt, rot, trans, err)"""
    z = np.load(os.path.join(GOLDEN, "ate_golden.npz"))
    return {f"c{k}": tuple(z[f"c{k}/{f}"] for f in ("est", "gt", "rot", "trans", "err")) for k in range(4)}


def poses_of(points: np.ndarray) -> np.ndarray:
    """fp32 [n, 4, 4] poses with the translations ``points`` (3, n)"""
    out = np.tile(np.eye(4, dtype=np.float32), (points.shape[1], 1, 1))
    out[:, :3, 3] = points.T
    return out
