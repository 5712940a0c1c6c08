"""CPU tests of the rendering evaluation (nice_slam_amd/csrc/nsr_imgmetrics.h, nice_slam_amd/imgeval.py): the kernel sources run
on the emulator against the fp64 restatement (tests/imgmetrics_reference.py) -- counts, maxima and residual maps exactly, the
sums and the SSIM within the bounds derived there -- then the properties that do not need a reference (batch independence,
repeatability, identical and constant images, frames without depth), the input conversions, the ABI's error paths, the command
line and evaluate_rendering over a stub renderer."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import emu_harness
import imgmetrics_reference as R
from nice_slam_amd import imgeval
from nice_slam_amd.engine import Engine

EXACT, check_against_reference = R.EXACT, R.check_against_reference


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def main_case(E):
    imgs = R.make_images(*R.CASES[0])
    return imgs, imgeval.image_metrics(*imgs, residuals=True, engine=E), R.batch_metrics(*imgs)


def same_bits(a, b, keys=EXACT):
    return all(a[k].numpy().tobytes() == b[k].numpy().tobytes() for k in keys)


def test_bounds_are_what_was_measured():
    assert R.BOUND_SUM_REL == 4 * R.MEASURED_SUM_REL and R.BOUND_SSIM_ABS == 4 * R.MEASURED_SSIM_ABS
    assert R.BOUND_SSIM_ABS <= 1e-5                  # above that the moment arithmetic is at fault, not the tolerance


def test_main_case_matches_restatement(main_case):
    imgs, got, ref = main_case
    color, gt_color, depth, gt_depth = imgs
    assert color.max() > 1.0 and color.min() < 0.0 and gt_color.max() > 1.0         # the clip matters
    assert (gt_depth[0] == 0).any() and (gt_depth[0] != 0).any() and not gt_depth[2].any()
    check_against_reference(imgs, got, ref)
    assert int(got["n_valid"][2]) == 0 and math.isnan(float(got["depth_l1_cm"][2])) and math.isnan(float(got["psnr_valid"][2]))
    assert float(got["depth_abs_err"][2]) == 0.0 and math.isfinite(float(got["psnr"][2]))
    assert not got["depth_residual"][2].any() and not got["color_residual"][2].any()


@pytest.mark.parametrize("case", R.CASES[1:], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_sizes_match_restatement(E, case):
    imgs = R.make_images(*case)
    got = imgeval.image_metrics(*imgs, residuals=True, engine=E)
    check_against_reference(imgs, got, R.batch_metrics(*imgs))


def test_one_window(E):
    color, gt_color, depth, gt_depth = (x[0] for x in R.make_images(*R.CASES[2]))
    got = imgeval.image_metrics(color, gt_color, depth, gt_depth, engine=E)
    assert got["ssim"].dim() == 0                                                  # one frame in, scalars out
    x, y = np.clip(color.astype(np.float64), 0, 1), np.clip(gt_color.astype(np.float64), 0, 1)
    w = R.gaussian_window().numpy()
    vals = []
    for c in range(3):                                                             # the one window per channel, written out
        mx, my = (w * x[..., c]).sum(), (w * y[..., c]).sum()
        vx, vy, vxy = (w * x[..., c] ** 2).sum() - mx * mx, (w * y[..., c] ** 2).sum() - my * my, (w * x[..., c] * y[..., c]).sum() - mx * my
        vals.append((2 * mx * my + R.C1) * (2 * vxy + R.C2) / ((mx * mx + my * my + R.C1) * (vx + vy + R.C2)))
    assert abs(float(got["ssim"]) - np.mean(vals)) <= R.BOUND_SSIM_ABS


def test_frame_alone_equals_frame_in_batch(E, main_case):
    imgs, got, _ = main_case
    for k in range(3):
        one = imgeval.image_metrics(*(x[k] for x in imgs), residuals=True, engine=E)
        for key in EXACT + ("depth_residual", "color_residual"):
            assert one[key].numpy().tobytes() == got[key][k].numpy().tobytes(), (k, key)


def test_batch_order_does_not_leak(E, main_case):
    imgs, got, _ = main_case
    perm = [2, 0, 1]
    shuffled = imgeval.image_metrics(*(x[perm] for x in imgs), residuals=True, engine=E)
    for key in EXACT + ("depth_residual", "color_residual"):
        assert shuffled[key].numpy().tobytes() == got[key][perm].contiguous().numpy().tobytes(), key


def test_two_runs_are_bit_identical(E, main_case):
    imgs, got, _ = main_case
    again = imgeval.image_metrics(*imgs, residuals=True, engine=E)
    assert same_bits(got, again, EXACT + ("depth_residual", "color_residual"))


def test_residual_pointers_do_not_change_the_metrics(E, main_case):
    imgs, got, _ = main_case
    assert same_bits(got, imgeval.image_metrics(*imgs, residuals=False, engine=E))


def test_identical_images(E):
    color, _, depth, gt_depth = R.make_images(2, 37, 53, seed=7)
    got = imgeval.image_metrics(color, color.copy(), depth, gt_depth, engine=E)
    assert got["ssim"].tolist() == [1.0, 1.0]
    assert got["sq_err"].tolist() == [0.0, 0.0] and got["psnr"].tolist() == [math.inf, math.inf]
    assert got["psnr_valid"].tolist() == [math.inf, math.inf]


def test_constant_images(E):
    H, W = 37, 53
    color = np.full((2, H, W, 3), 0.25, np.float32)
    gt_color = np.full((2, H, W, 3), 0.75, np.float32)
    gt_color[1] = 1.5                                                              # clipped to 1
    depth, gt_depth = np.full((2, H, W), 2.0, np.float32), np.full((2, H, W), 2.5, np.float32)
    got = imgeval.image_metrics(color, gt_color, depth, gt_depth, engine=E)
    for k, b in enumerate((0.75, 1.0)):
        want = (2 * 0.25 * b + R.C1) * R.C2 / ((0.25 ** 2 + b ** 2 + R.C1) * R.C2)      # no variance: the luminance term alone
        assert abs(float(got["ssim"][k]) - want) <= R.BOUND_SSIM_ABS
        assert abs(float(got["sq_err"][k]) - 3 * H * W * (b - 0.25) ** 2) <= R.BOUND_SUM_REL * 3 * H * W * (b - 0.25) ** 2
    assert got["depth_l1_cm"].tolist() == [50.0, 50.0] and got["n_valid"].tolist() == [H * W, H * W]
    assert got["depth_max"].tolist() == [2.5, 2.5]


def test_fp64_and_strided_inputs(E, main_case):
    imgs, got, _ = main_case
    as64 = imgeval.image_metrics(*(torch.from_numpy(x).double() for x in imgs), engine=E)
    assert same_bits(got, as64)
    wide = [np.zeros(x.shape[:2] + (2 * x.shape[2],) + x.shape[3:], np.float32) for x in imgs]
    for w, x in zip(wide, imgs):
        w[:, :, ::2] = x
    strided = [torch.from_numpy(w)[:, :, ::2] for w in wide]
    assert not strided[0].is_contiguous()
    assert same_bits(got, imgeval.image_metrics(*strided, engine=E))


def test_abi_error_paths(E):
    lib = E.lib
    color, gt_color, depth, gt_depth = R.make_images(1, 16, 16, seed=3)
    res = np.zeros(8)
    n = lib.nsr_image_metrics_workspace_bytes(1, 16, 16)
    assert n == 8 * 6 * 1 and lib.nsr_image_metrics_workspace_bytes(3, 37, 53) == 8 * 6 * 3 * 2
    assert lib.nsr_image_metrics_workspace_bytes(1, 10, 16) == -1 and lib.nsr_image_metrics_workspace_bytes(-1, 16, 16) == -1
    assert lib.nsr_image_metrics_workspace_bytes(0, 16, 16) == 0
    ws = np.zeros(n, np.uint8)
    p = emu_harness.ptr

    def call(c=color, g=gt_color, d=depth, gd=gt_depth, B=1, H=16, W=16, r=res, w=ws, nbytes=n):
        return lib.nsr_image_metrics(p(c), p(g), p(d), p(gd), B, H, W, p(r), None, None, p(w), nbytes, None)

    assert call() == 0
    assert call(H=10) != 0 and b"11 x 11" in lib.nsr_last_error()
    assert call(W=10) != 0 and b"11 x 11" in lib.nsr_last_error()
    assert call(nbytes=n - 1) != 0 and b"workspace" in lib.nsr_last_error()
    assert call(B=-1) != 0 and b"negative" in lib.nsr_last_error()
    for kw in ({"c": None}, {"g": None}, {"d": None}, {"gd": None}, {"r": None}, {"w": None}):
        assert call(**kw) != 0 and b"null" in lib.nsr_last_error(), kw
    before = res.copy()
    assert call(B=0) == 0 and call(B=0, c=None, w=None, nbytes=0) == 0 and np.array_equal(res, before)
    with pytest.raises(Exception):
        imgeval.image_metrics(color[:, :10], gt_color[:, :10], depth[:, :10], gt_depth[:, :10], engine=E)
    with pytest.raises(ValueError):
        imgeval.image_metrics(color, gt_color, depth[:, :12], gt_depth, engine=E)


def test_command_line(E, main_case, tmp_path, capsys):
    imgs, got, _ = main_case
    np.savez(tmp_path / "rendered.npz", color=imgs[0], depth=imgs[2])
    np.savez(tmp_path / "gt.npz", color=imgs[1], depth=imgs[3])
    assert imgeval.main([str(tmp_path / "rendered.npz"), str(tmp_path / "gt.npz")], engine=E) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["PSNR", "SSIM", "Depth L1"]
    vals = [float(ln.split(":")[1]) for ln in lines]
    assert vals[0] == math.fsum(got["psnr"].tolist()) / 3 and vals[1] == math.fsum(got["ssim"].tolist()) / 3
    assert vals[2] == math.fsum(got["depth_l1_cm"][:2].tolist()) / 2               # the frame without depth is left out


class StubRenderer:
    """render_img returns the prepared images of the frame whose index the pose carries in its translation's x"""

    def __init__(self, color, depth):
        self.color, self.depth, self.calls = color, depth, []

    def render_img(self, c, decoders, c2w, device, stage, gt_depth=None):
        assert tuple(c2w.shape) == (4, 4) and gt_depth is not None and c2w[3].tolist() == [0.0, 0.0, 0.0, 1.0]
        k = int(round(float(c2w[0, 3])))
        self.calls.append((k, stage, device))
        return torch.from_numpy(self.depth[k]).double(), None, torch.from_numpy(self.color[k])


def test_evaluate_rendering_with_a_stub_renderer(E, main_case, monkeypatch):
    imgs, got, _ = main_case
    color, gt_color, depth, gt_depth = imgs

    def camera(t):                                   # [R | T] of (quaternion, translation): identity rotations only here
        assert t.shape == (7,) and t[:4].tolist() == [1.0, 0.0, 0.0, 0.0]
        return torch.cat([torch.eye(3), t[4:, None]], 1)

    monkeypatch.setattr(imgeval, "get_camera_from_tensor", camera)
    launches = []
    real = imgeval.image_metrics
    monkeypatch.setattr(imgeval, "image_metrics", lambda *a, **k: launches.append(len(a[0])) or real(*a, **k))
    frames = []
    for k in range(3):
        c2w = torch.eye(4)
        c2w[0, 3] = k
        pose = c2w if k != 1 else torch.tensor([1.0, 0, 0, 0, k, 0, 0])          # frame 1: the camera-tensor branch
        frames.append((10 * k, torch.from_numpy(gt_color[k]), torch.from_numpy(gt_depth[k]), pose))
    stub = StubRenderer(color, depth)
    out = imgeval.evaluate_rendering(stub, None, None, frames, stage="color", device="cpu", batch=2, residuals=True, engine=E)
    assert stub.calls == [(0, "color", "cpu"), (1, "color", "cpu"), (2, "color", "cpu")]
    assert launches == [2, 1]                                                      # two frames a launch, then the rest
    assert out["n_frames"] == 3 and out["n_no_depth"] == 1 and [r["idx"] for r in out["frames"]] == [0, 10, 20]
    for k, row in enumerate(out["frames"]):
        for key in ("psnr", "ssim"):
            assert row[key] == float(got[key][k]), (k, key)
        assert row["n_valid"] == int(got["n_valid"][k]) and row["depth_max"] == float(got["depth_max"][k])
        assert np.array_equal(row["depth_residual"].numpy(), got["depth_residual"][k].numpy())
        assert np.array_equal(row["color_residual"].numpy(), got["color_residual"][k].numpy())
    assert math.isnan(out["frames"][2]["depth_l1_cm"]) and math.isnan(out["frames"][2]["psnr_valid"])
    assert out["mean"]["psnr"] == math.fsum(got["psnr"].tolist()) / 3
    assert out["mean"]["ssim"] == math.fsum(got["ssim"].tolist()) / 3
    assert out["mean"]["depth_l1_cm"] == math.fsum(got["depth_l1_cm"][:2].tolist()) / 2
    assert out["mean"]["psnr_valid"] == math.fsum(got["psnr_valid"][:2].tolist()) / 2
