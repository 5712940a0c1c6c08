"""TEST INFRASTRUCTURE: the rendering-evaluation metrics of nice_slam_amd.imgeval restated from their definitions, independently
of the kernel (nice_slam_amd/csrc/nsr_imgmetrics.h): fp64 throughout, the Gaussian window as an outer product, the moments by
``torch.nn.functional.conv2d`` without padding, the residuals in numpy after src/utils/Visualizer.py:62-65.  Also the test
images the emulator and the GPU tests share, and the bounds both hold the kernel to."""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2

# Bounds on |kernel - restatement|: 4 x the largest deviation the emulator showed over the cases of tests/test_imgmetrics_emu.py
# (measured: DESIGN.md 3.12).  The sums are fp64 sums of exact fp64 terms in another order; the SSIM carries the fp32 window
# moments (121 terms each).
MEASURED_SUM_REL = 2.2e-16
MEASURED_SSIM_ABS = 2.92e-7
BOUND_SUM_REL = 4 * MEASURED_SUM_REL
BOUND_SSIM_ABS = 4 * MEASURED_SSIM_ABS


# (B, H, W, seed, frame without input depth) of make_images: the cases the deviations were measured over.  37 x 53: 27 x 43 window
# positions, two tiles of 32 with ragged edges; 47 x 75: 37 x 65, two by three tiles; one window; one row / column of windows; the GPU test's 120 x 160 (4 x 5 tiles)
CASES = ((3, 37, 53, 0, 2), (2, 47, 75, 4, None), (1, 11, 11, 1, None), (2, 11, 64, 2, None), (2, 64, 11, 3, None), (1, 120, 160, 5, None))


def gaussian_window():
    x = torch.arange(WIN, dtype=torch.float64) - WIN // 2
    g = torch.exp(-(x ** 2) / (2 * SIGMA ** 2))
    g = g / g.sum()
    return torch.outer(g, g)


def ssim(a, b):
    """a, b [H, W, 3], any float dtype: the mean SSIM of the clipped images over the valid windows and the channels (fp64)"""
    x = torch.as_tensor(np.asarray(a, dtype=np.float64)).clamp(0.0, 1.0).permute(2, 0, 1)[:, None]      # [3, 1, H, W]
    y = torch.as_tensor(np.asarray(b, dtype=np.float64)).clamp(0.0, 1.0).permute(2, 0, 1)[:, None]
    w = gaussian_window()[None, None]
    mx, my = F.conv2d(x, w), F.conv2d(y, w)
    vx = F.conv2d(x * x, w) - mx * mx
    vy = F.conv2d(y * y, w) - my * my
    vxy = F.conv2d(x * y, w) - mx * my
    m = ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return float(m.mean())


def residuals(color, gt_color, depth, gt_depth):
    """Visualizer.py:62-65 on fp32 arrays: (depth_residual, color_residual)"""
    gt_depth_np, gt_color_np = np.asarray(gt_depth, np.float32), np.asarray(gt_color, np.float32)
    depth_np, color_np = np.asarray(depth, np.float32), np.asarray(color, np.float32)
    depth_residual = np.abs(gt_depth_np - depth_np)
    depth_residual[gt_depth_np == 0.0] = 0.0
    color_residual = np.abs(gt_color_np - color_np)
    color_residual[gt_depth_np == 0.0] = 0.0
    return depth_residual, color_residual


def frame_metrics(color, gt_color, depth, gt_depth):
    """one frame (fp32 arrays, as the kernel reads them) -> dict of the raw sums, counts and metrics in fp64"""
    a = np.clip(np.asarray(color, np.float32).astype(np.float64), 0.0, 1.0)
    b = np.clip(np.asarray(gt_color, np.float32).astype(np.float64), 0.0, 1.0)
    d, g = np.asarray(depth, np.float32).astype(np.float64), np.asarray(gt_depth, np.float32).astype(np.float64)
    valid = g != 0.0
    sq = (a - b) ** 2
    se_all, se_valid = float(sq.sum()), float(sq[valid].sum())
    n_all, n_valid = int(valid.size), int(valid.sum())
    l1 = float(np.abs(g - d)[valid].sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = float(-10.0 * np.log10(np.float64(se_all) / (3.0 * n_all)))
        psnr_valid = float(-10.0 * np.log10(np.float64(se_valid) / np.float64(3.0 * n_valid)))
        depth_l1_cm = float(100.0 * np.float64(l1) / np.float64(n_valid))
    return {"se_all": se_all, "se_valid": se_valid, "n_all": n_all, "n_valid": n_valid, "l1": l1, "psnr": psnr, "psnr_valid": psnr_valid,
            "depth_l1_cm": depth_l1_cm, "ssim": ssim(color, gt_color), "depth_max": float(np.asarray(gt_depth, np.float32).max())}


def batch_metrics(color, gt_color, depth, gt_depth):
    return [frame_metrics(color[k], gt_color[k], depth[k], gt_depth[k]) for k in range(len(depth))]


def make_images(B, H, W, seed=0, zero_frame=None):
    """(color, gt_color, depth, gt_depth) fp32: smooth images with structure (a gradient, a few sinusoids, seeded noise), values
    a little outside [0, 1], an input depth with a band of zeros; frame ``zero_frame``'s input depth is all zero"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    gt_color = np.zeros((B, H, W, 3))
    for k in range(B):
        for c in range(3):
            f = rng.uniform(1.0, 6.0, size=4)
            ph = rng.uniform(0.0, 2 * np.pi, size=2)
            gt_color[k, ..., c] = (0.5 + 0.45 * (x - 0.5) * np.cos(0.7 * c + k) + 0.35 * (y - 0.5) + 0.18 * np.sin(2 * np.pi * f[0] * x + ph[0])
                                   * np.cos(2 * np.pi * f[1] * y + ph[1]) + 0.12 * np.sin(2 * np.pi * (f[2] * x + f[3] * y)))
    gt_color = 1.15 * (gt_color - 0.5) + 0.5 + rng.normal(scale=0.01, size=gt_color.shape)
    color = gt_color + 0.05 * np.sin(2 * np.pi * 3 * x)[None, ..., None] + rng.normal(scale=0.03, size=gt_color.shape)
    gt_depth = 2.0 + 1.5 * x[None] + 0.8 * np.sin(2 * np.pi * y)[None] + rng.uniform(0.0, 0.3, size=(B, 1, 1))
    gt_depth = np.repeat(gt_depth, 1, axis=0)
    gt_depth[:, H // 3:H // 3 + max(H // 8, 1), :] = 0.0                    # a band without depth
    gt_depth[:, :, W - 3:] = 0.0                                            # and the image's right edge
    depth = np.abs(gt_depth + rng.normal(scale=0.05, size=gt_depth.shape)) + 0.01
    if zero_frame is not None:
        gt_depth[zero_frame] = 0.0
    return (color.astype(np.float32), gt_color.astype(np.float32), depth.astype(np.float32), gt_depth.astype(np.float32))


EXACT = ("psnr", "psnr_valid", "ssim", "depth_l1_cm", "n_valid", "depth_max", "sq_err", "sq_err_valid", "depth_abs_err")
# PSNR and the depth L1 in cm are one log10 / one division of sums inside BOUND_SUM_REL: d psnr = 10 / ln 10 x the relative
# deviation, plus the rounding of two log10 evaluations and a product of values below 128 (2^-46 an ulp): 8 ulp allowed
PSNR_ABS = 10.0 / math.log(10.0) * BOUND_SUM_REL + 8 * 2.0 ** -46


def check_against_reference(imgs, got, ref, deviations=None):
    for k, r in enumerate(ref):
        assert int(got["n_valid"][k]) == r["n_valid"]
        assert float(got["depth_max"][k]) == r["depth_max"]
        for key, want in (("sq_err", r["se_all"]), ("sq_err_valid", r["se_valid"]), ("depth_abs_err", r["l1"])):
            dev = abs(float(got[key][k]) - want) / want if want != 0.0 else abs(float(got[key][k]))
            print(f"frame {k} {key}: relative deviation {dev:.3e} (bound {BOUND_SUM_REL:.3e})")
            assert dev <= BOUND_SUM_REL, (k, key)
        dev = abs(float(got["ssim"][k]) - r["ssim"])
        print(f"frame {k} ssim: {float(got['ssim'][k]):.9f}, deviation {dev:.3e} (bound {BOUND_SSIM_ABS:.3e})")
        assert dev <= BOUND_SSIM_ABS, k
        for key in ("psnr", "psnr_valid", "depth_l1_cm"):
            g, w = float(got[key][k]), r[key]
            if math.isnan(w):
                assert math.isnan(g), (k, key)
            elif key == "depth_l1_cm":
                assert abs(g - w) <= (BOUND_SUM_REL + 2.0 ** -51) * w, (k, key)
            else:
                assert abs(g - w) <= PSNR_ABS, (k, key)
        if "depth_residual" in got:
            dr, cr = residuals(imgs[0][k], imgs[1][k], imgs[2][k], imgs[3][k])
            assert np.array_equal(got["depth_residual"][k].numpy(), dr)
            assert np.array_equal(got["color_residual"][k].numpy(), cr)
