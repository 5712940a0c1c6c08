"""TEST INFRASTRUCTURE: the figure of nice_slam_amd.imgeval.figure_sheet restated in numpy from its contract
(nice_slam_amd/csrc/nsr_figure.h), operation for operation in fp32 -- every step there is ONE fp32 operation, so the bytes must be
the same, and the tests compare without a tolerance.  The colour map is read from the fixture tests/golden/plasma_lut.npy
(tests/golden/make_golden_plasma.py mints it from matplotlib), not from the header.  Also the inputs the emulator and the GPU
tests share."""
import os

import numpy as np

from imgmetrics_reference import residuals

LUT = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plasma_lut.npy"))
assert LUT.shape == (256, 3) and LUT.dtype == np.uint8

F32 = np.float32
# (stride, margin, gap) of the byte-for-byte cases, and the images beside the main 3 x 37 x 53 batch
LAYOUTS = ((1, 8, 8), (3, 0, 0), (2, 5, 3))
SMALL = ((1, 1), (11, 4))


def fold_max(g):
    """fmaxf over all pixels from -inf: a NaN does not win"""
    return np.fmax.reduce(np.asarray(g, F32).reshape(-1), initial=F32(-np.inf)).astype(F32)


def colormap(v, vmax):
    """u8 [..., 3] of fp32 values: white for a NaN; index 0 if vmax == 0, else with t = v / vmax (fp32): 255 if t >= 1,
    (int)(t * 256) if 0 < t < 1, else 0"""
    v, vmax = np.asarray(v, F32), F32(vmax)
    idx = np.zeros(v.shape, np.int64)
    if vmax != 0:
        with np.errstate(all="ignore"):
            t = (v / vmax).astype(F32)
            inside = (t > 0) & (t < 1)
            idx = np.where(t >= 1, 255, (np.where(inside, t, F32(0)) * F32(256)).astype(F32).astype(np.int64))
    out = LUT[idx]
    out[np.isnan(v)] = 255
    return out


def rgb_bytes(v):
    """(uint8)(fminf(fmaxf(v, 0), 1) * 255.0f): a NaN gives 0"""
    c = np.fmin(np.fmax(np.asarray(v, F32), F32(0)), F32(1))
    return (c * F32(255)).astype(F32).astype(np.uint8)


def sheet_size(H, W, stride, margin, gap):
    h, w = -(-H // stride), -(-W // stride)
    return 2 * margin + 2 * h + gap, 2 * margin + 3 * w + 2 * gap


def panels(color, gt_color, depth, gt_depth):
    """one frame -> (vmax, [[g, d, depth residual], [b, a, colour residual]]) as u8 [H, W, 3] images at full size"""
    color, gt_color, depth, gt_depth = (np.asarray(x, F32) for x in (color, gt_color, depth, gt_depth))
    vmax = fold_max(gt_depth)
    with np.errstate(all="ignore"):
        dres, cres = residuals(color, gt_color, depth, gt_depth)
    return vmax, [[colormap(gt_depth, vmax), colormap(depth, vmax), colormap(dres, vmax)],
                  [rgb_bytes(gt_color), rgb_bytes(color), rgb_bytes(cres)]]


def expected_sheet(color, gt_color, depth, gt_depth, stride=1, margin=8, gap=8):
    """u8 [B, SH, SW, 3] (inputs [B, H, W(, 3)]) and the [B] fp32 maxima"""
    B, H, W = np.asarray(depth).shape
    h, w = -(-H // stride), -(-W // stride)
    SH, SW = sheet_size(H, W, stride, margin, gap)
    out = np.full((B, SH, SW, 3), 255, np.uint8)
    vmaxes = np.zeros(B, F32)
    for k in range(B):
        vmaxes[k], rows = panels(color[k], gt_color[k], depth[k], gt_depth[k])
        for r in range(2):
            for c in range(3):
                y0, x0 = margin + r * (h + gap), margin + c * (w + gap)
                out[k, y0:y0 + h, x0:x0 + w] = rows[r][c][::stride, ::stride]
    return out, vmaxes


def panel_mask(H, W, stride, margin, gap):
    """bool [SH, SW]: the pixels that belong to one of the six panels"""
    h, w = -(-H // stride), -(-W // stride)
    SH, SW = sheet_size(H, W, stride, margin, gap)
    m = np.zeros((SH, SW), bool)
    for r in range(2):
        for c in range(3):
            m[margin + r * (h + gap):margin + r * (h + gap) + h, margin + c * (w + gap):margin + c * (w + gap) + w] = True
    return m


def make_images(B, H, W, seed=0):
    """(color, gt_color, depth, gt_depth) fp32 random images: colours in [0, 1], depths in [0.5, 4], about 20 % of the input
    depth 0"""
    rng = np.random.default_rng(seed)
    gt_color = rng.uniform(0.0, 1.0, size=(B, H, W, 3))
    color = np.clip(gt_color + rng.normal(scale=0.1, size=gt_color.shape), 0.0, 1.0)
    gt_depth = rng.uniform(0.5, 4.0, size=(B, H, W))
    depth = np.abs(gt_depth + rng.normal(scale=0.3, size=gt_depth.shape))
    gt_depth[rng.uniform(size=gt_depth.shape) < 0.2] = 0.0
    return color.astype(F32), gt_color.astype(F32), depth.astype(F32), gt_depth.astype(F32)


def main_case(H=37, W=53, seed=0):
    """Three frames: 0 with about 20 % zero input depth; 1 with an all-zero input depth (vmax = 0); 2 whose rendered depth holds
    a NaN, a +inf, values above vmax and negative values, and whose colours leave [0, 1] on both sides"""
    color, gt_color, depth, gt_depth = make_images(3, H, W, seed)
    gt_depth[1] = 0.0
    rng = np.random.default_rng(seed + 100)
    d = depth[2].reshape(-1)
    pick = rng.permutation(d.size)
    d[pick[0]] = np.nan
    d[pick[1]] = np.inf
    d[pick[2:2 + d.size // 10]] = gt_depth[2].max() * rng.uniform(1.0, 3.0, size=d.size // 10).astype(F32)
    d[pick[2 + d.size // 10:2 + d.size // 5]] *= -1.0
    color[2] = 1.6 * color[2] - 0.3
    gt_color[2] = 1.4 * gt_color[2] - 0.2
    return color, gt_color, depth, gt_depth


def assert_main_case_holds_its_cases(imgs):
    color, gt_color, depth, gt_depth = imgs
    z0 = (gt_depth[0] == 0).mean()
    assert 0.1 < z0 < 0.3 and not gt_depth[1].any() and fold_max(gt_depth[1]) == 0
    vmax = fold_max(gt_depth[2])
    assert np.isnan(depth[2]).sum() == 1 and np.isposinf(depth[2]).sum() == 1
    finite = np.isfinite(depth[2])
    assert (depth[2][finite] > vmax).any() and (depth[2] < 0).any()
    assert color[2].min() < 0 and color[2].max() > 1 and gt_color[2].min() < 0 and gt_color[2].max() > 1
    assert (gt_depth[2] == vmax).any()                                     # t = 1 exactly occurs: the input's own maximum
