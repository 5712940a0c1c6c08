"""GPU tests of the rendering evaluation (nice_slam_amd/csrc/nsr_imgmetrics.h, nice_slam_amd/imgeval.py): the emulator test's
batches against the fp64 restatement (tests/imgmetrics_reference.py) within the same bounds, repeat runs bit for bit, a batch
with more blocks in flight than the device has CUs, and evaluate_rendering end to end on the small scene rendered by
render_img at its own pose."""
import numpy as np
import pytest
import torch

import imgmetrics_reference as R
from nice_slam_amd import imgeval

EXACT, check_against_reference = R.EXACT, R.check_against_reference

pytestmark = pytest.mark.gpu


def on_host(m):
    return {k: v.cpu() for k, v in m.items()}


@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2]], ids=["3x37x53", "1x11x11"])
def test_batches_match_restatement(case):
    imgs = R.make_images(*case)
    got = on_host(imgeval.image_metrics(*imgs, residuals=True))
    check_against_reference(imgs, got, R.batch_metrics(*imgs))
    again = on_host(imgeval.image_metrics(*imgs, residuals=True))
    for key in EXACT + ("depth_residual", "color_residual"):
        assert got[key].numpy().tobytes() == again[key].numpy().tobytes(), key


def test_many_blocks_in_flight():
    imgs = R.make_images(4, 120, 160, seed=11, zero_frame=1)          # 4 x 20 tiles, 71 KB of LDS each
    dev = [torch.from_numpy(x).cuda() for x in imgs]
    got = on_host(imgeval.image_metrics(*dev, residuals=True))
    check_against_reference(imgs, got, R.batch_metrics(*imgs))
    wide = on_host(imgeval.image_metrics(*(torch.cat([x] * 40) for x in dev)))          # 3200 blocks: every CU several times over
    for key in EXACT:
        assert wide[key].reshape(40, 4).numpy().tobytes() == got[key].repeat(40, 1).numpy().tobytes(), key


def test_evaluate_rendering_end_to_end():
    from scene_util import make_scene, build_product
    sc = make_scene(seed=6, small=True)
    renderer, dec, grids = build_product(sc, "cuda:0")
    gt_color, gt_depth = sc["color_img"].cuda(), sc["depth_img"].cuda()
    assert (gt_depth == 0).any()
    frames = [(0, gt_color, gt_depth, sc["c2w"].cuda()), (1, gt_color, torch.zeros_like(gt_depth), sc["c2w"].cuda())]
    out = imgeval.evaluate_rendering(renderer, grids, dec, frames, stage="color", device="cuda:0", residuals=True)
    assert out["n_frames"] == 2 and out["n_no_depth"] == 1
    rows = out["frames"]
    imgs = [np.stack([r[k].cpu().numpy() for r in rows]) for k in ("color", "depth")]
    imgs = (imgs[0], np.stack([gt_color.cpu().numpy()] * 2), imgs[1], np.stack([gt_depth.cpu().numpy(), np.zeros(gt_depth.shape, np.float32)]))
    assert imgs[0].dtype == np.float32 and imgs[2].dtype == np.float32 and np.isfinite(imgs[0]).all() and np.isfinite(imgs[2]).all()
    got = {k: torch.tensor([r[k] for r in rows], dtype=torch.float64) for k in ("psnr", "psnr_valid", "ssim", "depth_l1_cm", "n_valid", "depth_max")}
    again = on_host(imgeval.image_metrics(*imgs, residuals=True))          # the raw sums and residual maps of the same images
    for k in ("psnr", "ssim", "n_valid", "depth_max"):
        assert got[k].tolist() == again[k].double().tolist(), k
    got.update({k: again[k] for k in ("sq_err", "sq_err_valid", "depth_abs_err")})
    got["depth_residual"] = torch.stack([r["depth_residual"].cpu() for r in rows])
    got["color_residual"] = torch.stack([r["color_residual"].cpu() for r in rows])
    check_against_reference(imgs, got, R.batch_metrics(*imgs))
    assert np.isfinite(out["mean"]["depth_l1_cm"]) and out["mean"]["depth_l1_cm"] == rows[0]["depth_l1_cm"]
    assert out["mean"]["psnr"] == (rows[0]["psnr"] + rows[1]["psnr"]) / 2
