"""Trajectory evaluation on the device (csrc/nsr_trajeval.h): src/tools/eval_ate.py.

evaluate_ate       : convert_poses' mask and scale (:239-256), align (:44-78) and the statistics (:215-223) of B problems in one launch
ate_curve          : the same at many checkpoints / prefixes of one run
plot_trajectories  : eval_ate_plot.png (:196-204, :213) as bytes on the device; save_plot writes them
python -m nice_slam_amd.trajeval CONFIG [--output DIR] [--curve]      the script's command line (:264-301)

The poses never leave the device: a problem's numbers are one record of 32 doubles there (include/nsr.h), read back only by
``AteResult.dict``.  Everything goes through an ``Engine``: the product's on the GPU, or one on the emulator library in the CPU tests.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, gpu

__all__ = ["AteResult", "evaluate_ate", "ate_curve", "plot_trajectories", "save_plot", "REC", "PLOT_H", "PLOT_W"]

REC = 32                            # doubles per record (nsr::kAteRec)
PLOT_H, PLOT_W = 432, 576           # 4.8 x 6.4 in at the 90 dpi of eval_ate.py:213
FLAG_FEW, FLAG_RANGE, FLAG_BAD_EST = 1, 2, 4
# eval_ate.py:140-143 (the message continues over a line break inside the literal)
NO_PAIRS = "Couldn't find matching timestamp pairs between groundtruth and estimated trajectory! " + " " * 12 + "Did you choose the correct sequence?"
_STATS = ("rmse", "mean", "median", "std", "min", "max")


def _poses(E: Engine, c2w) -> torch.Tensor:
    if isinstance(c2w, (list, tuple)):
        c2w = torch.stack([p if isinstance(p, torch.Tensor) else torch.from_numpy(np.asarray(p)) for p in c2w])
    t = c2w if isinstance(c2w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c2w))
    if t.dim() != 3 or tuple(t.shape[1:]) != (4, 4) or t.shape[0] < 1:
        raise _capi.NsrError(f"trajeval: poses are [n, 4, 4] with n >= 1 (got {tuple(t.shape)})")
    return t.detach().to(E.device, torch.float32).contiguous()


def _launch(E: Engine, est, gt, last, scale, rec, err=None):
    with torch.no_grad(), E.guard():
        E.call("nsr_ate_eval", est.data_ptr(), gt.data_ptr(), est.shape[0], last.data_ptr(), last.numel(), float(scale), rec.data_ptr(),
               err.data_ptr() if err is not None else None)


class AteResult:
    """B evaluations.  ``record`` fp64 [B, 32] (the layout of include/nsr.h), ``last`` int64 [B], ``errors`` fp64 [B, n_frames] or
    None (row b: the errors of the used frames in their order in its first ``pairs`` entries, NaN behind them); all on the
    inputs' device.  ``pairs``, ``rmse``, ... ``rot``, ``trans`` are views of the record; ``dict`` reads one problem back."""

    def __init__(self, engine, record, last, scale, errors=None):
        self.E, self.record, self.last, self.scale, self.errors = engine, record, last, float(scale), errors

    def __len__(self):
        return self.record.shape[0]

    pairs = property(lambda self: self.record[:, 0])
    dropped = property(lambda self: self.record[:, 1])
    rmse = property(lambda self: self.record[:, 3])
    mean = property(lambda self: self.record[:, 4])
    median = property(lambda self: self.record[:, 5])
    std = property(lambda self: self.record[:, 6])
    min = property(lambda self: self.record[:, 7])
    max = property(lambda self: self.record[:, 8])
    rot = property(lambda self: self.record[:, 9:18].reshape(-1, 3, 3))
    trans = property(lambda self: self.record[:, 18:21])
    limits = property(lambda self: self.record[:, 21:25])
    flags = property(lambda self: self.record[:, 25])

    def dict(self, b: int = 0) -> dict:
        """The dict eval_ate.py:215-223 returns for problem ``b`` (one read-back); fewer than two pairs raise its ValueError (:140-143)"""
        r = self.record[b].cpu().numpy()
        if int(r[25]) & FLAG_FEW:
            raise ValueError(NO_PAIRS)
        out = {"compared_pose_pairs": int(r[0])}
        out.update({"absolute_translational_error." + k: float(r[3 + i]) for i, k in enumerate(_STATS)})
        return out


def evaluate_ate(est_c2w, gt_c2w, last=None, scale: float = 1.0, errors: bool = False, engine: Optional[Engine] = None) -> AteResult:
    """The absolute trajectory error of ``est_c2w`` against ``gt_c2w`` ([n, 4, 4], tensors, arrays or lists of poses: a
    checkpoint's estimate_c2w_list / gt_c2w_list, or ``Trajectory.est`` / ``.gt``) over the frames ``0..last`` (the checkpoint's
    ``idx``; default: the final frame).  ``last``: an int, a list, or an int64 tensor -- one on the device is used where it is
    (``Trajectory.idx``), and nothing is read back.  ``scale``: the config's (translations are divided by it in fp32)."""
    E = engine if engine is not None else gpu()
    src = est_c2w.device if isinstance(est_c2w, torch.Tensor) else torch.device("cpu")
    est, gt = _poses(E, est_c2w), _poses(E, gt_c2w)
    if est.shape != gt.shape:
        raise _capi.NsrError(f"evaluate_ate: {est.shape[0]} estimated and {gt.shape[0]} ground-truth poses")
    n = est.shape[0]
    if last is None:
        last = [n - 1]
    if isinstance(last, torch.Tensor):
        if last.dtype is not torch.int64:
            raise _capi.NsrError("evaluate_ate: a tensor of last frames is int64")
        last = last.detach().reshape(-1).to(E.device).contiguous()
    else:
        last = torch.tensor([int(v) for v in np.atleast_1d(np.asarray(last))], dtype=torch.int64).to(E.device)
    B = last.numel()
    rec = torch.empty((B, REC), dtype=torch.float64, device=E.device)
    err = torch.full((B, n), float("nan"), dtype=torch.float64, device=E.device) if errors else None
    _launch(E, est, gt, last, scale, rec, err)
    if src != E.device:
        rec, last, err = rec.to(src), last.to(src), (err.to(src) if err is not None else None)
    return AteResult(E, rec, last, scale, err)


def ate_curve(est_c2w, gt_c2w, lasts, scale: float = 1.0, engine: Optional[Engine] = None) -> AteResult:
    """The ATE over the frames ``0..k`` for every k of ``lasts`` (checkpoint indices, or every prefix of a run) in one launch;
    ``.rmse`` is the curve."""
    return evaluate_ate(est_c2w, gt_c2w, last=lasts, scale=scale, engine=engine)


def plot_trajectories(est_c2w, gt_c2w, result: AteResult, b: int = 0, height: int = PLOT_H, width: int = PLOT_W) -> torch.Tensor:
    """eval_ate_plot.png of problem ``b`` of ``result``: u8 [height, width, 3] on the poses' device, drawn from the record in device
    memory (ground truth black, the aligned estimate blue on top, the axes box; no title, legend, ticks or labels)."""
    E = result.E
    if not 0 <= int(b) < len(result):
        raise IndexError(f"plot_trajectories: problem {b} of {len(result)}")
    src = est_c2w.device if isinstance(est_c2w, torch.Tensor) else torch.device("cpu")
    est, gt = _poses(E, est_c2w), _poses(E, gt_c2w)
    if est.shape != gt.shape:
        raise _capi.NsrError(f"plot_trajectories: {est.shape[0]} estimated and {gt.shape[0]} ground-truth poses")
    rec = result.record[int(b)].to(E.device).contiguous()
    last = result.last[int(b):int(b) + 1].to(E.device).contiguous()
    img = torch.empty((int(height), int(width), 3), dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        E.call("nsr_ate_plot", est.data_ptr(), gt.data_ptr(), est.shape[0], last.data_ptr(), result.scale, rec.data_ptr(), int(height),
               int(width), img.data_ptr())
    return img if src == E.device else img.to(src)


def save_plot(img, path: str):
    """Write the bytes of ``plot_trajectories`` as an image file (PNG by the path's suffix)"""
    from PIL import Image
    a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    Image.fromarray(np.ascontiguousarray(a, dtype=np.uint8)).save(path)


# --------------------------------------------------------------------------------------------------
# src/tools/eval_ate.py:259-301
# --------------------------------------------------------------------------------------------------
def main(argv=None, engine: Optional[Engine] = None) -> int:
    from .slam import _resolve, load_config
    from .viewer import load_run
    ap = argparse.ArgumentParser(prog="python -m nice_slam_amd.trajeval", description="Arguments to eval the tracking ATE.")
    ap.add_argument("config", type=str, help="Path to config file.")
    ap.add_argument("--output", type=str, help="output folder, this have higher priority, can overwrite the one in config file")
    ap.add_argument("--default", type=str, default=None, help="the default config the chain ends in (configs/nice_slam.yaml)")
    ap.add_argument("--curve", action="store_true", help="also print the rmse of the frames 0..k for every k up to the checkpoint's idx")
    a = ap.parse_args(argv)
    default = a.default
    if default is None:
        cand = _resolve(os.path.join("configs", "nice_slam.yaml"), a.config)
        default = cand if os.path.exists(cand) else None
    cfg = load_config(a.config, default)
    scale = float(cfg.get("scale", 1.0))
    output = cfg["data"]["output"] if a.output is None else a.output
    est, gt, N = load_run(output, 1.0)              # the lists as they were saved: the kernel divides by the scale, in fp32
    E = engine if engine is not None else gpu()
    est, gt = _poses(E, est), _poses(E, gt)
    res = evaluate_ate(est, gt, last=N, scale=scale, engine=E)
    results = res.dict()
    print(results)
    plot = os.path.join(output, "eval_ate_plot.png")
    save_plot(plot_trajectories(est, gt, res), plot)
    if a.curve:
        lasts = list(range(1, N + 1))
        curve = ate_curve(est, gt, lasts, scale=scale, engine=E).rmse.cpu().numpy() if lasts else []
        for k, v in zip(lasts, curve):
            print(f"{k} {float(v)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
