"""Rendering evaluation on the GPU: how well the learned scene re-renders the frames it was built from -- PSNR, SSIM and the
rendered-depth L1 against the input frames, with the residual maps of the reference's ``Visualizer.vis``
(src/utils/Visualizer.py:53-65: ``|gt - rendered|`` of depth and colour, zeroed where the input depth is 0).

    from nice_slam_amd import imgeval
    m = imgeval.image_metrics(color, gt_color, depth, gt_depth)            # {"psnr", "psnr_valid", "ssim", "depth_l1_cm", ...}
    r = imgeval.evaluate_rendering(renderer, c, decoders, frames)          # {"frames": [...], "mean": {...}, ...}

    s = imgeval.figure_sheet(color, gt_color, depth, gt_depth)             # u8 [SH, SW, 3]: the Visualizer's 2 x 3 figure
    vis = imgeval.Visualizer(freq, inside_freq, vis_dir, renderer, verbose, device)       # Visualizer.py:8-107
    vis.vis(idx, it, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders)               # -> {vis_dir}/{idx:05d}_{it:04d}.jpg

    python -m nice_slam_amd.imgeval RENDERED.npz GT.npz [--figures DIR]    # each file: arrays ``color`` and ``depth``

Every per-pixel and per-window loop runs in libnsr.so (include/nsr.h, "Rendering evaluation" and "Rendering figures"; the
definitions are written out in csrc/nsr_imgmetrics.h and csrc/nsr_figure.h): one launch evaluates a whole batch of frame pairs.

  * PSNR: ``-10 log10(mean((clip(a, 0, 1) - clip(b, 0, 1))^2))``, data range 1, over all pixels (``psnr``) and over the pixels
    with an input depth (``psnr_valid``); the clip is the Visualizer's (:85-87).
  * SSIM: Wang et al. 2004 in the convention of ``pytorch_msssim.ssim(X, Y, data_range=1)``: clipped colours, a normalised
    11 x 11 Gaussian (sigma 1.5), windows wholly inside the image, biased moments, C1 = 0.01^2, C2 = 0.03^2, the mean over
    windows and channels; not masked by depth.
  * Depth L1: ``100 mean |gt - rendered|`` (cm) over the pixels whose input depth is not 0; NaN for a frame without one.
  * Figure: the sheet of Visualizer.py:67-102 as bytes -- input depth, generated depth and depth residual over input RGB,
    generated RGB and RGB residual; the depths through matplotlib's ``Normalize(0, max input depth)`` and plasma map, the
    colours clipped to [0, 1] -- point-sampled, without titles.

Not here: LPIPS (it needs trained network weights).
"""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os
import sys
from typing import Optional

import numpy as np
import torch

from . import _capi
from .common import get_camera_from_tensor
from .engine import Engine, gpu

__all__ = ["image_metrics", "evaluate_rendering", "figure_sheet", "figure_sheet_size", "colorize_depth", "Visualizer", "RESULT_DOUBLES"]

RESULT_DOUBLES = 8               # per frame, include/nsr.h
MIN_SIDE = 11                    # one SSIM window
MAX_FRAMES_PER_LAUNCH = 65535
FIGURE_FRAMES_PER_LAUNCH = 65532  # a multiple of 4: every launch's part of the output starts on a dword


def _images(E: Engine, x, channels: bool, what: str) -> torch.Tensor:
    """[B, H, W(, 3)] contiguous fp32 on the engine's device of one image or a batch (tensor or array, any device, fp32 / fp64)"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    t = t.detach()
    nd = 3 if channels else 2
    if t.dim() == nd:
        t = t[None]
    if t.dim() != nd + 1 or (channels and t.shape[-1] != 3):
        raise ValueError(f"image_metrics: {what} must be [H, W{', 3' if channels else ''}] or a batch of them (got {tuple(t.shape)})")
    return t.to(E.device, torch.float32).contiguous()


def image_metrics(color, gt_color, depth, gt_depth, residuals: bool = False, engine: Optional[Engine] = None) -> dict:
    """Metrics of rendered images against the input frames, one frame (``color`` [H, W, 3], ``depth`` [H, W]) or a batch
    ([B, H, W, 3] / [B, H, W]); tensors or arrays of any device, fp32 or fp64 (evaluated as fp32).  Returns per-frame tensors
    on the engine's device ([B], or 0-dim for one frame): ``psnr``, ``psnr_valid``, ``ssim``, ``depth_l1_cm`` (fp64),
    ``n_valid`` (int64: pixels whose input depth is not 0), ``depth_max`` (fp32: the largest input depth, the Visualizer's
    ``vmax``) and the raw fp64 sums behind them, ``sq_err`` / ``sq_err_valid`` (squared colour error over all / the valid
    pixels, three channels) and ``depth_abs_err`` (m, over the valid pixels); with ``residuals`` also ``depth_residual``
    [B, H, W] and ``color_residual`` [B, H, W, 3] (fp32).  The sums are taken in a fixed order: the same input gives the same
    bits, whatever else is in the batch."""
    E = engine or gpu()
    lib = E.lib
    single = (color.ndim if hasattr(color, "ndim") else np.asarray(color).ndim) == 3
    a, b = _images(E, color, True, "color"), _images(E, gt_color, True, "gt_color")
    d, g = _images(E, depth, False, "depth"), _images(E, gt_depth, False, "gt_depth")
    if a.shape != b.shape or d.shape != g.shape or a.shape[:3] != d.shape:
        raise ValueError(f"image_metrics: shapes differ (color {tuple(a.shape)}, gt_color {tuple(b.shape)}, depth {tuple(d.shape)}, "
                         f"gt_depth {tuple(g.shape)})")
    B, H, W = d.shape
    if H < MIN_SIDE or W < MIN_SIDE:
        raise _capi.NsrError(f"image_metrics: images must be at least {MIN_SIDE} x {MIN_SIDE} (got {H} x {W})")
    res = torch.zeros((B, RESULT_DOUBLES), dtype=torch.float64, device=E.device)
    dres = torch.empty((B, H, W), dtype=torch.float32, device=E.device) if residuals else None
    cres = torch.empty((B, H, W, 3), dtype=torch.float32, device=E.device) if residuals else None
    with torch.no_grad(), E.guard():
        for k0 in range(0, B, MAX_FRAMES_PER_LAUNCH):
            kb = min(MAX_FRAMES_PER_LAUNCH, B - k0)
            nbytes = int(lib.nsr_image_metrics_workspace_bytes(kb, H, W))
            if nbytes < 0:
                raise _capi.NsrError(f"image_metrics: unsupported sizes ({kb} frames of {H} x {W})")
            ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=E.device)
            sl = slice(k0, k0 + kb)
            E.call("nsr_image_metrics", a[sl].data_ptr(), b[sl].data_ptr(), d[sl].data_ptr(), g[sl].data_ptr(), kb, H, W,
                   res[sl].data_ptr(), dres[sl].data_ptr() if residuals else None, cres[sl].data_ptr() if residuals else None,
                   ws.data_ptr(), nbytes)
    se_all, n_all, se_valid, n_valid, ssim, l1, dmax = (res[:, i] for i in range(7))
    out = {"psnr": -10.0 * torch.log10(se_all / (3.0 * n_all)),
           "psnr_valid": -10.0 * torch.log10(se_valid / (3.0 * n_valid)),        # 0 / 0: NaN for a frame without valid depth
           "ssim": ssim.clone(),
           "depth_l1_cm": 100.0 * l1 / n_valid,
           "n_valid": n_valid.to(torch.int64),
           "depth_max": dmax.to(torch.float32),
           "sq_err": se_all.clone(), "sq_err_valid": se_valid.clone(), "depth_abs_err": l1.clone()}
    if residuals:
        out["depth_residual"], out["color_residual"] = dres, cres
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out


# --------------------------------------------------------------------------------------------------
# the figure (src/utils/Visualizer.py:67-102)
# --------------------------------------------------------------------------------------------------
def figure_sheet_size(H: int, W: int, stride: int = 1, margin: int = 8, gap: int = 8, engine: Optional[Engine] = None):
    """(SH, SW) of the sheet of an H x W frame: 2 margin + 2 ceil(H / stride) + gap by 2 margin + 3 ceil(W / stride) + 2 gap"""
    lib = (engine or gpu()).lib
    sh, sw = C.c_int32(0), C.c_int32(0)
    lib.call("nsr_figure_sheet_size", int(H), int(W), int(stride), int(margin), int(gap), C.byref(sh), C.byref(sw))
    return sh.value, sw.value


def figure_sheet(color, gt_color, depth, gt_depth, stride: int = 1, margin: int = 8, gap: int = 8, engine: Optional[Engine] = None,
                 return_vmax: bool = False):
    """The Visualizer's figure of rendered images against the input frames as bytes: u8 [B, SH, SW, 3] on the engine's device
    ([SH, SW, 3] for one frame), inputs as for ``image_metrics`` (any size from 1 x 1).  Row 0 shows the input depth, the
    generated depth and their residual through the plasma map with ``vmax`` = the frame's largest input depth, row 1 the input
    colour, the generated colour and their residual clipped to [0, 1]; every ``stride``-th pixel, ``margin`` white pixels around
    and ``gap`` between the panels.  One ``nsr_figure_sheet`` call for the batch.  ``return_vmax``: also the [B] fp32 maxima."""
    E = engine or gpu()
    single = (color.ndim if hasattr(color, "ndim") else np.asarray(color).ndim) == 3
    a, b = _images(E, color, True, "color"), _images(E, gt_color, True, "gt_color")
    d, g = _images(E, depth, False, "depth"), _images(E, gt_depth, False, "gt_depth")
    if a.shape != b.shape or d.shape != g.shape or a.shape[:3] != d.shape:
        raise ValueError(f"figure_sheet: shapes differ (color {tuple(a.shape)}, gt_color {tuple(b.shape)}, depth {tuple(d.shape)}, "
                         f"gt_depth {tuple(g.shape)})")
    B, H, W = d.shape
    SH, SW = figure_sheet_size(H, W, stride, margin, gap, E)
    sheet = torch.empty((B, SH, SW, 3), dtype=torch.uint8, device=E.device)
    vmax = torch.empty((B,), dtype=torch.float32, device=E.device)
    with torch.no_grad(), E.guard():
        for k0 in range(0, B, FIGURE_FRAMES_PER_LAUNCH):
            sl = slice(k0, min(B, k0 + FIGURE_FRAMES_PER_LAUNCH))
            E.call("nsr_figure_sheet", a[sl].data_ptr(), b[sl].data_ptr(), d[sl].data_ptr(), g[sl].data_ptr(), sl.stop - k0, H, W,
                   int(stride), int(margin), int(gap), vmax[sl].data_ptr(), sheet[sl].data_ptr())
    if single:
        sheet, vmax = sheet[0], vmax[0]
    return (sheet, vmax) if return_vmax else sheet


def colorize_depth(depth, vmax=None, engine: Optional[Engine] = None) -> torch.Tensor:
    """Depth image(s) [H, W] or [B, H, W] through the figure's colour map -- matplotlib's ``plasma(Normalize(0, vmax)(depth))``
    as bytes, a NaN white -- u8 [B, H, W, 3] ([H, W, 3] for one image) on the engine's device.  ``vmax``: a number, a [B]
    tensor or array, or None: each image's own maximum."""
    E = engine or gpu()
    single = (depth.ndim if hasattr(depth, "ndim") else np.asarray(depth).ndim) == 2
    d = _images(E, depth, False, "depth")
    B, H, W = d.shape
    vm = None
    if vmax is not None:
        vm = torch.as_tensor(vmax).detach().to(E.device, torch.float32).reshape(-1)
        vm = (vm.expand(B) if vm.numel() == 1 else vm).contiguous()
        if vm.shape != (B,):
            raise ValueError(f"colorize_depth: vmax must be one number or one per image (got {tuple(vm.shape)} for {B} images)")
    rgb = torch.empty((B, H, W, 3), dtype=torch.uint8, device=E.device)
    with torch.no_grad(), E.guard():
        for k0 in range(0, B, FIGURE_FRAMES_PER_LAUNCH):
            sl = slice(k0, min(B, k0 + FIGURE_FRAMES_PER_LAUNCH))
            E.call("nsr_depth_colorize", d[sl].data_ptr(), sl.stop - k0, H, W, None if vm is None else vm[sl].data_ptr(), rgb[sl].data_ptr())
    return rgb[0] if single else rgb


def save_sheet(sheet: torch.Tensor, path: str, quality: int = 90, encoder: str = "pil", engine: Optional[Engine] = None):
    """one u8 [SH, SW, 3] sheet as an image file (``viewer.save_image``: ``encoder`` "pil" or "gpu")"""
    from .viewer import save_image
    save_image(sheet, path, quality=quality, encoder=encoder, engine=engine)


class Visualizer:
    """src/utils/Visualizer.py:8-107 on the GPU: ``vis`` renders the frame at a pose and saves the 2 x 3 figure when
    ``idx % freq == 0 and iter % inside_freq == 0``.  ``freq <= 0`` or ``inside_freq <= 0``: off, nothing is ever drawn (the
    reference would divide by zero) and the directory is not created.  ``stride`` / ``margin`` / ``gap``: the sheet's layout
    (``figure_sheet``); ``engine``: where the sheet is built (default: the product's engine of ``device``); ``encoder``: "pil"
    (the host encodes each sheet) or "gpu" (the sheets of a ``vis_many`` call are encoded where they are, in one call)."""

    def __init__(self, freq, inside_freq, vis_dir, renderer, verbose, device="cuda:0", stride: int = 1, margin: int = 8, gap: int = 8,
                 engine: Optional[Engine] = None, encoder: str = "pil"):
        if encoder not in ("pil", "gpu"):
            raise ValueError(f"Visualizer: encoder must be 'pil' or 'gpu' (got {encoder!r})")
        self.encoder = encoder
        self.freq, self.inside_freq = int(freq), int(inside_freq)
        self.device, self.vis_dir, self.verbose, self.renderer = device, vis_dir, verbose, renderer
        self.stride, self.margin, self.gap, self.engine = stride, margin, gap, engine
        self.on = self.freq > 0 and self.inside_freq > 0
        self.drawn = 0
        if self.on:
            os.makedirs(f"{vis_dir}", exist_ok=True)

    def due(self, idx, iter) -> bool:
        return self.on and int(idx) % self.freq == 0 and int(iter) % self.inside_freq == 0

    def due_iters(self, idx, n_iters: int) -> list:
        """the iterations of ``range(n_iters)`` on which frame ``idx`` has a figure due"""
        if not self.on or int(idx) % self.freq != 0:
            return []
        return list(range(0, int(n_iters), self.inside_freq))

    def _c2w(self, pose):
        if len(pose.shape) == 1:                                                   # Visualizer.py:43-49
            bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=pose.device)
            return torch.cat([get_camera_from_tensor(pose.clone().detach()), bottom], dim=0)
        return pose

    def vis_many(self, idx, iters, poses, gt_depth, gt_color, c, decoders):
        """Several poses of ONE frame (``poses[i]`` belongs to iteration ``iters[i]``; 4x4 poses or 7-float camera tensors):
        those that are due are rendered, their sheets are built by one ``nsr_figure_sheet`` launch and saved as
        ``{vis_dir}/{idx:05d}_{iter:04d}.jpg``.  Returns the sheets u8 [n, SH, SW, 3] in the order given, None when none is due."""
        todo = [(int(it), p) for it, p in zip(iters, poses) if self.due(idx, it)]
        if not todo:
            return None
        E = self.engine or _engine_of(self.device)
        with torch.no_grad():
            depths, colors = [], []
            for _, pose in todo:
                depth, _, color = self.renderer.render_img(c, decoders, self._c2w(pose), self.device, stage="color", gt_depth=gt_depth)
                depths.append(depth.detach().to(E.device, torch.float32))
                colors.append(color.detach().to(E.device, torch.float32))
            n = len(todo)
            gd = torch.as_tensor(gt_depth).detach().to(E.device, torch.float32)
            gc = torch.as_tensor(gt_color).detach().to(E.device, torch.float32)
            sheets = figure_sheet(torch.stack(colors), gc[None].expand(n, *gc.shape), torch.stack(depths), gd[None].expand(n, *gd.shape),
                                  stride=self.stride, margin=self.margin, gap=self.gap, engine=E)
        streams = None
        if self.encoder == "gpu":
            from .jpeg import encode_jpeg
            streams = encode_jpeg(sheets, quality=90, engine=E)
        for k, ((it, _), sheet) in enumerate(zip(todo, sheets)):
            path = f"{self.vis_dir}/{int(idx):05d}_{it:04d}.jpg"
            if streams is None:
                save_sheet(sheet, path)
            else:
                with open(path, "wb") as fh:
                    fh.write(streams[k])
            self.drawn += 1
            if self.verbose:
                print(f"Saved rendering visualization of color/depth image at {path}")
        return sheets

    def vis(self, idx, iter, gt_depth, gt_color, c2w_or_camera_tensor, c, decoders):
        """Visualizer.py:24-107"""
        return self.vis_many(idx, [iter], [c2w_or_camera_tensor], gt_depth, gt_color, c, decoders)


def _engine_of(device) -> Engine:
    from .engine import on
    return on(device)


METRICS = ("psnr", "psnr_valid", "ssim", "depth_l1_cm")


def _means(rows) -> dict:
    """the mean of each metric over the frames where it is a number (a frame without valid depth has no depth L1 and no
    psnr_valid), summed in frame order"""
    out = {}
    for k in METRICS:
        vals = [r[k] for r in rows if not math.isnan(r[k])]
        out[k] = math.fsum(vals) / len(vals) if vals else float("nan")
    return out


def evaluate_rendering(renderer, c, decoders, frames, stage: str = "color", device="cuda:0", batch: int = 8, residuals: bool = False,
                       engine: Optional[Engine] = None, figures: Optional[str] = None) -> dict:
    """Re-render frames and measure them: ``frames`` is an iterable of ``(idx, gt_color [H, W, 3], gt_depth [H, W],
    c2w_or_camera_tensor)``; a 7-float camera tensor (quaternion, translation) goes through ``get_camera_from_tensor`` as in
    Visualizer.py:43-51.  Each frame is rendered with ``renderer.render_img(c, decoders, c2w, device, stage, gt_depth=gt_depth)``
    and ``batch`` frames at a time are evaluated by one launch.  Returns

        {"frames": [{"idx", "psnr", "psnr_valid", "ssim", "depth_l1_cm", "n_valid", "depth_max"}, ...],     # floats, frame order
         "mean": {"psnr", "psnr_valid", "ssim", "depth_l1_cm"},      # each over the frames where it is a number
         "n_frames": int, "n_no_depth": int}                          # frames without any valid depth: not in the depth mean

    With ``residuals`` every frame's row also holds the rendered ``depth`` and ``color`` and the two residual maps (fp32, on
    the engine's device).  ``figures``: a directory that receives each frame's figure (``figure_sheet``) as ``{idx:05d}.jpg``,
    one launch per ``batch`` frames."""
    E = engine or gpu()
    batch = max(1, int(batch))
    rows, pending = [], []
    if figures is not None:
        os.makedirs(figures, exist_ok=True)

    def flush():
        if not pending:
            return
        m = image_metrics(torch.stack([p[1] for p in pending]), torch.stack([p[2] for p in pending]),
                          torch.stack([p[3] for p in pending]), torch.stack([p[4] for p in pending]), residuals=residuals, engine=E)
        host = {k: m[k].cpu() for k in METRICS + ("n_valid", "depth_max")}
        if figures is not None:
            sheets = figure_sheet(torch.stack([p[1] for p in pending]), torch.stack([p[2] for p in pending]),
                                  torch.stack([p[3] for p in pending]), torch.stack([p[4] for p in pending]), engine=E)
            for p_, sheet in zip(pending, sheets):
                save_sheet(sheet, os.path.join(figures, f"{int(p_[0]):05d}.jpg"))
        for i, p in enumerate(pending):
            row = {"idx": p[0]}
            row.update({k: float(host[k][i]) for k in METRICS})
            row["n_valid"], row["depth_max"] = int(host["n_valid"][i]), float(host["depth_max"][i])
            if residuals:
                row.update(depth=p[3], color=p[1], depth_residual=m["depth_residual"][i], color_residual=m["color_residual"][i])
            rows.append(row)
        pending.clear()

    with torch.no_grad():
        for idx, gt_color, gt_depth, pose in frames:
            if len(pose.shape) == 1:
                bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=pose.device)
                c2w = torch.cat([get_camera_from_tensor(pose.clone().detach()), bottom], dim=0)
            else:
                c2w = pose
            depth, _, color = renderer.render_img(c, decoders, c2w, device, stage, gt_depth=gt_depth)
            pending.append((idx, color.detach().to(E.device, torch.float32), torch.as_tensor(gt_color).detach().to(E.device, torch.float32),
                            depth.detach().to(E.device, torch.float32), torch.as_tensor(gt_depth).detach().to(E.device, torch.float32)))
            if len(pending) == batch:
                flush()
        flush()
    return {"frames": rows, "mean": _means(rows), "n_frames": len(rows), "n_no_depth": sum(1 for r in rows if r["n_valid"] == 0)}


# --------------------------------------------------------------------------------------------------
# command line
# --------------------------------------------------------------------------------------------------
def main(argv=None, engine: Optional[Engine] = None):
    ap = argparse.ArgumentParser(prog="python -m nice_slam_amd.imgeval",
                                 description="PSNR, SSIM and depth L1 of rendered frames against input frames on the GPU, and their figures.")
    ap.add_argument("rendered", type=str, help=".npz with the rendered frames: color [B, H, W, 3] (or [H, W, 3]) and depth [B, H, W]")
    ap.add_argument("gt", type=str, help=".npz with the input frames: color and depth of the same shapes")
    ap.add_argument("--figures", type=str, default=None, help="a directory for one figure per frame, {frame:05d}.jpg (Visualizer.py:67-102)")
    args = ap.parse_args(argv)
    r, g = np.load(args.rendered), np.load(args.gt)
    m = image_metrics(r["color"], g["color"], r["depth"], g["depth"], engine=engine)
    if args.figures is not None:
        os.makedirs(args.figures, exist_ok=True)
        sheets = figure_sheet(r["color"], g["color"], r["depth"], g["depth"], engine=engine)
        for k, sheet in enumerate(sheets if sheets.dim() == 4 else sheets[None]):
            save_sheet(sheet, os.path.join(args.figures, f"{k:05d}.jpg"))
    rows = [{k: float(v) for k, v in zip(METRICS, vals)}
            for vals in zip(*(m[k].reshape(-1).cpu().tolist() for k in METRICS))]
    mean = _means(rows)
    print("PSNR: ", mean["psnr"])
    print("SSIM: ", mean["ssim"])
    print("Depth L1: ", mean["depth_l1_cm"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
