"""NICE-SLAM on a sequence, from its config to the run directory (``ckpts/*.tar``, ``mesh/*_mesh.ply``).

    cfg = load_config("configs/Replica/room0.yaml", "configs/nice_slam.yaml")        # src/config.py:10-59
    slam = NICE_SLAM(cfg, args)                                                       # src/NICE_SLAM.py:26-98
    slam.run()                                                                        # src/NICE_SLAM.py:252-305

    python -m nice_slam_amd.slam CONFIG [--default DEFAULT.yaml] [--input_folder D] [--output D] [--random-decoders] [--frames N]

What the reference spreads over run.py, src/NICE_SLAM.py, src/Tracker.py, src/Mapper.py, src/utils/Logger.py and src/config.py,
on the package's own pieces: ``get_dataset``, ``tracking_loss`` / ``mapping_loss`` with ``FlatAdam`` / ``MaskedGridAdam``,
``FrustumSelector``, ``KeyframeSelector``, ``Mesher`` and the device-side ``Trajectory`` (poses.py).  One process, strict
synchronisation: a frame is tracked, then -- every ``mapping.every_frame`` frames and on the last one -- mapped, the coarse level
after the others (Tracker.py:161-166, Mapper.py:554-556).

The estimated trajectory and the keyframe poses live in device memory.  A tracked frame is: two image copies, one fill of the
frame index, and ONE graph replay holding the motion model (``nsr_pose_predict``), the optimiser reset, ``tracking.iters``
iterations and the choice of the best one (``nsr_pose_commit``) -- nothing is read back.  A mapping call gathers its window's
poses on the device (``get_tensor_from_camera``) and writes them back with ``Trajectory.store``; it does synchronise, because
``FrustumSelector`` and ``KeyframeSelector`` read poses and counts on the host.

The figures of the reference's ``Visualizer`` (``tracking_vis/``, ``mapping_vis/``: ``vis_freq``, ``vis_inside_freq``,
``no_vis_on_first_frame``) are drawn by ``imgeval.Visualizer``.  The tracked frame stays one replay: its figures are drawn
after it, from the pose BEFORE each due iteration -- the motion model's 7-vector, which the frame copies into a ``start``
buffer, then ``hist[j - 1, 1:]`` -- all of one frame in one ``nsr_figure_sheet`` launch.  An optional ``encoder: gpu`` next to
``vis_freq`` (``tracking`` / ``mapping``) has the sheets encoded on the GPU too (``jpeg.encode_jpeg``); absent, PIL does it.  An
optional ``decoder: gpu`` under ``data`` has the sequence's colour JPEGs decoded on the GPU (``jpeg.decode_jpeg``: the same
pixels; absent, PIL decodes them).  The copy is recorded only when some
tracked frame of the sequence can have a figure due; a frame (and a mapping call) without one executes what it did before.

Deviations from the reference, all deliberate:
  * ``sync_method`` 'loose' and 'free' run as 'strict' (one notice); the run is one process, not three, on ``mapping.device``;
  * the coarse mapper shares the mapper's keyframe list (in the reference it keeps a copy that misses the bundle-adjusted poses);
  * the figures are sheets of pixels without titles; the coarse mapper draws none (in the reference
    it overwrites the mapper's files of the same name); the tracker reads ``tracking.no_vis_on_first_frame`` (the reference's
    reads the mapping section's, Tracker.py:58);
  * ``low_gpu_mem`` is accepted and ignored: keyframe colour and depth stay on the device;
  * a frame none of whose iterations has a loss below 1e10 keeps the motion model's pose (the reference fails on ``None`` there,
    Tracker.py:250-251);
  * the pixels of an iteration are drawn inside the window kernel (mapping.PIXEL_DRAW), not by ``torch.randint`` per keyframe.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import shutil
import sys
import time
import types
import weakref
from typing import Optional

import numpy as np
import torch

from . import _capi
from .common import get_camera_from_tensor, grid_init, load_bound, set_decoder_bounds
from .datasets import get_dataset
from .decoders import NICE
from .engine import on
from .frustum import FrustumSelector
from .imgeval import Visualizer
from .keyframes import KeyframeSelector
from .mapping import backward, mapping_loss, tracking_loss
from .mesher import Mesher
from .optim import FlatAdam, MaskedGridAdam
from .poses import Trajectory, get_tensor_from_camera
from .renderer import Renderer

__all__ = ["load_config", "update_recursive", "NICE_SLAM", "Tracker", "Mapper", "load_pretrained", "ate_rmse", "main"]

CKPT_KEYS = ("c", "decoder_state_dict", "gt_c2w_list", "estimate_c2w_list", "keyframe_list", "selected_keyframes", "idx")   # Logger.py:23-31


# --------------------------------------------------------------------------------------------------
# src/config.py
# --------------------------------------------------------------------------------------------------
def update_recursive(dict1: dict, dict2: dict):
    """src/config.py:45-59"""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v


def _resolve(path: str, near: str) -> str:
    """``inherit_from`` names a path relative to the reference's root (its working directory): when it does not exist from
    here, look for it from the directories above the file that names it"""
    if os.path.exists(path) or os.path.isabs(path):
        return path
    d = os.path.dirname(os.path.abspath(near))
    while d != os.path.dirname(d):
        if os.path.exists(os.path.join(d, path)):
            return os.path.join(d, path)
        d = os.path.dirname(d)
    return path


def load_config(path: str, default_path: Optional[str] = None) -> dict:
    """src/config.py:10-42: the file, on top of what its ``inherit_from`` chain gives (else ``default_path``, else nothing)"""
    import yaml
    with open(path, "r") as f:
        cfg_special = yaml.full_load(f)
    inherit_from = cfg_special.get("inherit_from")
    if inherit_from is not None:
        cfg = load_config(_resolve(inherit_from, path), default_path)
    elif default_path is not None:
        with open(default_path, "r") as f:
            cfg = yaml.full_load(f)
    else:
        cfg = dict()
    update_recursive(cfg, cfg_special)
    return cfg


# --------------------------------------------------------------------------------------------------
# trajectory error (src/tools/eval_ate.py:44-78,147-223; the formula of tools/ate.py)
# --------------------------------------------------------------------------------------------------
def align(model: np.ndarray, data: np.ndarray):
    """Horn's closed-form alignment of two (3, n) trajectories -> (rot, trans, per-point error of rot model + trans against data)"""
    model, data = np.asarray(model, np.float64), np.asarray(data, np.float64)
    mz, dz = model - model.mean(1, keepdims=True), data - data.mean(1, keepdims=True)
    U, _, Vh = np.linalg.svd((mz @ dz.T).T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    trans = data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True)
    err = rot @ model + trans - data
    return rot, trans, np.sqrt((err * err).sum(0))


def ate_rmse(est_c2w, gt_c2w) -> dict:
    """Absolute trajectory error of matching pose lists, the estimate aligned to the ground truth (eval_ate.py:166), in the poses' unit"""
    est = np.stack([np.asarray(c, np.float64)[:3, 3] for c in est_c2w], 1)
    gt = np.stack([np.asarray(c, np.float64)[:3, 3] for c in gt_c2w], 1)
    _, _, e = align(est, gt)
    return {"compared_pose_pairs": int(e.shape[0]), "rmse": float(np.sqrt(np.dot(e, e) / len(e))), "mean": float(e.mean()),
            "median": float(np.median(e)), "std": float(e.std()), "min": float(e.min()), "max": float(e.max())}


# --------------------------------------------------------------------------------------------------
# pretrained decoders (src/NICE_SLAM.py:159-190)
# --------------------------------------------------------------------------------------------------
def load_pretrained(decoders: NICE, cfg: dict, device="cpu"):
    """Load the ConvONet checkpoints ``cfg['pretrained_decoders']`` names into the coarse, middle and fine decoders: the keys
    that contain 'decoder' and not 'encoder', with 'decoder.' (8 characters) stripped for the coarse decoder and 'decoder.coarse.'
    (8 + 7) / 'decoder.fine.' (8 + 5) for the middle / fine one.  A missing file raises FileNotFoundError naming it."""
    def read(path):
        if not os.path.isfile(path):
            raise FileNotFoundError(f"pretrained decoders: {path} does not exist (cfg['pretrained_decoders']); pass decoders=\"random\" "
                                    f"(--random-decoders) to run from randomly initialised decoders")
        try:
            return torch.load(path, map_location=device, weights_only=True)
        except Exception:                                        # checkpoints of the reference hold more than tensors
            return torch.load(path, map_location=device, weights_only=False)

    if cfg["coarse"]:
        ckpt = read(cfg["pretrained_decoders"]["coarse"])
        coarse_dict = {}
        for key, val in ckpt["model"].items():
            if ("decoder" in key) and ("encoder" not in key):
                coarse_dict[key[8:]] = val
        decoders.coarse_decoder.load_state_dict(coarse_dict)
    ckpt = read(cfg["pretrained_decoders"]["middle_fine"])
    middle_dict, fine_dict = {}, {}
    for key, val in ckpt["model"].items():
        if ("decoder" in key) and ("encoder" not in key):
            if "coarse" in key:
                middle_dict[key[8 + 7:]] = val
            elif "fine" in key:
                fine_dict[key[8 + 5:]] = val
    decoders.middle_decoder.load_state_dict(middle_dict)
    decoders.fine_decoder.load_state_dict(fine_dict)


# --------------------------------------------------------------------------------------------------
# the tracker (src/Tracker.py:130-258)
# --------------------------------------------------------------------------------------------------
class Tracker:
    """One frame: ``update_para_from_mapping``, then one replay of the frame's graph.  ``slam`` provides cfg, device, renderer,
    shared_c, shared_decoders, traj, counters and timers, and output, verbose and n_img for the figures (NICE_SLAM below; a
    test may pass a namespace)."""

    def __init__(self, slam):
        tc = slam.cfg["tracking"]
        self._slam, self.device, self.traj = weakref.ref(slam), slam.device, slam.traj     # (no cycle: see NICE_SLAM.release)
        self.cam_lr, self.num_cam_iters, self.pixels = tc["lr"], int(tc["iters"]), int(tc["pixels"])
        self.gt_camera, self.seperate_LR = tc["gt_camera"], tc["seperate_LR"]
        self.w_color_loss, self.handle_dynamic = tc["w_color_loss"], tc["handle_dynamic"]
        self.ignore_edge_W, self.ignore_edge_H = tc["ignore_edge_W"], tc["ignore_edge_H"]
        self.use_color_in_tracking, self.const_speed_assumption = tc["use_color_in_tracking"], tc["const_speed_assumption"]
        self.prev_map_version = None
        self.c, self.decoders = None, None
        self._ft = None
        self.no_vis_on_first_frame = tc["no_vis_on_first_frame"]
        self.visualizer = Visualizer(tc["vis_freq"], tc["vis_inside_freq"],                # Tracker.py:66-68
                                     os.path.join(slam.output, "vis" if "Demo" in slam.output else "tracking_vis"), slam.renderer,
                                     slam.verbose, self.device, encoder=tc.get("encoder", "pil"))
        # a tracked frame (idx >= 1) of this sequence can have a figure due: only then does the frame keep the motion model's pose
        self.keep_start = self.visualizer.on and self.num_cam_iters > 0 and any(
            self.visualizer.due(i, 0) for i in range(1, slam.n_img))

    slam = property(lambda self: self._slam())

    def update_para_from_mapping(self):
        """Tracker.py:130-142: the tracker renders from its own copy of the map, refreshed when the mapper has run.  Static
        buffers, so that the captured frame keeps reading the same addresses; grids and decoder blobs in one multi-tensor copy."""
        slam = self.slam
        if self.c is None:
            self.c = {k: v.detach().clone(memory_format=torch.preserve_format) for k, v in slam.shared_c.items()}
            self.decoders = copy.deepcopy(slam.shared_decoders)
            for p in self.decoders.parameters():
                p.requires_grad_(False)                          # nothing steps them (the reference discards their gradients)
        if self.prev_map_version == slam.map_version:
            return
        self.prev_map_version = slam.map_version
        with torch.no_grad():
            dst = list(self.c.values()) + [m.flat_params() for m in self.decoders.children()]
            src = list(slam.shared_c.values()) + [m.flat_params() for m in slam.shared_decoders.children()]
            torch._foreach_copy_(dst, src)
        self.decoders.repack()

    def _setup(self, color, depth):
        dev, n_it = self.device, self.num_cam_iters
        buf = torch.zeros(7, dtype=torch.float32, device=dev)          # the pose parameters: nsr_pose_predict writes them
        if self.seperate_LR:                                            # Tracker.py:202-213: T at lr, the quaternion at 0.2 lr
            quad, T = buf[:4].detach().requires_grad_(True), buf[4:].detach().requires_grad_(True)
            params, lrs = [T, quad], [self.cam_lr, self.cam_lr * 0.2]
        else:                                                           # Tracker.py:214-219
            quad = T = None
            params, lrs = [buf.detach().requires_grad_(True)], [self.cam_lr]
        self._ft = {"buf": buf, "quad": quad, "T": T, "params": params, "opt": FlatAdam(params, lr=lrs),
                    "depth": depth.clone(), "color": color.clone(), "i": torch.zeros(1, dtype=torch.long, device=dev),
                    "hist": torch.zeros((max(n_it, 1), 8), dtype=torch.float32, device=dev),       # loss | pose per iteration
                    "best": torch.zeros(8, dtype=torch.float32, device=dev), "graph": None,
                    "start": torch.zeros(7, dtype=torch.float32, device=dev) if self.keep_start else None}
        return self._ft

    def _iteration(self):
        """Tracker.optimize_cam_in_batch (Tracker.py:71-128) and the bookkeeping of :232-247 on the device"""
        ft, slam = self._ft, self.slam
        ft["opt"].zero_grad(set_to_none=True)
        cam = torch.cat([ft["quad"], ft["T"]], 0) if self.seperate_LR else ft["params"][0]            # Tracker.py:226-227
        c2w = get_camera_from_tensor(cam)
        loss = tracking_loss(slam.renderer, self.c, self.decoders, c2w, ft["depth"], ft["color"], self.pixels, self.ignore_edge_H,
                             self.ignore_edge_W, w_color=self.w_color_loss, handle_dynamic=self.handle_dynamic,
                             use_color=self.use_color_in_tracking)
        backward(loss)
        ft["opt"].step()
        with torch.no_grad():
            ft["hist"].index_copy_(0, ft["i"], torch.cat([loss.detach().reshape(1).float(), ft["buf"]]).reshape(1, 8))
            ft["i"] += 1

    def _frame(self, iters: int):
        """what a frame's graph holds: Tracker.py:192-201, :212-224, the iterations, :245-253"""
        ft = self._ft
        self.traj.predict(ft["buf"], const_speed=self.const_speed_assumption)
        with torch.no_grad():
            if ft["start"] is not None:
                ft["start"].copy_(ft["buf"])                        # the pose before iteration 0, for the frame's figures
            ft["opt"].reset_state()
            ft["i"].zero_()
        for _ in range(iters):
            self._iteration()
        if iters == self.num_cam_iters and iters > 0:
            self.traj.commit(ft["hist"], ft["best"])

    def track(self, idx: int, color: torch.Tensor, depth: torch.Tensor):
        """est[idx] := the tracked pose of frame ``idx`` (colour [H,W,3], depth [H,W] on the device).  After the first tracked
        frame -- which runs one eager iteration and captures the graph -- nothing here waits for the device."""
        slam = self.slam
        self.update_para_from_mapping()
        self.traj.set_index(idx)
        if idx == 0 or self.gt_camera:                              # Tracker.py:184-188
            self.traj.est[idx].copy_(self.traj.gt[idx])
            if not self.no_vis_on_first_frame:
                self.visualizer.vis(idx, 0, depth, color, self.traj.gt[idx], self.c, self.decoders)
            return
        ft = self._ft
        if ft is None:
            t_cap = time.perf_counter()
            ft = self._setup(color, depth)
            if self.num_cam_iters > 0:
                self._frame(1)                                      # eager once: optimiser state, code objects, the draw state
                torch.cuda.synchronize(self.device)
                ft["graph"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ft["graph"]):
                    self._frame(self.num_cam_iters)
                torch.cuda.synchronize(self.device)
            slam.timers["tracking_capture_s"] += time.perf_counter() - t_cap
        else:
            with torch.no_grad():
                ft["depth"].copy_(depth)
                ft["color"].copy_(color)
        if ft["graph"] is None:                                     # tracking.iters = 0: the motion model alone
            self._frame(0)
        else:
            ft["graph"].replay()
        slam.counters["tracking_iters"] += self.num_cam_iters
        slam.counters["tracking_rays"] += self.num_cam_iters * self.pixels
        due = self.visualizer.due_iters(idx, self.num_cam_iters) if self.keep_start else []
        if due:                                                     # Tracker.py:229-230, after the replay
            self.visualizer.vis_many(idx, due, self.figure_poses(due), depth, color, self.c, self.decoders)

    def figure_poses(self, iters) -> list:
        """the camera tensors the frame's iterations ``iters`` started from: ``start``, then the pose after iteration j - 1"""
        ft = self._ft
        return [ft["start"] if j == 0 else ft["hist"][j - 1, 1:] for j in iters]


# --------------------------------------------------------------------------------------------------
# the mapper (src/Mapper.py:230-657)
# --------------------------------------------------------------------------------------------------
def random_select(length: int, k: int, rng=np.random) -> list:
    """src/common.py:204-208"""
    return list(rng.permutation(np.array(range(length)))[:min(length, k)])


class Mapper:
    """``optimize_map`` of the mapper (stages middle / fine / colour, local BA) and of the coarse mapper (``coarse_mapper=True``:
    stage coarse, 'global' selection, no BA, no depth-guided samples, every coarse voxel; Mapper.py:79-80,305-306,403-404,484,
    602-603).  Both work on the keyframes NICE_SLAM holds."""

    def __init__(self, slam, coarse_mapper: bool = False):
        mc = slam.cfg["mapping"]
        self._slam, self.device, self.coarse_mapper, self.mc = weakref.ref(slam), slam.device, coarse_mapper, mc
        self.fix_fine, self.fix_color = mc["fix_fine"], mc["fix_color"]
        self.BA_cam_lr, self.mapping_pixels, self.w_color_loss = mc["BA_cam_lr"], int(mc["pixels"]), mc["w_color_loss"]
        self.fine_iter_ratio, self.middle_iter_ratio = mc["fine_iter_ratio"], mc["middle_iter_ratio"]
        self.mapping_window_size = int(mc["mapping_window_size"])
        self.frustum_feature_selection = mc["frustum_feature_selection"]
        self.keyframe_selection_method = "global" if coarse_mapper else mc["keyframe_selection_method"]
        if self.keyframe_selection_method not in ("overlap", "global"):
            raise ValueError(f"mapping.keyframe_selection_method '{self.keyframe_selection_method}': 'overlap' or 'global'")
        self.save_selected_keyframes_info = mc["save_selected_keyframes_info"]
        self.selected_keyframes = {}
        self.BA = False
        self.rng = np.random.RandomState(slam.seed + 1) if coarse_mapper else np.random     # (its own process in the reference)
        self.last_loss = float("nan")
        self.no_vis_on_first_frame = mc["no_vis_on_first_frame"]
        self.visualizer = None                                      # Mapper.py:88-90; the coarse mapper draws nothing
        if not coarse_mapper and "Demo" not in slam.output:
            self.visualizer = Visualizer(mc["vis_freq"], mc["vis_inside_freq"], os.path.join(slam.output, "mapping_vis"), slam.renderer,
                                         slam.verbose, self.device, encoder=mc.get("encoder", "pil"))

    slam = property(lambda self: self._slam())

    def _zero_grads(self):
        for g in self.slam.shared_c.values():
            g.grad = None
        for p in self.slam._params:
            p.grad = None

    def _stepped_decoders(self):
        """Mapper.py:335-341"""
        d = self.slam.shared_decoders
        return ([] if self.fix_fine else [d.fine_decoder]) + ([] if self.fix_color else [d.color_decoder])

    def optimize_map(self, num_joint_iters, lr_factor, idx, cur_gt_color, cur_gt_depth):
        """Mapper.py:230-540.  The current pose is est[idx]; with BA the optimised poses go back into est[idx] and the keyframe
        pose table (one ``Trajectory.store`` launch per table)."""
        slam, mc, dev = self.slam, self.mc, self.device
        traj, kf_est, keyframe_list = slam.traj, slam.kf_est, slam.keyframe_list
        n_kf = len(keyframe_list)
        cur_c2w = traj.est[idx]
        if n_kf == 0:                                                                   # Mapper.py:256-265
            optimize_frame = []
        elif self.keyframe_selection_method == "global":
            optimize_frame = random_select(n_kf - 1, self.mapping_window_size - 2, self.rng)
        else:
            optimize_frame = slam.kf_sel.keyframe_selection_overlap(cur_gt_color, cur_gt_depth, cur_c2w,
                                                                    [{"est_c2w": kf_est[k]} for k in range(n_kf - 1)],
                                                                    self.mapping_window_size - 2)
        optimize_frame = [int(f) for f in optimize_frame]
        oldest_frame = None
        if n_kf > 0:                                                                    # Mapper.py:267-272
            optimize_frame = optimize_frame + [n_kf - 1]
            oldest_frame = min(optimize_frame)
        optimize_frame += [-1]
        if self.save_selected_keyframes_info:                                           # Mapper.py:274-287
            self.selected_keyframes[idx] = [
                {"idx": keyframe_list[f] if f != -1 else idx,
                 "gt_c2w": (traj.gt[keyframe_list[f]] if f != -1 else traj.gt[idx]).cpu(),
                 "est_c2w": (kf_est[f] if f != -1 else cur_c2w).cpu()} for f in optimize_frame]
        pixs_per_image = self.mapping_pixels // len(optimize_frame)

        c = slam.shared_c
        if self.coarse_mapper:
            keys, masks = ("grid_coarse",), None
        else:
            keys = tuple(k for k in ("grid_middle", "grid_fine", "grid_color") if k in c)
            masks = None
            if self.frustum_feature_selection:                                          # Mapper.py:315-318, once per call
                masks = {k: slam.frustum.voxel_mask(cur_c2w, k, c[k].shape[2:], cur_gt_depth) for k in keys}
        gopt = MaskedGridAdam({k: c[k] for k in keys}, masks, capturable=True)

        BA = self.BA and not self.coarse_mapper
        cam_all, cam_of = None, {}
        if BA:                                                                          # Mapper.py:346-363: every optimised pose is a row of ONE
            rows = [f for f in optimize_frame if f != oldest_frame]                     # [n, 7] parameter (Adam is elementwise)
            cam_of = {f: i for i, f in enumerate(rows)}
            poses = torch.stack([kf_est[f] if f != -1 else cur_c2w for f in rows])
            cam_all = get_tensor_from_camera(poses).requires_grad_(True)
        dec = [] if self.coarse_mapper else self._stepped_decoders()
        entries = dec + ([cam_all] if BA else [])
        opt = FlatAdam(entries, lr=0.0) if entries else None                            # Mapper.py:365-379, the dense rest
        data = [(f, slam.keyframe_dict[f]["depth"], slam.keyframe_dict[f]["color"], kf_est[f]) if f != -1 else
                (f, cur_gt_depth, cur_gt_color, cur_c2w) for f in optimize_frame]
        loss_buf = torch.zeros(1, dtype=torch.float64, device=dev)
        lrs = [0.0] * len(entries)

        def iteration(stage):                                                           # Mapper.py:430-519
            if opt is not None:
                opt.zero_grad(set_to_none=True)
            self._zero_grads()
            poses = get_camera_from_tensor(cam_all).unbind(0) if BA else ()
            fr = [(poses[cam_of[f]] if f in cam_of else c2w, d, col) for f, d, col, c2w in data]
            loss = mapping_loss(slam.renderer, c, slam.shared_decoders, fr, pixs_per_image, stage, w_color=self.w_color_loss,
                                coarse_mapper=self.coarse_mapper)
            backward(loss)
            if opt is not None:
                opt.step(lr=lrs)
            st = mc["stage"][stage]
            with torch.no_grad():
                gopt.step({k: st[k[len("grid_"):] + "_lr"] * lr_factor for k in keys})
            loss_buf.copy_(loss.detach().reshape(1))

        vis = self.visualizer                                                           # Mapper.py:426-428, before joint_iter's step
        draws = vis is not None and not (idx == 0 and self.no_vis_on_first_frame) and bool(vis.due_iters(idx, num_joint_iters))

        def figure(joint_iter):
            if draws:
                vis.vis(idx, joint_iter, cur_gt_depth, cur_gt_color, cur_c2w, c, slam.shared_decoders)

        n, done = int(num_joint_iters), 0
        if self.coarse_mapper:                                                          # Mapper.py:403-410
            plan = (("coarse", n),)
        else:
            n_mid = min(n, int(n * self.middle_iter_ratio) + 1)
            n_fine = max(0, min(n, int(n * self.fine_iter_ratio) + 1) - n_mid)
            plan = (("middle", n_mid), ("fine", n_fine), ("color", n - n_mid - n_fine))
        for stage, cnt in plan:
            if cnt <= 0:
                continue
            for i in range(len(dec)):
                lrs[i] = mc["stage"][stage]["decoders_lr"] * lr_factor                  # Mapper.py:412
            if BA:
                lrs[-1] = self.BA_cam_lr if stage == "color" else 0.0                   # Mapper.py:417-419
            figure(done)
            iteration(stage)                                                            # eager: also initialises optimiser state
            if cnt > 3:                                                                 # one graph per stage, the rest are replays
                torch.cuda.synchronize(dev)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    iteration(stage)
                for j in range(1, cnt):
                    figure(done + j)
                    graph.replay()
                del graph
            else:
                for j in range(1, cnt):
                    figure(done + j)
                    iteration(stage)
            done += cnt
            slam.counters["coarse_iters" if self.coarse_mapper else "mapping_iters"] += cnt
            if not self.coarse_mapper:
                slam.counters["mapping_rays"] += cnt * pixs_per_image * len(optimize_frame)
        self.last_loss = float(loss_buf.item())                                         # the call's one read of the loss
        if BA:                                                                          # Mapper.py:521-538
            kf_rows = [f for f in cam_of if f != -1]
            with torch.no_grad():
                if kf_rows:
                    traj.store(cam_all.detach()[:len(kf_rows)].contiguous(), torch.tensor(kf_rows, dtype=torch.int64, device=dev), kf_est)
                traj.store(cam_all.detach()[cam_of[-1]:cam_of[-1] + 1].contiguous(), traj.idx)
        self._zero_grads()


# --------------------------------------------------------------------------------------------------
# the system (src/NICE_SLAM.py)
# --------------------------------------------------------------------------------------------------
class NICE_SLAM:
    """src/NICE_SLAM.py:26-98,252-305 in one process.  ``args`` needs ``input_folder``, ``output`` and ``nice``.

    ``decoders``: "pretrained" (``cfg['pretrained_decoders']``; a missing file is an error) or "random" (the initialisation
    of ``nice_slam_amd.NICE``).  ``frames``: stop after that many frames of the sequence.  ``dataset``: a frame reader to use
    instead of ``get_dataset`` (``len``, ``ds[i] -> (i, colour, depth, c2w)`` on the device, ``ds.poses``), e.g. frames held in
    memory.  ``sync_timers``: wait for the device after each tracked and each mapped frame, so that ``timers`` hold device time
    too and ``track_frame_s`` lists every tracked frame (a measurement aid; off, a tracked frame never waits)."""

    def __init__(self, cfg, args, decoders: str = "pretrained", frames: Optional[int] = None, dataset=None, seed: int = 0,
                 sync_timers: bool = False):
        if decoders not in ("pretrained", "random"):
            raise ValueError("decoders: 'pretrained' or 'random'")
        self.cfg, self.args, self.nice = cfg, args, args.nice
        self.coarse, self.occupancy, self.low_gpu_mem = cfg["coarse"], cfg["occupancy"], cfg["low_gpu_mem"]
        self.verbose, self.dataset, self.scale = cfg["verbose"], cfg["dataset"], cfg["scale"]
        self.coarse_bound_enlarge = cfg["model"]["coarse_bound_enlarge"]
        self.seed, self.sync_timers = int(seed), sync_timers
        self.device = torch.device(cfg["mapping"]["device"])
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = (cfg["cam"][k] for k in ("H", "W", "fx", "fy", "cx", "cy"))
        self.update_cam()
        self.bound = load_bound(cfg, self.scale)
        self.renderer = Renderer(cfg, args, self)                   # (raises NotImplementedError for nice = False: iMAP*)
        if not torch.cuda.is_available() or self.device.type != "cuda":
            raise _capi.NsrError("nice_slam_amd needs the AMD GPU; there is no CPU path")
        if torch.device(cfg["tracking"]["device"]) != self.device:
            print(f"INFO: one process on one device: tracking.device {cfg['tracking']['device']} is ignored, everything runs on {self.device}")
        if cfg["sync_method"] != "strict":
            print(f"INFO: sync_method '{cfg['sync_method']}' runs as 'strict' (one process: a frame is tracked, then mapped)")
        self.output = cfg["data"]["output"] if args.output is None else args.output     # NICE_SLAM.py:38-45
        self.ckptsdir = os.path.join(self.output, "ckpts")
        os.makedirs(self.output, exist_ok=True)
        os.makedirs(self.ckptsdir, exist_ok=True)
        os.makedirs(os.path.join(self.output, "mesh"), exist_ok=True)

        m = cfg["model"]                                            # src/conv_onet/config.py:5-33
        self.shared_decoders = NICE(dim=cfg["data"]["dim"], c_dim=m["c_dim"], coarse=cfg["coarse"], coarse_grid_len=cfg["grid_len"]["coarse"],
                                    middle_grid_len=cfg["grid_len"]["middle"], fine_grid_len=cfg["grid_len"]["fine"],
                                    color_grid_len=cfg["grid_len"]["color"], pos_embedding_method=m["pos_embedding_method"])
        if decoders == "pretrained":
            load_pretrained(self.shared_decoders, cfg, "cpu")
        self.shared_decoders = self.shared_decoders.to(self.device)
        set_decoder_bounds(self.shared_decoders, self.bound, self.coarse_bound_enlarge)
        self.shared_c = {k: v.to(self.device).requires_grad_(True) for k, v in grid_init(cfg, self.bound).items()}
        self._params = list(self.shared_decoders.parameters())
        mc = cfg["mapping"]
        # the decoders the mapper steps (Mapper.py:335-341) are the only ones whose parameter gradients anyone reads
        self.renderer.decoder_grads = tuple(s for s, fixed in (("fine", mc["fix_fine"]), ("color", mc["fix_color"])) if not fixed)

        if dataset is None:
            folder = cfg["data"]["input_folder"] if getattr(args, "input_folder", None) is None else args.input_folder
            dataset = get_dataset(cfg, folder, self.scale, device=self.device, decoder=cfg["data"].get("decoder", "pil"))
        self.frame_reader = dataset
        self.n_img = len(dataset) if frames is None else max(1, min(int(frames), len(dataset)))
        self.traj = Trajectory(self.n_img, on(self.device))
        self.traj.gt.copy_(torch.stack([torch.as_tensor(p).float() for p in dataset.poses[:self.n_img]]))      # one upload for the run
        self.keyframe_list, self.keyframe_dict = [], []
        n_kf = self.n_img // max(1, int(mc["keyframe_every"])) + 3
        self.kf_est = torch.zeros((n_kf, 4, 4), dtype=torch.float32, device=self.device)     # est_c2w of the keyframes
        self.map_version = 0
        self.counters = {"tracking_iters": 0, "mapping_iters": 0, "coarse_iters": 0, "tracking_rays": 0, "mapping_rays": 0}
        self.timers = {"tracking_s": 0.0, "mapping_s": 0.0, "coarse_s": 0.0, "tracking_capture_s": 0.0, "load_s": 0.0, "log_s": 0.0, "mesh_s": 0.0}
        self.track_frame_s = []

        self.mesher = Mesher(cfg, args, self)
        self.frustum = FrustumSelector(self.bound, self.H, self.W, self.fx, self.fy, self.cx, self.cy)
        self.kf_sel = KeyframeSelector(self.H, self.W, self.fx, self.fy, self.cx, self.cy)
        self.mapper = Mapper(self, coarse_mapper=False)
        self.coarse_mapper = Mapper(self, coarse_mapper=True) if self.coarse else None
        self.tracker = Tracker(self)
        self.every_frame, self.keyframe_every = int(mc["every_frame"]), int(mc["keyframe_every"])
        self.mesh_freq, self.ckpt_freq = int(mc["mesh_freq"]), int(mc["ckpt_freq"])
        if self.verbose:
            print(f"INFO: The output folder is {self.output}")
            print(f"INFO: The mesh can be found under {self.output}/mesh/")
            print(f"INFO: The checkpoint can be found under {self.output}/ckpts/")

    def update_cam(self):
        """NICE_SLAM.py:113-135: crop_size, then crop_edge"""
        cam = self.cfg["cam"]
        if "crop_size" in cam:
            crop_size = cam["crop_size"]
            sx, sy = crop_size[1] / self.W, crop_size[0] / self.H
            self.fx, self.fy, self.cx, self.cy = sx * self.fx, sy * self.fy, sx * self.cx, sy * self.cy
            self.W, self.H = crop_size[1], crop_size[0]
        if cam["crop_edge"] > 0:
            self.H -= cam["crop_edge"] * 2
            self.W -= cam["crop_edge"] * 2
            self.cx -= cam["crop_edge"]
            self.cy -= cam["crop_edge"]

    # ---- Logger.log (src/utils/Logger.py:21-35)
    def log(self, idx):
        path = os.path.join(self.ckptsdir, "{:05d}.tar".format(idx))
        torch.save({"c": {k: v.detach().cpu() for k, v in self.shared_c.items()},
                    "decoder_state_dict": {k: v.detach().cpu() for k, v in self.shared_decoders.state_dict().items()},
                    "gt_c2w_list": self.traj.gt.cpu(),
                    "estimate_c2w_list": self.traj.est.cpu(),
                    "keyframe_list": list(self.keyframe_list),
                    "selected_keyframes": self.mapper.selected_keyframes if self.mapper.save_selected_keyframes_info else None,
                    "idx": int(idx)}, path)
        if self.verbose:
            print("Saved checkpoints at", path)

    def _mesh(self, name, idx, show_forecast, use_all_frames=False):
        path = os.path.join(self.output, "mesh", name)
        self.mesher.get_mesh(path, self.shared_c, self.shared_decoders, self.keyframe_dict, self.traj.est, idx, self.device,
                             show_forecast=show_forecast, clean_mesh=self.cfg["meshing"]["clean_mesh"],
                             get_mask_use_all_frames=use_all_frames, mesh_bound="frames")
        return path

    # ---- Mapper.run, one frame (Mapper.py:572-654)
    def map_frame(self, idx, color, depth, first: bool):
        mc, mapper = self.cfg["mapping"], self.mapper
        t0 = time.perf_counter()
        lr_factor = mc["lr_first_factor"] if first else mc["lr_factor"]
        num_joint_iters = mc["iters_first"] if first else mc["iters"]
        outer_joint_iters = 1
        if not first and idx == self.n_img - 1 and mc["color_refine"]:      # Mapper.py:578-586: the colour refinement of the last frame
            outer_joint_iters = 5
            mapper.mapping_window_size *= 2
            mapper.middle_iter_ratio = mapper.fine_iter_ratio = 0.0
            num_joint_iters *= 5
            mapper.fix_color = True
            mapper.frustum_feature_selection = False
        iters = num_joint_iters // outer_joint_iters
        for outer in range(outer_joint_iters):
            mapper.BA = len(self.keyframe_list) > 4 and mc["BA"]                             # Mapper.py:602-603
            mapper.optimize_map(iters, lr_factor, idx, color, depth)
            if self.sync_timers:
                torch.cuda.synchronize(self.device)
            t1 = time.perf_counter()
            if outer == 0 and self.coarse_mapper is not None:       # the coarse level: its own process in the reference, one call per frame
                self.coarse_mapper.optimize_map(mc["iters_first"] if first else mc["iters"], lr_factor, idx, color, depth)
                if self.sync_timers:
                    torch.cuda.synchronize(self.device)
                self.timers["coarse_s"] += time.perf_counter() - t1
                t0 += time.perf_counter() - t1
            if outer == outer_joint_iters - 1:                      # Mapper.py:612-617
                if (idx % self.keyframe_every == 0 or idx == self.n_img - 2) and idx not in self.keyframe_list:
                    k = len(self.keyframe_list)
                    self.kf_est[k].copy_(self.traj.est[idx])
                    self.keyframe_list.append(idx)
                    self.keyframe_dict.append({"gt_c2w": self.traj.gt[idx].cpu(), "idx": idx, "color": color, "depth": depth,
                                               "est_c2w": self.kf_est[k]})
        self.map_version += 1
        self.timers["mapping_s"] += time.perf_counter() - t0
        t2 = time.perf_counter()
        if (not (idx == 0 and mc["no_log_on_first_frame"]) and idx % self.ckpt_freq == 0) or idx == self.n_img - 1:     # Mapper.py:627-631
            self.log(idx)
        t3 = time.perf_counter()
        self.timers["log_s"] += t3 - t2
        mg = self.cfg["meshing"]
        if idx % self.mesh_freq == 0 and not (idx == 0 and mc["no_mesh_on_first_frame"]):                                # Mapper.py:636-640
            self._mesh(f"{idx:05d}_mesh.ply", idx, mg["mesh_coarse_level"])
        if idx == self.n_img - 1:                                                                                        # Mapper.py:642-653
            final = self._mesh("final_mesh.ply", idx, mg["mesh_coarse_level"])
            if os.path.exists(final):
                shutil.copyfile(final, os.path.join(self.output, "mesh", f"{idx:05d}_mesh.ply"))
            if mg["eval_rec"]:
                self._mesh("final_mesh_eval_rec.ply", idx, False, use_all_frames=True)
        self.timers["mesh_s"] += time.perf_counter() - t3

    def run(self) -> dict:
        """Tracker.run + Mapper.run under strict synchronisation (Tracker.py:152-256, Mapper.py:542-657) -> the result dict"""
        np.random.seed(self.seed)                                   # the keyframe permutations (Mapper.py:227, common.py:208)
        t_run = time.perf_counter()
        for idx in range(self.n_img):
            t0 = time.perf_counter()
            _, color, depth, _ = self.frame_reader[idx]
            t1 = time.perf_counter()
            self.timers["load_s"] += t1 - t0
            self.tracker.track(idx, color, depth)
            if self.sync_timers:
                torch.cuda.synchronize(self.device)
            cap, self._cap_seen = self.timers["tracking_capture_s"] - getattr(self, "_cap_seen", 0.0), self.timers["tracking_capture_s"]
            dt = time.perf_counter() - t1 - cap                     # the one-time capture of the frame's graph is reported apart
            self.timers["tracking_s"] += dt
            if idx > 0 and cap == 0.0:
                self.track_frame_s.append(dt)
            if idx % self.every_frame == 0 or idx == self.n_img - 1:                         # Mapper.py:552-556
                if self.verbose:
                    print("Mapping Frame ", idx)
                self.map_frame(idx, color, depth, first=(idx == 0))
        torch.cuda.synchronize(self.device)
        res = self.result()
        res["wall_s"] = round(time.perf_counter() - t_run, 3)
        self.release()
        return res

    def release(self):
        """Destroy the tracker's captured graph now.  A hipGraph must not be destroyed while some stream of the process is
        capturing; one that waits for Python's cycle collector can meet exactly that (the collector runs at any allocation, a
        later run's capture included).  So the runner's objects form no reference cycle -- the tracker and the mappers hold
        weak references to the system -- and the graph goes when the run ends or the system is dropped, whichever is first."""
        ft = self.tracker._ft
        if ft is not None and ft["graph"] is not None:
            torch.cuda.synchronize(self.device)
            ft["graph"] = None
            self.tracker._ft = None

    def result(self) -> dict:
        est, gt = self.traj.est.cpu().numpy(), self.traj.gt.cpu().numpy()
        res = {"ate": ate_rmse(list(est), list(gt)), "n_img": self.n_img, "output": self.output,
               "keyframe_list": [int(k) for k in self.keyframe_list]}
        res.update(self.counters)
        res.update({k: round(v, 4) for k, v in self.timers.items()})
        return res


# --------------------------------------------------------------------------------------------------
# run.py
# --------------------------------------------------------------------------------------------------
def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m nice_slam_amd.slam", description="Run NICE-SLAM on a sequence from its config (run.py).")
    ap.add_argument("config", type=str, help="the scene's YAML config")
    ap.add_argument("--default", type=str, default=None, help="the default config the chain ends in (run.py: configs/nice_slam.yaml)")
    ap.add_argument("--input_folder", type=str, default=None, help="overrides data.input_folder")
    ap.add_argument("--output", type=str, default=None, help="overrides data.output")
    ap.add_argument("--random-decoders", action="store_true", help="do not load cfg['pretrained_decoders']")
    ap.add_argument("--frames", type=int, default=None, help="stop after N frames")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    default = a.default
    if default is None:
        cand = _resolve(os.path.join("configs", "nice_slam.yaml"), a.config)
        default = cand if os.path.exists(cand) else None
    cfg = load_config(a.config, default)
    args = types.SimpleNamespace(config=a.config, input_folder=a.input_folder, output=a.output, nice=True)
    torch.manual_seed(a.seed)
    slam = NICE_SLAM(cfg, args, decoders="random" if a.random_decoders else "pretrained", frames=a.frames, seed=a.seed)
    res = slam.run()
    res["metric"] = "ATE RMSE [cm]"
    res["value"] = res["ate"]["rmse"] * 100
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
