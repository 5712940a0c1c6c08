"""NICE-SLAM on a synthetic RGB-D sequence, end to end through the drop-in surface.

There is no dataset and there are no pretrained decoders in this environment, so the only way to obtain
a trajectory error is to generate a sequence: an analytic room (box + two cuboids, procedural texture) ray-cast along a
smooth camera path gives depth / colour / ground-truth poses.  The tracker and the mapper below restate the reference's
loops -- Tracker.run / optimize_cam_in_batch (src/Tracker.py:71-128,150-260) and Mapper.run / optimize_map /
keyframe_selection_overlap (src/Mapper.py:166-228,230-545,547-657), strict synchronisation, single process -- on top of
the product: get_samples, Renderer.render_batch_ray, NICE decoders, FrustumSelector and MaskedGridAdam.  The coarse-level
mapper (a separate process in the reference, src/NICE_SLAM.py:288-305; its grid is not read by the tracker's 'color' stage)
runs after each mapping call when ``coarse_mapper=True`` (the command line's default): 'global' keyframe selection,
stage 'coarse' throughout, no depth-guided samples, every coarse voxel optimised (Mapper.py:79-80,305-306,403-404,484).
Meshing, visualisation and the final colour refinement are not part of this loop.  Decoders are random-init (the reference loads pretrained
middle/fine decoders), so the absolute ATE is not comparable with published numbers; what it shows is that the hot path
carries a complete tracking + mapping run.

    python tools/slam_synthetic.py --frames 100            # on the GPU box; prints one JSON line

Defaults differ from Replica's in two places, both because nothing pretrained exists here: the mapper runs 300 iterations
every 2nd frame instead of 60 every 5th (with the reference's schedule the random-init decoders cannot absorb newly seen
regions fast enough and the trajectory drifts; `--map-iters 60 --every-frame 5` reproduces that), and keyframes are taken
every 10 frames because the sequence is 100 frames long, not 2000.

``MiniSLAM`` takes an ``ops`` object so that tests/test_slam_synthetic.py can drive the same loop on the CPU with the
oracle as the renderer (test infrastructure); ``ProductOps`` is the nice_slam_amd binding and has no CPU path.
"""
from __future__ import annotations

import argparse
import math
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ate import ate_rmse  # noqa: E402

# nice_slam.yaml / Replica/replica.yaml values (mapping.stage, tracking, rendering)
DEFAULT_CFG = {
    "tracking": {"ignore_edge_W": 20, "ignore_edge_H": 20, "use_color_in_tracking": True, "handle_dynamic": True,
                 "w_color_loss": 0.5, "const_speed_assumption": True, "lr": 0.001, "pixels": 200, "iters": 10},
    "mapping": {"middle_iter_ratio": 0.4, "fine_iter_ratio": 0.6, "every_frame": 5, "BA": True, "BA_cam_lr": 0.001,
                "keyframe_every": 50, "mapping_window_size": 5, "w_color_loss": 0.2, "lr_first_factor": 5, "lr_factor": 1,
                "pixels": 1000, "iters_first": 1500, "iters": 60,
                "stage": {"coarse": {"decoders_lr": 0.0, "coarse_lr": 0.001},
                          "middle": {"decoders_lr": 0.0, "middle_lr": 0.1, "fine_lr": 0.0, "color_lr": 0.0},
                          "fine": {"decoders_lr": 0.0, "middle_lr": 0.005, "fine_lr": 0.005, "color_lr": 0.0},
                          "color": {"decoders_lr": 0.005, "middle_lr": 0.005, "fine_lr": 0.005, "color_lr": 0.005}}},
}


# --------------------------------------------------------------------------------------------------------------------
# camera parametrisation (src/common.py:137-201)
# --------------------------------------------------------------------------------------------------------------------
def quad2rotation(q: torch.Tensor) -> torch.Tensor:
    qr, qi, qj, qk = q[0], q[1], q[2], q[3]
    two_s = 2.0 / (q * q).sum()
    return torch.stack([
        torch.stack([1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr)]),
        torch.stack([two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr)]),
        torch.stack([two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2)])])


def get_camera_from_tensor(t: torch.Tensor) -> torch.Tensor:
    """[quaternion (w,x,y,z), translation] -> 3x4 (common.py:163-176)."""
    return torch.cat([quad2rotation(t[:4]), t[4:, None]], 1)


def get_tensor_from_camera(c2w: torch.Tensor) -> torch.Tensor:
    """3x4 / 4x4 -> [quaternion (w,x,y,z), translation] (common.py:179-201; mathutils replaced by scipy)."""
    from scipy.spatial.transform import Rotation
    m = c2w.detach().cpu().double().numpy()
    x, y, z, w = Rotation.from_matrix(m[:3, :3]).as_quat()
    return torch.tensor([w, x, y, z, m[0, 3], m[1, 3], m[2, 3]], dtype=torch.float32, device=c2w.device)


def _cam_np(c2w) -> torch.Tensor:
    """get_tensor_from_camera for a pose on the host without scipy's object machinery (Shepperd's branches; the same quaternion
    up to sign, tests/test_slam_synthetic.py) -> 7 floats on the host."""
    m = np.asarray(c2w, dtype=np.float64)
    r00, r11, r22 = m[0, 0], m[1, 1], m[2, 2]
    t = r00 + r11 + r22
    if t > 0.0:
        s = 2.0 * math.sqrt(t + 1.0)
        q = (0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s)
    elif r00 > r11 and r00 > r22:
        s = 2.0 * math.sqrt(1.0 + r00 - r11 - r22)
        q = ((m[2, 1] - m[1, 2]) / s, 0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s)
    elif r11 > r22:
        s = 2.0 * math.sqrt(1.0 + r11 - r00 - r22)
        q = ((m[0, 2] - m[2, 0]) / s, (m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s)
    else:
        s = 2.0 * math.sqrt(1.0 + r22 - r00 - r11)
        q = ((m[1, 0] - m[0, 1]) / s, (m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s)
    n = math.sqrt(sum(v * v for v in q))
    return torch.tensor([q[0] / n, q[1] / n, q[2] / n, q[3] / n, m[0, 3], m[1, 3], m[2, 3]], dtype=torch.float32)


def _pose_np(t7) -> torch.Tensor:
    """get_camera_from_tensor + to44 for a pose on the host, in numpy (one frame's result; common.py:137-176)."""
    q = np.asarray(t7[:4], dtype=np.float64)
    w, x, y, z = q
    s = 2.0 / float(q @ q)
    m = np.eye(4)
    m[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    m[:3, 3] = t7[4:7]
    return torch.from_numpy(m.astype(np.float32))


def _inv44(c2w: torch.Tensor) -> torch.Tensor:
    """Inverse of a 4x4 pose on the HOST in numpy (what Mapper.py:196-197 does; torch.inverse on the GPU is a rocSOLVER call with
    a host synchronisation, measured at up to 0.9 s per call on some boxes) -> fp32 tensor on the host."""
    return torch.from_numpy(np.linalg.inv(to44(c2w.detach()).cpu().double().numpy()).astype(np.float32))


def to44(c2w: torch.Tensor) -> torch.Tensor:
    if c2w.shape[0] == 4:
        return c2w
    return torch.cat([c2w, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=c2w.dtype, device=c2w.device)], 0)


# --------------------------------------------------------------------------------------------------------------------
# synthetic sequence
# --------------------------------------------------------------------------------------------------------------------
class SyntheticSequence:
    """Room = inside of an axis-aligned box, plus solid cuboids; camera convention of the reference
    (common.py:82-88: dirs = ((i-cx)/fx, -(j-cy)/fy, -1), depth = z-depth = the ray parameter)."""

    def __init__(self, n_frames=100, H=240, W=320, device="cpu", room=((-2.0, 2.0), (-1.4, 1.4), (-2.0, 2.0)),
                 step_deg=0.9, seed=0):
        self.n, self.H, self.W, self.device = n_frames, H, W, torch.device(device)
        self.fx = self.fy = 0.5 * W
        self.cx, self.cy = (W - 1) / 2.0, (H - 1) / 2.0
        self.room = torch.tensor(room, dtype=torch.float32, device=self.device)
        self.boxes = torch.tensor([[[-1.9, -1.0], [-1.4, -0.5], [0.6, 1.7]],
                                   [[0.7, 1.6], [-1.4, -0.2], [-1.8, -0.9]],
                                   [[-0.4, 0.5], [-1.4, -0.9], [-0.3, 0.4]]], dtype=torch.float32, device=self.device)
        # scene bound handed to the SLAM system: the room with a margin (cfg['mapping']['bound'])
        self.bound_cfg = [[lo - 0.3, hi + 0.3] for lo, hi in room]
        rng = np.random.RandomState(seed)
        self.freq = torch.tensor(rng.uniform(2.0, 4.5, (3, 3)), dtype=torch.float32, device=self.device)
        self.phase = torch.tensor(rng.uniform(0, 6.28, (3,)), dtype=torch.float32, device=self.device)
        self.poses = [self._pose(k, step_deg) for k in range(n_frames)]
        ii, jj = torch.meshgrid(torch.arange(W, dtype=torch.float32, device=self.device),
                                torch.arange(H, dtype=torch.float32, device=self.device), indexing="xy")
        self.dirs = torch.stack([(ii - self.cx) / self.fx, -(jj - self.cy) / self.fy, -torch.ones_like(ii)], -1)   # (H,W,3)

    def _pose(self, k, step_deg):
        """Smooth path: the camera circles slowly around the room centre at radius 0.5 m, looking outwards-sideways,
        with a gentle vertical bob; ~1.5 cm and `step_deg` degrees per frame."""
        from scipy.spatial.transform import Rotation
        a = np.deg2rad(step_deg) * k
        pos = np.array([0.5 * np.cos(a), 0.15 * np.sin(2.3 * a), 0.5 * np.sin(a)])
        R = Rotation.from_euler("yxz", [-(a + 0.9), 0.12 * np.sin(1.7 * a), 0.05 * np.sin(1.1 * a)]).as_matrix()
        c2w = np.eye(4, dtype=np.float32)
        c2w[:3, :3], c2w[:3, 3] = R, pos
        return torch.tensor(c2w, device=self.device)

    def _texture(self, p, nrm_axis):
        base = 0.5 + 0.5 * torch.sin(p @ self.freq.T + self.phase)                       # smooth, position dependent
        checker = ((torch.floor(p[..., 0] * 2.0) + torch.floor(p[..., 1] * 2.0) + torch.floor(p[..., 2] * 2.0)) % 2.0)
        tint = torch.nn.functional.one_hot(nrm_axis, 3).float() * 0.25
        return (0.75 * base + 0.15 * checker[..., None] + tint).clamp(0.0, 1.0)

    def frame(self, k):
        """(color (H,W,3) fp32, depth (H,W) fp32, c2w 4x4) of frame k."""
        c2w = self.poses[k]
        d = self.dirs @ c2w[:3, :3].T                               # (H,W,3), z-depth parametrisation (not normalised)
        o = c2w[:3, 3]
        inv = 1.0 / torch.where(d.abs() < 1e-9, torch.full_like(d, 1e-9), d)
        # room: exit distance of a ray starting inside the box
        t_hi = (torch.where(d > 0, self.room[:, 1], self.room[:, 0]) - o) * inv
        t_room, ax_room = t_hi.min(-1)
        depth, axis = t_room, ax_room
        for b in self.boxes:                                        # solid cuboids: entry distance (slab test)
            t0, t1 = (b[:, 0] - o) * inv, (b[:, 1] - o) * inv
            tn, tf = torch.minimum(t0, t1), torch.maximum(t0, t1)
            t_in, ax_in = tn.max(-1)
            hit = (t_in < tf.min(-1)[0]) & (t_in > 0) & (t_in < depth)
            depth = torch.where(hit, t_in, depth)
            axis = torch.where(hit, ax_in, axis)
        p = o + d * depth[..., None]
        return self._texture(p, axis), depth.contiguous(), c2w


# --------------------------------------------------------------------------------------------------------------------
# the product binding
# --------------------------------------------------------------------------------------------------------------------
class ProductOps:
    """nice_slam_amd on an AMD GPU: channels-last grids, NICE decoders (random init), HIP renderer, fused grid Adam."""

    def __init__(self, seq: SyntheticSequence, device, seed=0, fused=False):
        import types
        import nice_slam_amd as nsa
        self.fused = fused           # mapping iterations through nice_slam_amd.mapping_loss, replayed from hipGraphs
        from nice_slam_amd.common import set_decoder_bounds
        self.nsa, self.device = nsa, torch.device(device)
        cfg = {"scale": 1, "occupancy": True, "coarse": True, "mapping": {"bound": seq.bound_cfg},
               "grid_len": {"coarse": 2.0, "middle": 0.32, "fine": 0.16, "color": 0.16, "bound_divisible": 0.32},
               "model": {"c_dim": 32, "coarse_bound_enlarge": 2},
               "rendering": {"lindisp": False, "perturb": 0.0, "N_samples": 32, "N_surface": 16, "N_importance": 0}}
        torch.manual_seed(seed)
        self.bound = nsa.load_bound(cfg)
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = seq.H, seq.W, seq.fx, seq.fy, seq.cx, seq.cy
        slam = types.SimpleNamespace(nice=True, bound=self.bound, H=seq.H, W=seq.W, fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        self.renderer = nsa.Renderer(cfg, None, slam)
        # This mapper only ever steps the colour decoder (like the reference with fix_fine: True, Mapper.py:335-341); the
        # reference's autograd nevertheless produces dW for the middle and fine decoders in every iteration and nobody reads
        # them.  Tell the renderer which parameter gradients are consumed: the other passes skip their dW work.
        self.renderer.decoder_grads = ("color",)
        self.decoders = nsa.NICE(coarse=True).to(self.device)
        set_decoder_bounds(self.decoders, self.bound, 2.0)
        self.c = {k: v.to(self.device).requires_grad_(True) for k, v in nsa.grid_init(cfg, self.bound).items()}
        self.selector = nsa.FrustumSelector(self.bound, seq.H, seq.W, seq.fx, seq.fy, seq.cx, seq.cy)
        self.bound_dev = self.bound.to(self.device)
        self._params = list(self.decoders.parameters())

    def update_tracker_copy(self):
        """The tracker renders from its OWN copy of the map, refreshed from the shared one before a frame is tracked
        (Tracker.update_para_from_mapping, src/Tracker.py:130-142: deepcopy of the decoders, clone of every grid).  Static
        buffers here, so that the captured tracking iteration keeps reading the same addresses."""
        if not hasattr(self, "c_track"):
            import copy
            self.c_track = {k: v.detach().clone(memory_format=torch.preserve_format) for k, v in self.c.items()}
            self.decoders_track = copy.deepcopy(self.decoders)
            for p in self.decoders_track.parameters():
                p.requires_grad_(False)                         # nothing steps them; the reference leaves requires_grad on and discards the grads
            self._track_copy_version = None                     # ... and run the refresh once now: the first multi-tensor copy
                                                                # loads its code object (~40-90 ms, measured), set-up like the capture
        if getattr(self, "_track_copy_version", None) == getattr(self, "map_version", 0):
            return                                              # the mapper did not run since the last refresh
        self._track_copy_version = getattr(self, "map_version", 0)
        with torch.no_grad():                                   # grids and decoder blobs in ONE multi-tensor copy
            dst = list(self.c_track.values()) + [m.flat_params() for m in self.decoders_track.children()]
            src = list(self.c.values()) + [m.flat_params() for m in self.decoders.children()]
            torch._foreach_copy_(dst, src)
        self.decoders_track.repack()                            # same packed buffers: the captured iteration reads the new weights

    def get_samples(self, H0, H1, W0, W1, n, c2w, depth, color):
        return self.nsa.get_samples(H0, H1, W0, W1, n, self.H, self.W, self.fx, self.fy, self.cx, self.cy, c2w, depth, color, self.device)

    def render(self, stage, rays_d, rays_o, gt_depth, gt_max=None):
        return self.renderer.render_batch_ray(self.c, self.decoders, rays_d, rays_o, self.device, stage, gt_depth=gt_depth,
                                              gt_max=gt_max)

    def keep_mask(self, rays_o, rays_d, gt_depth):
        """bounding-box pre-filter as a mask (nsr_aabb_keep): (keep, max depth over the kept rays)"""
        return self.nsa.aabb_keep(rays_o, rays_d, gt_depth, self.bound)

    def color_decoder_params(self):
        return list(self.decoders.color_decoder.parameters())

    def all_decoder_params(self):
        return list(self.decoders.parameters())

    def frustum_masks(self, c2w, depth):
        return {k: self.selector.voxel_mask(to44(c2w), k, v.shape[2:], depth) for k, v in self.c.items() if k != "grid_coarse"}

    def grid_optimizer(self, masks):
        keys = ("grid_middle", "grid_fine", "grid_color")
        return self.nsa.MaskedGridAdam({k: self.c[k] for k in keys}, masks)

    def zero_grads(self):
        for g in self.c.values():
            g.grad = None
        for p in self._params:                  # cached: Module.parameters() walks the module tree on every call
            p.grad = None


# --------------------------------------------------------------------------------------------------------------------
# tracker + mapper
# --------------------------------------------------------------------------------------------------------------------
class MiniSLAM:
    def __init__(self, ops, seq: SyntheticSequence, cfg=None, seed=0, verbose=False, gt_mapping_pose=False, coarse_mapper=False):
        self.ops, self.seq, self.cfg, self.verbose = ops, seq, cfg or DEFAULT_CFG, verbose
        self.coarse_mapper = coarse_mapper and getattr(ops, "fused", False)
        self.coarse_rng = np.random.RandomState(seed + 1)   # its own stream: the coarse mapper is its own process in the reference
        self.coarse_losses = []
        self.gt_mapping_pose = gt_mapping_pose          # diagnostic: the mapper sees ground-truth poses (isolates tracking)
        self.device = ops.device
        self.H, self.W = seq.H, seq.W
        self.est = [None] * seq.n
        self.gt = [None] * seq.n
        self.keyframe_list, self.keyframe_dict = [], []
        self.np_rng = np.random.RandomState(seed)
        self.counters = {"tracking_iters": 0, "mapping_iters": 0, "tracking_rays": 0, "mapping_rays": 0, "coarse_iters": 0}
        self.timers = {"tracking_s": 0.0, "mapping_s": 0.0, "coarse_s": 0.0, "tracking_capture_s": 0.0}

    # The reference drops the rays whose depth lies outside the bound by boolean-mask compaction (Tracker.py:95-104,
    # Mapper.py:471-481) and indexes its loss terms with further masks -- a host synchronisation each.  Here the batch
    # keeps its size: ops.keep_mask() gives the same mask plus the kept rays' maximum depth (the batch-global scalar of
    # the renderer), and every loss term is weighted by its mask.  Same loss, same gradients, no sync inside an iteration.

    # -- Tracker.optimize_cam_in_batch (Tracker.py:71-128)
    def _track_iter(self, cam, color, depth, opt):
        tc = self.cfg["tracking"]
        opt.zero_grad()
        c2w = get_camera_from_tensor(cam)
        He, We = tc["ignore_edge_H"], tc["ignore_edge_W"]
        o, d, gd, gc = self.ops.get_samples(He, self.H - He, We, self.W - We, tc["pixels"], c2w, depth, color)
        keep, kmax = self.ops.keep_mask(o, d, gd)
        self.ops.zero_grads()
        dep, unc, col = self.ops.render("color", d, o, gd, gt_max=kmax)
        unc = unc.detach()
        tmp = torch.abs(gd - dep) / torch.sqrt(unc + 1e-10)
        if tc["handle_dynamic"]:                       # median over the kept rays only, like the compacted batch
            med = torch.nanmedian(torch.where(keep, tmp.detach(), torch.full_like(tmp, float("nan"))))
            mask = (tmp < 10 * med) & (gd > 0) & keep
        else:
            mask = (gd > 0) & keep
        loss = torch.where(mask, tmp, torch.zeros_like(tmp)).sum()
        if tc["use_color_in_tracking"]:
            loss = loss + tc["w_color_loss"] * torch.where(mask[:, None], torch.abs(gc - col), torch.zeros_like(col)).sum()
        loss.backward()
        opt.step()
        opt.zero_grad()
        self.counters["tracking_iters"] += 1
        self.counters["tracking_rays"] += int(o.shape[0])
        return loss.detach()

    # -- the same iteration on the fused path: nice_slam_amd.tracking_loss (one autograd node) + capturable Adam, recorded ONCE
    # into a hipGraph; every later iteration of every frame is a replay (the frame, the pose and the optimiser state live in
    # static buffers that are refilled / zeroed per frame; per-iteration losses and poses go to device-side history slots).
    def _track_fused(self, init_cam, color, depth):
        """``init_cam``: the 7 pose parameters on the HOST.  Per frame: one small H2D copy, two image copies, two multi-tensor
        zero fills, ``iters`` graph replays, one D2H read of the history (the only synchronisation of the frame)."""
        tc, ops, nsa = self.cfg["tracking"], self.ops, self.ops.nsa
        n_it = tc["iters"]
        ft = getattr(self, "_ft", None)
        if ft is None:
            t_cap = time.perf_counter()
            ft = self._ft = {"cam": torch.zeros(7, device=self.device).requires_grad_(True), "depth": depth.clone(), "color": color.clone(),
                             "i": torch.zeros(1, dtype=torch.long, device=self.device),
                             "hist": torch.zeros((n_it, 8), dtype=torch.float32, device=self.device),    # loss | pose per iteration
                             "host": torch.zeros(7, dtype=torch.float32).pin_memory(),
                             "hist_host": torch.zeros((n_it, 8), dtype=torch.float32).pin_memory(), "graph": None}
            ft["opt"] = nsa.FlatAdam([ft["cam"]], lr=tc["lr"])    # Adam of the pose: one launch pair, step count on the device
        cam, opt = ft["cam"], ft["opt"]

        def reset():
            ft["host"].copy_(init_cam)
            with torch.no_grad():
                cam.copy_(ft["host"], non_blocking=True); ft["depth"].copy_(depth); ft["color"].copy_(color); ft["i"].zero_()
                opt.reset_state()                               # a fresh optimiser per frame (Tracker.py:214-222)

        def iteration():
            opt.zero_grad(set_to_none=True)
            c2w = nsa.get_camera_from_tensor(cam)                # one launch each way (src/common.py:137-176)
            loss = nsa.tracking_loss(ops.renderer, ops.c_track, ops.decoders_track, c2w, ft["depth"], ft["color"], tc["pixels"],
                                     tc["ignore_edge_H"], tc["ignore_edge_W"], w_color=tc["w_color_loss"],
                                     handle_dynamic=tc["handle_dynamic"], use_color=tc["use_color_in_tracking"])
            nsa.backward(loss)
            opt.step()
            with torch.no_grad():
                ft["hist"].index_copy_(0, ft["i"], torch.cat([loss.detach().reshape(1).float(), cam.detach()]).reshape(1, 8))
                ft["i"] += 1

        t_r = time.perf_counter()
        reset()
        self.timers["tracking_reset_s"] = self.timers.get("tracking_reset_s", 0.0) + time.perf_counter() - t_r   # host: frame hand-over
        if ft["graph"] is None:                                 # once per run: an eager iteration (optimiser state, code load), the
            iteration()                                         # capture; timed apart (timers["tracking_capture_s"])
            torch.cuda.synchronize()
            ft["graph"] = torch.cuda.CUDAGraph()                # all iterations of a frame in ONE graph: one launch per frame
            with torch.cuda.graph(ft["graph"]):
                for _ in range(n_it):
                    iteration()
            reset()
            torch.cuda.synchronize()
            self.timers["tracking_capture_s"] += time.perf_counter() - t_cap
        tp = self.timers
        t_a = time.perf_counter()
        ft["graph"].replay()
        t_b = time.perf_counter()
        self.counters["tracking_iters"] += n_it
        self.counters["tracking_rays"] += n_it * tc["pixels"]
        ft["hist_host"].copy_(ft["hist"], non_blocking=True)
        torch.cuda.current_stream().synchronize()               # Tracker.py:236-246, the one host read of the frame
        tp["tracking_launch_s"] = tp.get("tracking_launch_s", 0.0) + t_b - t_a              # host time of the graph launch
        tp["tracking_wait_s"] = tp.get("tracking_wait_s", 0.0) + time.perf_counter() - t_b   # the GPU running the iterations
        h = ft["hist_host"].numpy()
        k = int(np.argmin(h[:, 0]))
        return h[k, 1:].copy(), float(h[k, 0])

    # -- Tracker.run, one frame (Tracker.py:176-256)
    def track(self, idx, color, depth):
        tc, t_in = self.cfg["tracking"], time.perf_counter()
        pdev = torch.device("cpu") if getattr(self.ops, "fused", False) else self.device    # 4x4 pose algebra: on the host when
        pre = self.est[idx - 1].to(pdev).float()                                             # the iterations are graph replays
        if tc["const_speed_assumption"] and idx - 2 >= 0:
            # (fused: self.est lives on the host and the inverse is numpy's; the eager loops keep torch's, whose rounding the recorded
            #  reference distribution of tests/golden/ate_reference_ops.json was made with)
            delta = pre @ (_inv44(self.est[idx - 2]).to(pdev) if getattr(self.ops, "fused", False) else self.est[idx - 2].to(pdev).float().inverse())
            init = delta @ pre
        else:
            init = pre
        if getattr(self.ops, "fused", False) and tc["iters"] > 0:
            tp, t_a = self.timers, time.perf_counter()
            cam0 = _cam_np(init.numpy())
            t_b = time.perf_counter()
            first = not hasattr(self.ops, "c_track")
            self.ops.update_tracker_copy()                       # Tracker.update_para_from_mapping (Tracker.py:130-142)
            t_c = time.perf_counter()
            if first:                                            # the first call ALLOCATES the tracker's copy (deepcopy of the decoders):
                tp["tracking_capture_s"] += t_c - t_b            # one-time set-up, reported with the capture
                t_b = t_c
            best, self.last_track_loss = self._track_fused(cam0, color, depth)
            tp["tracking_pose_s"] = tp.get("tracking_pose_s", 0.0) + (t_b - t_a) + (t_a - t_in)    # host: motion model, quaternion
            tp["tracking_refresh_s"] = tp.get("tracking_refresh_s", 0.0) + t_c - t_b               # host: launching the map copy
            return _pose_np(best), init                          # 4x4 on the host
        cam = get_tensor_from_camera(init.detach()).to(self.device).requires_grad_(True)
        opt = torch.optim.Adam([cam], lr=tc["lr"])
        best, self.last_track_loss = cam.clone().detach(), float("nan")          # iters == 0: the motion-model prediction alone
        if tc["iters"] > 0:                              # Tracker.py:236-246: keep the pose of the smallest loss (one sync per frame)
            losses, cams = [], []
            for _ in range(tc["iters"]):
                losses.append(self._track_iter(cam, color, depth, opt))
                cams.append(cam.clone().detach())
            k = int(torch.argmin(torch.stack(losses)))
            best, self.last_track_loss = cams[k], float(losses[k])
        return to44(get_camera_from_tensor(best)), init

    # -- Mapper.keyframe_selection_overlap (Mapper.py:166-228)
    def _select_keyframes(self, color, depth, c2w, keyframes, k, n_samples=16, pixels=100):
        o, d, gd, _ = self.ops.get_samples(0, self.H, 0, self.W, pixels, c2w, depth, color)
        gd = gd.reshape(-1, 1).repeat(1, n_samples)
        tv = torch.linspace(0.0, 1.0, n_samples, device=self.device)
        z = gd * 0.8 * (1.0 - tv) + (gd + 0.5) * tv
        pts = (o[:, None, :] + d[:, None, :] * z[..., None]).reshape(-1, 3).detach()
        K = torch.tensor([[self.seq.fx, 0.0, self.seq.cx], [0.0, self.seq.fy, self.seq.cy], [0.0, 0.0, 1.0]], device=self.device)
        out = []
        for kid, kf in enumerate(keyframes):
            w2c = _inv44(kf["est_c2w"]).to(self.device) if getattr(self.ops, "fused", False) else torch.inverse(to44(kf["est_c2w"].to(self.device).float()))
            cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
            cam = cam * torch.tensor([-1.0, 1.0, 1.0], device=self.device)
            uv = cam @ K.T
            zc = uv[:, 2:] + 1e-5
            uv = uv[:, :2] / zc
            edge = 20
            m = (uv[:, 0] < self.W - edge) & (uv[:, 0] > edge) & (uv[:, 1] < self.H - edge) & (uv[:, 1] > edge) & (zc[:, 0] < 0)
            out.append((kid, float(m.float().mean())))
        out.sort(key=lambda t: t[1], reverse=True)
        sel = [kid for kid, pct in out if pct > 0.0]
        return [int(v) for v in self.np_rng.permutation(np.array(sel, dtype=np.int64))[:k]]

    # -- Mapper.optimize_map (Mapper.py:230-545)
    def optimize_map(self, n_iters, lr_factor, idx, color, depth, cur_c2w):
        mc = self.cfg["mapping"]
        ops = self.ops
        if len(self.keyframe_dict) == 0:
            frames = []
        else:
            frames = self._select_keyframes(color, depth, cur_c2w, self.keyframe_dict[:-1], mc["mapping_window_size"] - 2)
        oldest = None
        if len(self.keyframe_list) > 0:
            frames = frames + [len(self.keyframe_list) - 1]
            oldest = min(frames)
        frames = frames + [-1]
        pix = mc["pixels"] // len(frames)
        BA = len(self.keyframe_list) > 4 and mc["BA"]

        masks = ops.frustum_masks(cur_c2w, depth)                        # Mapper.py:315-318, once per call
        if getattr(ops, "fused", False):
            return self._optimize_map_fused(n_iters, lr_factor, color, depth, cur_c2w, frames, oldest, BA, pix, masks)
        opt_grid = ops.grid_optimizer(masks)
        dec_params = ops.color_decoder_params()
        groups = [{"params": dec_params, "lr": 0.0}]
        cams = []
        if BA:
            for f in frames:
                if f != oldest:
                    c2w = self.keyframe_dict[f]["est_c2w"] if f != -1 else cur_c2w
                    cams.append(get_tensor_from_camera(c2w.to(self.device)).requires_grad_(True))
            groups.append({"params": cams, "lr": 0.0})
        opt = torch.optim.Adam(groups)

        for it in range(n_iters):
            if it <= int(n_iters * mc["middle_iter_ratio"]):
                stage = "middle"
            elif it <= int(n_iters * mc["fine_iter_ratio"]):
                stage = "fine"
            else:
                stage = "color"
            st = mc["stage"][stage]
            opt.param_groups[0]["lr"] = st["decoders_lr"] * lr_factor
            if BA and stage == "color":
                opt.param_groups[1]["lr"] = mc["BA_cam_lr"]
            opt.zero_grad()
            ops.zero_grads()
            ro, rd, gds, gcs = [], [], [], []
            cam_id = 0
            for f in frames:
                if f != -1:
                    kf = self.keyframe_dict[f]
                    f_depth, f_color = kf["depth"].to(self.device), kf["color"].to(self.device)
                    if BA and f != oldest:
                        c2w = get_camera_from_tensor(cams[cam_id]); cam_id += 1
                    else:
                        c2w = kf["est_c2w"].to(self.device)
                else:
                    f_depth, f_color = depth, color
                    c2w = get_camera_from_tensor(cams[cam_id]) if BA else cur_c2w
                o, d, gd, gc = ops.get_samples(0, self.H, 0, self.W, pix, c2w, f_depth, f_color)
                ro.append(o.float()); rd.append(d.float()); gds.append(gd.float()); gcs.append(gc.float())
            o, d, gd, gc = torch.cat(ro), torch.cat(rd), torch.cat(gds), torch.cat(gcs)
            keep, kmax = ops.keep_mask(o, d, gd)
            dep, _, col = ops.render(stage, d, o, gd, gt_max=kmax)
            dm = keep & (gd > 0)
            loss = torch.where(dm, torch.abs(gd - dep), torch.zeros_like(dep)).sum()
            if stage == "color":
                loss = loss + mc["w_color_loss"] * torch.where(keep[:, None], torch.abs(gc - col), torch.zeros_like(col)).sum()
            loss.backward()
            opt.step()
            opt_grid.step({"grid_middle": st["middle_lr"] * lr_factor, "grid_fine": st["fine_lr"] * lr_factor,
                           "grid_color": st["color_lr"] * lr_factor})
            self.counters["mapping_iters"] += 1
            self.counters["mapping_rays"] += int(o.shape[0])
        self.last_map_loss = float(loss.item())                          # the only host read of the call

        if BA:                                                             # Mapper.py:527-541
            cam_id = 0
            for f in frames:
                if f != -1:
                    if f != oldest:
                        self.keyframe_dict[f]["est_c2w"] = to44(get_camera_from_tensor(cams[cam_id].detach())).clone()
                        cam_id += 1
                else:
                    cur_c2w = to44(get_camera_from_tensor(cams[-1].detach())).clone()
            return cur_c2w
        return None

    # -- the same call on the fused path: every iteration is ONE autograd node (nice_slam_amd.mapping_loss: window sampling +
    # render + loss) followed by capturable optimisers; per stage, the first iteration runs eagerly, is then recorded into a
    # hipGraph, and the remaining iterations of the stage are replays (no host work, no host-side scalars).
    def _optimize_map_fused(self, n_iters, lr_factor, color, depth, cur_c2w, frames, oldest, BA, pix, masks):
        mc, ops, nsa = self.cfg["mapping"], self.ops, self.ops.nsa
        keys = ("grid_middle", "grid_fine", "grid_color")
        gopt = nsa.MaskedGridAdam({k: ops.c[k] for k in keys}, masks, capturable=True)
        cam_all, cam_of = None, {}
        if BA:                                                           # every optimised pose is a row of ONE [n,7] parameter (Adam is
            rows = []                                                    # elementwise: same update as the reference's per-tensor list)
            for f in frames:
                if f != oldest:
                    c2w = self.keyframe_dict[f]["est_c2w"] if f != -1 else cur_c2w
                    cam_of[f] = len(rows)
                    rows.append(_cam_np(c2w.detach().cpu().numpy()))
            cam_all = torch.stack(rows).to(self.device).requires_grad_(True)     # one H2D copy for the window's poses
        # the dense rest of the reference's optimiser (decoder parameters + pose tensors, Mapper.py:368-387): one launch pair
        opt = nsa.FlatAdam([ops.decoders.color_decoder] + ([cam_all] if BA else []), lr=0.0)
        lrs = [0.0, 0.0]
        data = []
        for f in frames:
            if f != -1:
                kf = self.keyframe_dict[f]
                data.append((f, kf["depth"].to(self.device), kf["color"].to(self.device), kf["est_c2w"].to(self.device).float()))
            else:
                data.append((f, depth, color, cur_c2w.float()))
        loss_buf = torch.zeros(1, dtype=torch.float64, device=self.device)

        def iteration(stage):
            opt.zero_grad(set_to_none=True)
            ops.zero_grads()
            poses = nsa.get_camera_from_tensor(cam_all).unbind(0) if BA else ()     # one launch each way for the whole window
            fr = [(poses[cam_of[f]] if f in cam_of else c2w, d, c) for f, d, c, c2w in data]
            loss = nsa.mapping_loss(ops.renderer, ops.c, ops.decoders, fr, pix, stage, w_color=mc["w_color_loss"])
            nsa.backward(loss)
            opt.step(lr=lrs[:len(opt.entries)])
            st = mc["stage"][stage]
            with torch.no_grad():
                gopt.step({"grid_middle": st["middle_lr"] * lr_factor, "grid_fine": st["fine_lr"] * lr_factor,
                           "grid_color": st["color_lr"] * lr_factor})
            loss_buf.copy_(loss.detach().reshape(1))

        n_mid = min(n_iters, int(n_iters * mc["middle_iter_ratio"]) + 1)
        n_fine = max(0, min(n_iters, int(n_iters * mc["fine_iter_ratio"]) + 1) - n_mid)
        for stage, cnt in (("middle", n_mid), ("fine", n_fine), ("color", n_iters - n_mid - n_fine)):
            if cnt <= 0:
                continue
            lrs[0] = mc["stage"][stage]["decoders_lr"] * lr_factor
            lrs[1] = mc["BA_cam_lr"] if (BA and stage == "color") else 0.0
            iteration(stage)                                              # eager: also initialises optimiser state
            if cnt > 3:
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    iteration(stage)
                for _ in range(cnt - 1):
                    graph.replay()
                del graph
            else:
                for _ in range(cnt - 1):
                    iteration(stage)
            self.counters["mapping_iters"] += cnt
            self.counters["mapping_rays"] += cnt * pix * len(frames)
        self.last_map_loss = float(loss_buf.item())                      # the only host read of the call
        if BA:                                                             # Mapper.py:527-541; one D2H copy of all poses, 4x4s on the host
            cams = cam_all.detach().cpu().numpy()
            for f in frames:
                if f in cam_of and f != -1:
                    self.keyframe_dict[f]["est_c2w"] = _pose_np(cams[cam_of[f]])
            return _pose_np(cams[cam_of[-1]])
        return None

    # -- the coarse mapper's optimize_map (Mapper.py:230-545 with coarse_mapper=True): 'global' keyframe selection (:79-80,
    # 258-260), stage 'coarse' in every iteration (:403-404), no BA (:602-603), rendering without gt_depth (:484), the whole
    # coarse grid optimised at coarse_lr (:305-306,413).  Same execution scheme as _optimize_map_fused.
    def optimize_coarse(self, n_iters, lr_factor, color, depth, cur_c2w):
        mc, ops, nsa = self.cfg["mapping"], self.ops, self.ops.nsa
        frames = []
        if len(self.keyframe_dict) > 0:
            n_old = len(self.keyframe_dict) - 1
            frames = [int(v) for v in self.coarse_rng.permutation(n_old)[:mc["mapping_window_size"] - 2]]
            frames = frames + [len(self.keyframe_list) - 1]
        frames = frames + [-1]
        pix = mc["pixels"] // len(frames)
        fr = []
        for f in frames:
            if f != -1:
                kf = self.keyframe_dict[f]
                fr.append((kf["est_c2w"].to(self.device).float(), kf["depth"].to(self.device), kf["color"].to(self.device)))
            else:
                fr.append((cur_c2w.float(), depth, color))
        gopt = nsa.MaskedGridAdam({"grid_coarse": ops.c["grid_coarse"]}, None, capturable=True)
        lr = mc["stage"]["coarse"]["coarse_lr"] * lr_factor
        loss_buf = torch.zeros(2, dtype=torch.float64, device=self.device)

        def iteration(slot):
            ops.zero_grads()
            loss = nsa.mapping_loss(ops.renderer, ops.c, ops.decoders, fr, pix, "coarse", w_color=mc["w_color_loss"], coarse_mapper=True)
            nsa.backward(loss)
            with torch.no_grad():
                gopt.step({"grid_coarse": lr})
            loss_buf[slot:slot + 1].copy_(loss.detach().reshape(1))

        iteration(0)
        if n_iters > 3:
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                iteration(1)
            for _ in range(n_iters - 1):
                graph.replay()
            del graph
        else:
            for _ in range(n_iters - 1):
                iteration(1)
        self.counters["coarse_iters"] += n_iters
        first, last = (float(v) for v in loss_buf.tolist())
        self.coarse_losses.append((first, last))

    # -- Tracker.run + Mapper.run, strict synchronisation (Tracker.py:150-260, Mapper.py:547-657)
    def run(self):
        mc = self.cfg["mapping"]
        n = self.seq.n
        for idx in range(n):
            color, depth, gt_c2w = self.seq.frame(idx)
            color, depth, gt_c2w = color.to(self.device), depth.to(self.device), gt_c2w.to(self.device)
            self.gt[idx] = gt_c2w.cpu()
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            if idx == 0:
                self.est[0] = gt_c2w.cpu() if getattr(self.ops, "fused", False) else gt_c2w.clone()
            else:
                c2w, _ = self.track(idx, color, depth)
                self.est[idx] = c2w.detach()
                if self.verbose:
                    e = float((self.est[idx][:3, 3].cpu() - self.gt[idx][:3, 3]).norm())
                    print(f"[trk] frame {idx:4d} loss {self.last_track_loss:9.3f} pose err {e*100:6.2f} cm", file=sys.stderr)
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            cap, self._cap_seen = self.timers["tracking_capture_s"] - getattr(self, "_cap_seen", 0.0), self.timers["tracking_capture_s"]
            self.timers["tracking_s"] += t1 - t0 - cap         # the one-time capture of the tracker's graph is reported apart
            if idx % mc["every_frame"] == 0 or idx == n - 1:
                first = idx == 0
                cur = (gt_c2w if self.gt_mapping_pose else self.est[idx]).to(self.device)
                new = self.optimize_map(mc["iters_first"] if first else mc["iters"],
                                        mc["lr_first_factor"] if first else mc["lr_factor"], idx, color, depth, cur)
                self.ops.map_version = getattr(self.ops, "map_version", 0) + 1
                if new is not None:
                    self.est[idx] = new.detach()                     # (fused: already on the host)
                if self.device.type == "cuda":
                    torch.cuda.synchronize()
                t2 = time.perf_counter()
                self.timers["mapping_s"] += t2 - t1
                if self.coarse_mapper:                       # sees the same keyframe list the mapper just used
                    self.optimize_coarse(mc["iters_first"] if first else mc["iters"],
                                         mc["lr_first_factor"] if first else mc["lr_factor"], color, depth, self.est[idx].to(self.device))
                    torch.cuda.synchronize()
                    self.timers["coarse_s"] += time.perf_counter() - t2
                if (idx % mc["keyframe_every"] == 0 or idx == n - 2) and idx not in self.keyframe_list:
                    self.keyframe_list.append(idx)
                    self.keyframe_dict.append({"idx": idx, "color": color, "depth": depth, "gt_c2w": gt_c2w.cpu(),
                                               "est_c2w": self.est[idx].clone()})
                if self.verbose:
                    e = float((self.est[idx][:3, 3].cpu() - self.gt[idx][:3, 3]).norm())
                    print(f"[map] frame {idx:4d} loss {self.last_map_loss:9.3f} pose err {e*100:6.2f} cm", file=sys.stderr)
        return self.result()

    def result(self):
        est = [e.detach().cpu().numpy() for e in self.est]
        gt = [g.numpy() for g in self.gt]
        res = {"ate": ate_rmse(est, gt)}
        # reference point: the same sequence with tracking replaced by the constant-speed extrapolation alone
        res["raw_translation_error_cm"] = {"final": float(np.linalg.norm(est[-1][:3, 3] - gt[-1][:3, 3]) * 100),
                                           "mean": float(np.mean([np.linalg.norm(a[:3, 3] - b[:3, 3]) for a, b in zip(est, gt)]) * 100)}
        res["path_length_m"] = float(sum(np.linalg.norm(gt[i + 1][:3, 3] - gt[i][:3, 3]) for i in range(len(gt) - 1)))
        res.update(self.counters)
        res.update({k: round(v, 3) for k, v in self.timers.items()})
        if self.coarse_losses:
            res["coarse_loss_first_call"] = [round(v, 3) for v in self.coarse_losses[0]]
            res["coarse_loss_last_call"] = [round(v, 3) for v in self.coarse_losses[-1]]
        return res


def eval_render(ops, seq, est, every):
    """PSNR / SSIM / depth L1 of every ``every``-th frame re-rendered at its estimated pose (nice_slam_amd.evaluate_rendering)"""
    def frames():
        for k in range(0, seq.n, every):
            color, depth, _ = seq.frame(k)
            yield k, color, depth, est[k].to(ops.device).float()
    t0 = time.perf_counter()
    with torch.no_grad():
        ev = ops.nsa.evaluate_rendering(ops.renderer, ops.c, ops.decoders, frames(), stage="color", device=ops.device)
    torch.cuda.synchronize()
    out = {"every": every, "n_frames": ev["n_frames"], "n_no_depth": ev["n_no_depth"], "seconds": round(time.perf_counter() - t0, 3),
           "psnr": ev["mean"]["psnr"], "ssim": ev["mean"]["ssim"], "depth_l1_cm": ev["mean"]["depth_l1_cm"]}
    print(f"PSNR: {out['psnr']:.3f} dB  SSIM: {out['ssim']:.4f}  Depth L1: {out['depth_l1_cm']:.3f} cm  ({out['n_frames']} frames)", file=sys.stderr)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--iters-first", type=int, default=DEFAULT_CFG["mapping"]["iters_first"])
    ap.add_argument("--keyframe-every", type=int, default=10, help="reference: 50 (Replica sequences have 2000 frames)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--map-iters", type=int, default=300,
                    help="mapping iterations per mapped frame (reference: 60, with pretrained geometry decoders; the random-init "
                         "decoders of this environment need more -- with 60 / every 5th frame the run drifts, see profiles/)")
    ap.add_argument("--track-iters", type=int, default=DEFAULT_CFG["tracking"]["iters"])
    ap.add_argument("--every-frame", type=int, default=2, help="map every n-th frame (reference: 5)")
    ap.add_argument("--step-deg", type=float, default=0.9, help="camera rotation per frame")
    ap.add_argument("--no-ba", action="store_true")
    ap.add_argument("--no-coarse", action="store_true", help="skip the coarse-level mapper (fused path only)")
    ap.add_argument("--gt-mapping-pose", action="store_true", help="diagnostic: mapper uses ground-truth poses")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--unfused", action="store_true", help="mapping through get_samples / render_batch_ray / torch losses, eagerly (default: "
                                                            "nice_slam_amd.mapping_loss + capturable optimisers, replayed from hipGraphs)")
    ap.add_argument("--eval-render", type=int, default=0, metavar="N",
                    help="after the run, re-render every N-th frame at its estimated pose and report PSNR, SSIM and depth L1 "
                         "(nice_slam_amd.evaluate_rendering); 0: off")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    import copy
    cfg = copy.deepcopy(DEFAULT_CFG)
    cfg["mapping"]["iters_first"] = args.iters_first
    cfg["mapping"]["keyframe_every"] = args.keyframe_every
    cfg["mapping"]["iters"], cfg["mapping"]["every_frame"], cfg["mapping"]["BA"] = args.map_iters, args.every_frame, not args.no_ba
    cfg["tracking"]["iters"] = args.track_iters
    torch.manual_seed(args.seed)
    seq = SyntheticSequence(args.frames, args.height, args.width, device=dev, step_deg=args.step_deg, seed=args.seed)
    ops = ProductOps(seq, dev, seed=args.seed, fused=not args.unfused)
    slam = MiniSLAM(ops, seq, cfg, seed=args.seed, verbose=args.verbose, gt_mapping_pose=args.gt_mapping_pose,
                    coarse_mapper=not args.no_coarse)
    t0 = time.perf_counter()
    res = slam.run()
    torch.cuda.synchronize()
    res["wall_s"] = round(time.perf_counter() - t0, 2)
    res["config"] = {"frames": args.frames, "image": [args.height, args.width], "keyframe_every": args.keyframe_every,
                     "iters_first": args.iters_first, "map_iters": args.map_iters, "track_iters": args.track_iters,
                     "every_frame": args.every_frame, "BA": not args.no_ba, "mapping_path": "unfused, eager" if args.unfused else "fused + hipGraph replay", "step_deg": args.step_deg, "decoders": "random init (no pretrained weights in this environment)",
                     "grids": {k: list(v.shape[2:]) for k, v in ops.c.items()}}
    res["mapping_ms_per_iter"] = round(1e3 * res["mapping_s"] / max(1, res["mapping_iters"]), 4)
    res["tracking_ms_per_iter"] = round(1e3 * res["tracking_s"] / max(1, res["tracking_iters"]), 4)
    res["coarse_ms_per_iter"] = round(1e3 * res["coarse_s"] / max(1, res["coarse_iters"]), 4)
    res["metric"] = "ATE RMSE [cm] on a synthetic RGB-D sequence"
    res["value"] = res["ate"]["rmse"] * 100
    if args.eval_render > 0:
        res["render_eval"] = eval_render(ops, seq, slam.est, args.eval_render)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
