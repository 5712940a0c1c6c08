"""Overlap keyframe selection on the device (``Mapper.keyframe_selection_overlap``, src/Mapper.py:166-228).

The reference draws 100 pixels of the current frame, places 16 points on each ray, copies the 1600 points to the host and,
in a Python loop over the keyframes, inverts each pose with numpy, projects the points and counts those inside the image
less a 20-pixel border in front of the camera; then it sorts the keyframes by that share, drops the zeros and takes ``k``
of them through ``np.random.permutation``.  ``KeyframeSelector`` does the counting in one ``nsr_keyframe_overlap`` launch
and restates the host half (sort, filter, permutation, ``select_overlapping``) so that the selection and both RNG streams
match the reference's.

    self.kf_sel = KeyframeSelector(H, W, fx, fy, cx, cy)                              # Mapper.__init__
    optimize_frame = self.kf_sel.keyframe_selection_overlap(cur_gt_color, cur_gt_depth, cur_c2w, keyframe_dict[:-1], num)

A call costs one launch, at most one device-to-host copy of the poses not seen before (the inverses are cached per pose
tensor, by identity and ``_version``), one host-to-device copy of the K inverses and one device-to-host copy of the K counts.
"""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _capi, engine
from .common import _require_cuda
from .engine import w2c_rows

EDGE = 20                                          # Mapper.py:213


def t_vals(n_samples: int) -> np.ndarray:
    """torch.linspace(0, 1, n_samples) as the reference computes it: on the CPU, before ``.to(device)`` (Mapper.py:190)."""
    return np.ascontiguousarray(torch.linspace(0.0, 1.0, steps=int(n_samples)).numpy(), dtype=np.float32)


def select_overlapping(counts, n_points: int, k: int) -> list:
    """What the reference does with the per-keyframe shares (Mapper.py:218-227): share = count / n_points in fp64; keyframe ids
    ordered by share, largest first, ties kept in id order (a stable sort); the ids whose share is positive; the first k of
    ``np.random.permutation`` of them.  The permuted array is built from a Python list as the reference builds it (int64, or
    float64 when empty), so the numpy RNG advances by the same draws."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    share = [counts[i] / n_points for i in range(counts.shape[0])]
    by_share = sorted(range(len(share)), key=share.__getitem__, reverse=True)
    ids = [i for i in by_share if share[i] > 0.0]
    return list(np.random.permutation(np.array(ids))[:k])


class KeyframeSelector:
    """H, W, fx, fy, cx, cy: the cropped-frame intrinsics the mapper holds (Mapper.py:91)."""

    def __init__(self, H: int, W: int, fx: float, fy: float, cx: float, cy: float):
        self.H, self.W, self.fx, self.fy, self.cx, self.cy = int(H), int(W), float(fx), float(fy), float(cx), float(cy)
        self._t: Dict[int, np.ndarray] = {}
        self._inv: Dict[int, tuple] = {}           # id(pose tensor) -> (weakref, _version, w2c row [12] fp32)

    def _t_vals(self, n_samples: int) -> np.ndarray:
        t = self._t.get(n_samples)
        if t is None:
            t = self._t[n_samples] = t_vals(n_samples)
        return t

    def w2c_rows(self, est_c2ws) -> np.ndarray:
        """[K, 12] fp32: rows 0..2 of inv(est_c2w) per keyframe, each inverted in the pose's own dtype (``np.linalg.inv``,
        Mapper.py:200).  Tensor poses are cached by identity and ``_version``: only new or changed ones cross the bus, in
        one stacked copy per device.  The version counter sees in-place torch operations, not writes through ``.data`` or
        through a raw pointer (a kernel writing a pose in place): after such a write, pass a new tensor (the reference's
        mapper replaces ``est_c2w``, Mapper.py:531) or clear the cache (``self._inv = {}``)."""
        if isinstance(est_c2ws, (torch.Tensor, np.ndarray)) and np.ndim(est_c2ws) == 3:
            return w2c_rows(list(est_c2ws.detach().cpu().numpy() if isinstance(est_c2ws, torch.Tensor) else est_c2ws), None)[:len(est_c2ws)]
        poses: Sequence = list(est_c2ws)
        K = len(poses)
        out = np.zeros((K, 12), dtype=np.float32)
        cache: Dict[int, tuple] = {}
        miss: Dict[torch.device, List[int]] = {}
        host: Dict[int, np.ndarray] = {}
        for i, p in enumerate(poses):
            if isinstance(p, torch.Tensor):
                hit = self._inv.get(id(p)) or cache.get(id(p))
                if hit is not None and hit[0]() is p and hit[1] == p._version:
                    out[i] = hit[2]
                    cache[id(p)] = hit
                elif p.device.type == "cpu":
                    host[i] = p.detach().numpy()
                else:
                    miss.setdefault(p.device, []).append(i)
            else:
                host[i] = np.asarray(p)
        for dev, ids in miss.items():                 # one device-to-host copy of the poses per device
            stack = torch.stack([poses[i].detach() for i in ids]).cpu().numpy()
            for j, i in enumerate(ids):
                host[i] = stack[j]
        if host:
            ids = sorted(host)
            rows = w2c_rows([host[i] for i in ids], None)
            for j, i in enumerate(ids):
                out[i] = rows[j]
                p = poses[i]
                if isinstance(p, torch.Tensor):
                    cache[id(p)] = (weakref.ref(p), p._version, rows[j].copy())
        self._inv = cache                          # only the poses of this call stay cached
        return out

    def overlap(self, c2w, gt_depth: torch.Tensor, est_c2ws, N_samples: int = 16, pixels: int = 100, indices=None) -> torch.Tensor:
        """int32 [K] device tensor: per keyframe, the number of the pixels * N_samples points of the current frame that it
        sees (the reference's ``percent_inside`` times pixels * N_samples).  ``c2w``: the current pose (3x4 or 4x4);
        ``gt_depth``: (H, W) device tensor; ``est_c2ws``: the K keyframe poses (a list of 4x4 tensors / arrays, or a [K,4,4]
        stack).  ``indices=None``: the pixels are drawn as get_samples draws them (one ``torch.randint(H*W, (pixels,))`` on
        the depth's device, common.py:99); else the given flat pixel indices are used."""
        _require_cuda(gt_depth, "KeyframeSelector: gt_depth")
        dev = gt_depth.device
        if tuple(gt_depth.shape) != (self.H, self.W):
            raise _capi.NsrError(f"KeyframeSelector: depth shape {tuple(gt_depth.shape)} != ({self.H}, {self.W})")
        if indices is None:
            indices = torch.randint(self.H * self.W, (int(pixels),), device=dev)
        else:
            indices = torch.as_tensor(indices).to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        w2c = self.w2c_rows(est_c2ws)
        K = w2c.shape[0]
        counts = torch.empty((K,), dtype=torch.int32, device=dev)
        if K == 0:
            return counts
        if isinstance(c2w, np.ndarray):
            c2w = torch.from_numpy(c2w)
        c2w = c2w.detach().to(device=dev, dtype=torch.float32).contiguous()
        if tuple(c2w.shape) not in ((3, 4), (4, 4)):
            raise _capi.NsrError(f"KeyframeSelector: c2w must be 3x4 or 4x4 (got {tuple(c2w.shape)})")
        depth = gt_depth.detach().to(torch.float32).contiguous()
        w2c_dev = torch.from_numpy(w2c).to(dev)
        tv = self._t_vals(int(N_samples))
        engine.on(dev).call("nsr_keyframe_overlap", indices.data_ptr(), int(indices.shape[0]), int(N_samples),
                            tv.ctypes.data_as(C.POINTER(C.c_float)), self.H, self.W, self.fx, self.fy, self.cx, self.cy, EDGE,
                            c2w.data_ptr(), c2w.stride(0), depth.data_ptr(), w2c_dev.data_ptr(), K, counts.data_ptr())
        return counts

    def keyframe_selection_overlap(self, gt_color, gt_depth, c2w, keyframe_dict, k, N_samples=16, pixels=100) -> list:
        """Drop-in for ``Mapper.keyframe_selection_overlap`` (Mapper.py:166-228): the same list (``numpy.int64`` ids, or [])
        for the same torch and numpy RNG states, which it leaves where the reference leaves them.  ``gt_color`` is unused,
        as in the reference's arithmetic."""
        counts = self.overlap(c2w, gt_depth, [kf["est_c2w"] for kf in keyframe_dict], N_samples, pixels)
        host = counts.cpu().numpy() if counts.numel() else np.zeros(0, dtype=np.int64)
        return select_overlapping(host, int(pixels) * int(N_samples), k)
