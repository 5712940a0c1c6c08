"""Camera poses of a run on the device (csrc/nsr_pose.h).

get_tensor_from_camera : src/common.py:179-201 (the inverse of get_camera_from_tensor; Shepperd's branches instead of mathutils)
Trajectory             : estimate_c2w_list / gt_c2w_list / idx of src/NICE_SLAM.py:70-76 in device memory, with the tracker's
                         motion model (src/Tracker.py:192-201), its choice of the best iteration (:224,245-247) and the
                         mapper's bundle-adjustment write-back (src/Mapper.py:527-541) as one launch each

Everything goes through an ``Engine``: the product's on the GPU, or one on the emulator library in the CPU tests.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, gpu

__all__ = ["get_tensor_from_camera", "Trajectory"]


def _f32(E: Engine, t) -> torch.Tensor:
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.detach().to(E.device, torch.float32).contiguous()


def get_tensor_from_camera(RT, Tquad: bool = False, engine: Optional[Engine] = None) -> torch.Tensor:
    """Drop-in for src/common.py:179-201: a (3,4) or (4,4) pose, or a batch (B,3,4) / (B,4,4), tensor or array -> the fp32
    7-vector ``[quaternion (w,x,y,z) | T]`` (``Tquad``: ``[T | quaternion]``), (7,) or (B,7), on the input's device.  One
    launch, nothing is read back; the quaternion's sign is the Shepperd branch's (``quad2rotation`` is even in it)."""
    E = engine if engine is not None else gpu()
    src = RT if isinstance(RT, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(RT))
    if src.dim() not in (2, 3) or tuple(src.shape[-2:]) not in ((3, 4), (4, 4)):
        raise _capi.NsrError(f"get_tensor_from_camera: expected (3,4), (4,4) or a batch of them, got {tuple(src.shape)}")
    rt = _f32(E, src).reshape(-1, src.shape[-2] * 4)
    cam = torch.empty((rt.shape[0], 7), dtype=torch.float32, device=E.device)
    with E.guard():
        E.call("nsr_tensor_from_camera", rt.data_ptr(), rt.shape[0], rt.shape[1], cam.data_ptr())
    if Tquad:
        cam = torch.cat([cam[:, 4:], cam[:, :4]], 1)
    cam = cam[0] if src.dim() == 2 else cam
    return cam if cam.device == src.device else cam.to(src.device)


class Trajectory:
    """``est`` and ``gt`` [N,4,4] fp32 and the frame index ``idx`` (int64 [1]) on the engine's device.  ``predict``, ``commit``
    and ``store`` read the index from device memory, so a graph captured around them serves every frame; none of them
    reads anything back."""

    def __init__(self, n_frames: int, engine: Optional[Engine] = None):
        self.E = engine if engine is not None else gpu()
        self.n = int(n_frames)
        if self.n < 1:
            raise ValueError("Trajectory: at least one frame")
        dev = self.E.device
        self.est = torch.zeros((self.n, 4, 4), dtype=torch.float32, device=dev)
        self.gt = torch.zeros((self.n, 4, 4), dtype=torch.float32, device=dev)
        self.idx = torch.zeros((1,), dtype=torch.int64, device=dev)

    def __len__(self):
        return self.n

    def set_index(self, i: int):
        if not 0 <= int(i) < self.n:
            raise IndexError(f"Trajectory: frame {i} of {self.n}")
        self.idx.fill_(int(i))

    def set_gt(self, i: int, c2w, copy_to_est: bool = False):
        """gt[i] := c2w (src/Tracker.py:161); ``copy_to_est``: est[i] as well (frame 0 and ``gt_camera``, :180-183)"""
        self.gt[i].copy_(_f32(self.E, c2w))
        if copy_to_est:
            self.est[i].copy_(self.gt[i])

    def _cam(self, cam, rows=None):
        ok = isinstance(cam, torch.Tensor) and cam.dtype is torch.float32 and cam.device == self.E.device and cam.is_contiguous() \
            and cam.shape[-1] == 7 and (cam.dim() == 1 if rows is None else cam.dim() == 2)
        if not ok:
            raise _capi.NsrError("Trajectory: camera tensors are contiguous fp32 [7] / [m, 7] on the trajectory's device")
        return cam

    def predict(self, cam: torch.Tensor, const_speed: bool = True):
        """cam [7] := the tracker's initial pose of frame ``idx`` (src/Tracker.py:192-201), est[idx] := its 4x4"""
        E = self.E
        self._cam(cam)
        with torch.no_grad(), E.guard():
            E.call("nsr_pose_predict", self.est.data_ptr(), self.n, self.idx.data_ptr(), 1 if const_speed else 0, cam.data_ptr())

    def commit(self, hist: torch.Tensor, best: Optional[torch.Tensor] = None):
        """est[idx] := the pose of the row of ``hist`` [n_iters, 8] (loss | cam) with the smallest loss (src/Tracker.py:224,
        245-247); no row below 1e10: est[idx] keeps the prediction.  ``best`` [8]: the taken row."""
        E = self.E
        if hist.dtype is not torch.float32 or hist.dim() != 2 or hist.shape[1] != 8 or not hist.is_contiguous() or hist.device != E.device:
            raise _capi.NsrError("Trajectory.commit: hist is contiguous fp32 [n_iters, 8] on the trajectory's device")
        if best is not None and (best.dtype is not torch.float32 or best.numel() != 8 or not best.is_contiguous() or best.device != E.device):
            raise _capi.NsrError("Trajectory.commit: best is contiguous fp32 [8] on the trajectory's device")
        with torch.no_grad(), E.guard():
            E.call("nsr_pose_commit", hist.data_ptr(), hist.shape[0], self.est.data_ptr(), self.n, self.idx.data_ptr(),
                   best.data_ptr() if best is not None else None)

    def ate(self, out: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
        """The absolute trajectory error of the frames ``0..idx`` (src/tools/eval_ate.py; ``idx`` is read on the device): the
        record of 32 doubles of include/nsr.h, rmse at [3].  With ``out`` (contiguous fp64 [32] on the trajectory's device)
        nothing is allocated and nothing is read back: the call can sit in a captured graph."""
        from .trajeval import REC, _launch
        E = self.E
        if out is None:
            out = torch.empty((REC,), dtype=torch.float64, device=E.device)
        elif out.dtype is not torch.float64 or out.numel() != REC or not out.is_contiguous() or out.device != E.device:
            raise _capi.NsrError("Trajectory.ate: out is contiguous fp64 [32] on the trajectory's device")
        _launch(E, self.est, self.gt, self.idx, scale, out)
        return out

    def store(self, cams: torch.Tensor, index: torch.Tensor, dst: Optional[torch.Tensor] = None):
        """dst[index[i]] := the 4x4 pose of cams[i] (src/Mapper.py:527-541); ``dst``: a [K,4,4] fp32 pose table on the
        device (default: ``est``); ``index``: int64 [m] on the device."""
        E = self.E
        dst = self.est if dst is None else dst
        cams = self._cam(cams.detach(), rows=True)
        if index.dtype is not torch.int64 or index.device != E.device or index.numel() != cams.shape[0] or not index.is_contiguous():
            raise _capi.NsrError("Trajectory.store: index is contiguous int64 [m] on the trajectory's device")
        if dst.dtype is not torch.float32 or dst.dim() != 3 or tuple(dst.shape[1:]) != (4, 4) or not dst.is_contiguous() or dst.device != E.device:
            raise _capi.NsrError("Trajectory.store: dst is contiguous fp32 [K, 4, 4] on the trajectory's device")
        with torch.no_grad(), E.guard():
            E.call("nsr_pose_store", cams.data_ptr(), cams.shape[0], index.data_ptr(), dst.data_ptr(), dst.shape[0])
