"""Host glue shared by the post-render modules (mesher, recon, bound, raster): the engine that drives libnsr.so on tensors of
one device, and the small conversions their entry points share (ctypes arrays, meshes, compaction, camera poses).

An ``Engine`` pairs a loaded library with a device, and ``Engine.call`` is how the package runs a library entry: on that
device, on its current stream.  The product runs the library on the GPU (``on(device)``, ``gpu()``); the CPU tests build an
engine on the emulator library (tests/emu/), which takes host pointers, and call the same module functions with ``engine=``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi
from .ply import read_mesh


class Engine:
    """Drives the entry points of a loaded library on tensors of one device."""

    def __init__(self, lib, device):
        self.lib = lib
        self.device = torch.device(device)
        self.index = self.device.index if self.device.type == "cuda" else None     # None: nothing to switch (the CPU emulator)

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == "cuda" else None

    def call(self, name, *args):
        """Run the entry point ``name`` on this device: ``args`` plus the device's current stream as the last argument, an error
        code raised as NsrError.  The library launches on the CURRENT device, so a caller working on tensors of another GPU of
        the process (the reference lets tracking and mapping name different devices, configs/nice_slam.yaml:31,44) gets the
        engine's made current for the call and its own back afterwards, exceptions included, like around a torch operator."""
        if self.index is None:
            self.lib.call(name, *args, self.stream())
        elif self.index == torch.cuda.current_device():
            self.lib.call(name, *args, torch.cuda.current_stream(self.device).cuda_stream)
        else:
            with self.guard():
                self.lib.call(name, *args, torch.cuda.current_stream(self.device).cuda_stream)

    def guard(self):
        return _capi.on_device(self.device if self.device.type == "cuda" else None)

    def tensor(self, a, dtype=None, what="points"):
        """[N, 3] contiguous tensor on this device (numpy and tensors of any device accepted; fp32 / fp64 kept)."""
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        if dtype is None:
            dtype = t.dtype if t.dtype in (torch.float32, torch.float64) else torch.float64
        t = t.detach().to(self.device, dtype).contiguous()
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{what} must be [N, 3] (got {tuple(t.shape)})")
        return t

    def faces(self, f):
        """[F, 3] contiguous int32 tensor on this device."""
        f = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f))
        f = f.detach().to(self.device)
        if f.dim() != 2 or f.shape[1] != 3:
            raise ValueError(f"faces must be [F, 3] (got {tuple(f.shape)})")
        return f.to(torch.int32).contiguous()

    def mesh(self, mesh):
        """(vertices fp64 [V, 3], faces int32 [F, 3]) on this device of a PLY path or a (vertices, faces) pair."""
        v, f = read_mesh(mesh) if isinstance(mesh, str) else (mesh[0], mesh[1])
        return self.tensor(v, torch.float64, "mesh vertices"), self.faces(f)

    def transform(self, pts: torch.Tensor, T):
        """pts fp64 [N, 3] on this device := R pts + t in place, (R | t) the top 3 x 4 of the pose T (nsr_transform_points)."""
        self.call("nsr_transform_points", pts.data_ptr(), pts.shape[0], c_doubles(np.asarray(T, np.float64)[:3, :4]))


_engines = {}
_gpu_engine = None


def on(device) -> Engine:
    """The product's engine of a CUDA device: libnsr.so there, one Engine per device ("cuda" without an index: the current one)."""
    E = _engines.get(device)
    if E is None:
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise _capi.NsrError(f"nice_slam_amd needs the AMD GPU (got {device}); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        E = _engines.get(device)
        if E is None:
            E = _engines[device] = Engine(_capi.get_lib(), device)
    return E


def gpu() -> Engine:
    """The product's engine on the device current at the first call."""
    global _gpu_engine
    if _gpu_engine is None:
        _gpu_engine = on("cuda")
    return _gpu_engine


def c_doubles(values, n: Optional[int] = None):
    """ctypes double array of the values (flattened); ``n``: its length, zero-filled behind short input."""
    v = [float(x) for x in np.asarray(values, dtype=np.float64).reshape(-1)]
    return (C.c_double * (len(v) if n is None else n))(*v)


def c_int32s(values):
    """ctypes int32 array of the values."""
    v = [int(x) for x in values]
    return (C.c_int32 * len(v))(*v)


def to_numpy(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def compact(verts: torch.Tensor, faces: torch.Tensor):
    """(the vertices some face uses, in their order; faces renumbered to them, int32)."""
    used = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    used[faces.reshape(-1).long()] = True
    remap = torch.cumsum(used.long(), 0) - 1
    return verts[used], remap[faces.long()].to(torch.int32)


# --------------------------------------------------------------------------------------------------
# camera poses
# --------------------------------------------------------------------------------------------------
def pose_stack(c2w, flip_yz: bool = False) -> np.ndarray:
    """[K, 4, 4] fp64 copy of one 4x4 pose, a [K, 4, 4] stack or a list of 4x4 poses (tensors or arrays).  ``flip_yz``
    negates the camera's y and z axes (OpenCV <-> the OpenGL / Open3D convention)."""
    m = np.array([to_numpy(p) for p in c2w] if isinstance(c2w, (list, tuple)) else to_numpy(c2w), np.float64)
    if m.shape == (4, 4):
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (4, 4):
        raise ValueError(f"c2w must be [4, 4] or [K, 4, 4] (got {m.shape})")
    if flip_yz:
        m[:, :3, 1] *= -1.0
        m[:, :3, 2] *= -1.0
    return m


def w2c_rows(c2ws, inv_dtype) -> np.ndarray:
    """[max(K, 1), 12] fp32: rows 0..2 of the inverse of each of the K 4x4 poses (a list or a [K, 4, 4] stack), inverted
    one matrix at a time in ``inv_dtype`` and then rounded to fp32 (zeros when K = 0, so the device copy is never empty).
    Each caller keeps the precision of the script it restates:

        mesher.point_masks_raw   None: the pose's own dtype (fp32 for tensor poses)  Mesher.py:130-132
        recon._w2c_rows (cull)   np.float32                                          cull_mesh.py:49 (float32 tensors)
        raster                   np.float64 (of pose_stack)                          --
        bound.frame_poses        np.float64 (of pose_stack(flip_yz=True))            Mesher.py:240-243
    """
    out = np.zeros((max(len(c2ws), 1), 12), dtype=np.float32)
    for k, c2w in enumerate(c2ws):
        c = to_numpy(c2w)
        out[k] = np.linalg.inv(c if inv_dtype is None else c.astype(inv_dtype))[:3].reshape(-1)
    return out
