"""RGB-D sequences: the readers of the reference's src/utils/datasets.py (Replica, ScanNet, Azure, CoFusion, TUM RGB-D) with
the per-frame preparation on the GPU.

    from nice_slam_amd import get_dataset, FramePreparer
    ds = get_dataset(cfg, input_folder=None, scale=None, device="cuda:0")      # cfg['dataset'] picks the class
    idx, gt_color, gt_depth, gt_c2w = ds[i]                                    # fp32 tensors on the device, as the reference's tuple
    idx, color, depth, c2w = ds.load_batch([0, 5, 10])                         # several frames, one launch
    H, W, fx, fy, cx, cy = ds.camera                                           # after NICE_SLAM.update_cam (NICE_SLAM.py:113-135)

    prep = FramePreparer(cfg)                                                  # frames that do not come from a folder
    color, depth = prep.prepare(color_u8, depth_u16, bgr=True)                 # e.g. what cv2.imread returned

The host decodes the files (PIL) and uploads the raw bytes -- u8 colour, u16 (or fp32) depth; with ``decoder="gpu"`` the colour
files' own bytes are uploaded and decoded on the device (nice_slam_amd.jpeg: the same pixels), depth stays on the host; with
``png_decoder="gpu"`` so are the compressed bytes of every PNG file, depth and colour (nice_slam_amd.png).  Everything
``BaseDataset.__getitem__`` (datasets.py:77-113) does after that runs in libnsr.so (include/nsr.h, "Frame preparation"; the
arithmetic is written out in csrc/nsr_frame.h): the undistortion of the colour image, BGR -> RGB, / 255, the resize to the
depth image's size, the depth scale, the ``crop_size`` resize, ``crop_edge`` and the cast to fp32.

Differences from the reference, both deliberate:
  * colour comes back fp32 (the reference hands fp64 to callers that cast it to fp32): the fp64 value rounded once;
  * the reference multiplies the stored pose's translation by ``scale`` on every access, in place (:111-112), so a frame read
    twice has its translation scaled twice; here the scale is applied once, when the poses are read.
"""
from __future__ import annotations

import ctypes as C
import glob
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _capi
from .engine import Engine, on

__all__ = ["FramePreparer", "get_dataset", "BaseDataset", "Replica", "ScanNet", "Azure", "CoFusion", "TUM_RGBD", "dataset_dict"]


def _engine(engine: Optional[Engine], device=None) -> Engine:
    return engine if engine is not None else on("cuda:0" if device is None else device)


class FramePreparer:
    """The camera block of a NICE-SLAM config (``cfg['cam']``, ``cfg['scale']``, read as BaseDataset.__init__ does,
    datasets.py:52-72) and the launch that turns raw frames into the tensors of ``BaseDataset.__getitem__``."""

    def __init__(self, cfg, engine: Optional[Engine] = None, scale: Optional[float] = None, device=None):
        cam = cfg["cam"]
        self.E = _engine(engine, device)
        self.scale = float(cfg["scale"] if scale is None else scale)
        self.png_depth_scale = float(cam["png_depth_scale"])
        self.raw_camera = (int(cam["H"]), int(cam["W"]), cam["fx"], cam["fy"], cam["cx"], cam["cy"])
        self.distortion = [float(v) for v in np.asarray(cam["distortion"]).reshape(-1)] if "distortion" in cam else None
        if self.distortion is not None and len(self.distortion) != 5:
            raise ValueError(f"cfg['cam']['distortion'] must be [k1, k2, p1, p2, k3] (got {len(self.distortion)} values)")
        self.crop_size = tuple(int(v) for v in cam["crop_size"]) if "crop_size" in cam else None
        self.crop_edge = int(cam["crop_edge"])

    @property
    def camera(self):
        """(H, W, fx, fy, cx, cy) of the prepared frames: NICE_SLAM.update_cam (NICE_SLAM.py:113-135), the same operations."""
        H, W, fx, fy, cx, cy = self.raw_camera
        if self.crop_size is not None:
            sx = self.crop_size[1] / W
            sy = self.crop_size[0] / H
            fx = sx * fx
            fy = sy * fy
            cx = sx * cx
            cy = sy * cy
            W = self.crop_size[1]
            H = self.crop_size[0]
        if self.crop_edge > 0:
            H -= self.crop_edge * 2
            W -= self.crop_edge * 2
            cx -= self.crop_edge
            cy -= self.crop_edge
        return H, W, fx, fy, cx, cy

    @property
    def out_size(self):
        """(H, W) of the prepared frames when the depth images have the config's size"""
        return self.camera[:2]

    def desc(self, color_hw, depth_hw, depth_f32: bool, bgr: bool) -> _capi.NsrFrameDesc:
        d = _capi.NsrFrameDesc()
        d.color_h, d.color_w = color_hw
        d.depth_h, d.depth_w = depth_hw
        d.depth_type = 1 if depth_f32 else 0
        d.color_bgr = 1 if bgr else 0
        d.crop_h, d.crop_w = self.crop_size if self.crop_size is not None else (0, 0)
        d.crop_edge = self.crop_edge
        d.has_distortion = 0 if self.distortion is None else 1
        _, _, d.fx, d.fy, d.cx, d.cy = self.raw_camera
        for i, v in enumerate(self.distortion or ()):
            d.dist[i] = v
        d.png_depth_scale, d.scale = self.png_depth_scale, self.scale
        return d

    def _raw(self, x, channels: bool, what: str) -> torch.Tensor:
        """[B, H, W(, 3)] contiguous on the engine's device; u16 depth travels as int16 (the same bytes)"""
        if not isinstance(x, torch.Tensor):
            a = np.ascontiguousarray(x)
            if not channels and a.dtype == np.uint16:
                a = a.view(np.int16)
            x = torch.from_numpy(a)
        t = x.detach()
        nd = 3 if channels else 2
        if t.dim() == nd:
            t = t[None]
        if t.dim() != nd + 1 or (channels and t.shape[-1] != 3):
            raise ValueError(f"prepare: {what} must be [H, W{', 3' if channels else ''}] or a batch of them (got {tuple(x.shape)})")
        if channels:
            if t.dtype != torch.uint8:
                raise ValueError(f"prepare: {what} must be uint8 (got {t.dtype})")
        elif t.dtype == torch.float64:
            t = t.to(torch.float32)
        elif t.dtype == getattr(torch, "uint16", None):
            t = t.view(torch.int16)
        elif t.dtype not in (torch.int16, torch.float32):
            raise ValueError(f"prepare: {what} must be uint16 (or its bytes as int16), float32 or float64 (got {t.dtype})")
        return t.to(self.E.device, non_blocking=True).contiguous()

    def prepare(self, color_u8, depth_raw, bgr: bool = False):
        """One frame (``color_u8`` [Hc, Wc, 3] uint8, ``depth_raw`` [Hd, Wd] uint16 or float) or a batch ([B, ...]); arrays or
        tensors of any device.  ``bgr``: the colour channels are in cv2's order.  Returns (colour [H, W, 3], depth [H, W]) fp32
        on the engine's device, with the leading B for a batch.  Device tensors in: nothing here waits for the device."""
        E, lib = self.E, self.E.lib
        single = (color_u8.ndim if hasattr(color_u8, "ndim") else np.asarray(color_u8).ndim) == 3
        c, d = self._raw(color_u8, True, "color_u8"), self._raw(depth_raw, False, "depth_raw")
        if c.shape[0] != d.shape[0]:
            raise ValueError(f"prepare: {c.shape[0]} colour images but {d.shape[0]} depth images")
        B = c.shape[0]
        desc = self.desc(c.shape[1:3], d.shape[1:3], d.dtype == torch.float32, bgr)
        H, W = C.c_int32(), C.c_int32()
        lib.call("nsr_frame_out_size", C.byref(desc), C.byref(H), C.byref(W))
        color = torch.empty((B, H.value, W.value, 3), dtype=torch.float32, device=E.device)
        depth = torch.empty((B, H.value, W.value), dtype=torch.float32, device=E.device)
        with torch.no_grad(), E.guard():
            nbytes = int(lib.nsr_frame_workspace_bytes(C.byref(desc), B))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=E.device) if nbytes > 0 else None
            E.call("nsr_frame_prepare", c.data_ptr(), d.data_ptr(), C.byref(desc), B, color.data_ptr(), depth.data_ptr(),
                   ws.data_ptr() if ws is not None else None, max(nbytes, 0))
        return (color[0], depth[0]) if single else (color, depth)


# --------------------------------------------------------------------------------------------------
# the sequence readers
# --------------------------------------------------------------------------------------------------
def read_exr_depth(path: str) -> np.ndarray:
    """the Y channel of an EXR file as fp32 [H, W] (datasets.py:12-44); needs the OpenEXR package"""
    try:
        import Imath
        import OpenEXR as exr
    except ImportError as e:
        raise ImportError(f"reading {path} needs the OpenEXR and Imath packages (only the CoFusion sequences store .exr depth); "
                          f"every other dataset works without them") from e
    f = exr.InputFile(path)
    header = f.header()
    dw = header["dataWindow"]
    size = (dw.max.y - dw.min.y + 1, dw.max.x - dw.min.x + 1)
    if "Y" not in header["channels"]:
        raise ValueError(f"{path}: no Y channel")
    return np.frombuffer(f.channel("Y", Imath.PixelType(Imath.PixelType.FLOAT)), dtype=np.float32).reshape(size).copy()


def _flip_yz(c2w: np.ndarray) -> torch.Tensor:
    c2w[:3, 1] *= -1
    c2w[:3, 2] *= -1
    return torch.from_numpy(c2w).float()


class BaseDataset:
    """``ds[i]`` -> (i, colour [H, W, 3], depth [H, W], c2w [4, 4]), fp32 on the device.  Subclasses fill ``color_paths``,
    ``depth_paths`` and ``poses`` (fp32 4 x 4 tensors in the reference's convention, translation NOT yet scaled)."""

    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine: Optional[Engine] = None, decoder: Optional[str] = None,
                 png_decoder: Optional[str] = None):
        self.name = cfg["dataset"]
        decoder = (cfg.get("data") or {}).get("decoder", "pil") if decoder is None else decoder
        if decoder not in ("pil", "gpu"):
            raise ValueError(f"decoder must be 'pil' or 'gpu' (got {decoder!r})")
        png_decoder = (cfg.get("data") or {}).get("png_decoder", "pil") if png_decoder is None else png_decoder
        if png_decoder not in ("pil", "gpu"):
            raise ValueError(f"png_decoder must be 'pil' or 'gpu' (got {png_decoder!r})")
        self.decoder = decoder
        self.png_decoder = png_decoder
        self.decode_fallbacks = 0                  # frames of decoder="gpu" that went through PIL after all
        self.png_fallbacks = 0                     # PNG files of png_decoder="gpu" that went through PIL after all
        self.prep = FramePreparer(cfg, engine=engine, scale=scale, device=device)
        self.device = self.prep.E.device
        self.scale = self.prep.scale
        self.input_folder = cfg["data"]["input_folder"] if input_folder is None else input_folder
        self.color_paths, self.depth_paths, self.poses = [], [], []

    def _finish(self):
        """the translation scale of datasets.py:111-112, applied once (fp32, as the reference's in-place product)"""
        self.n_img = len(self.color_paths)
        self.poses = [p.clone() for p in self.poses]
        for p in self.poses:
            p[:3, 3] *= self.scale

    camera = property(lambda self: self.prep.camera)

    def __len__(self):
        return self.n_img

    def read_raw(self, index: int):
        """(colour u8 [Hc, Wc, 3] RGB, depth u16 or fp32 [Hd, Wd]) as decoded, host arrays"""
        from PIL import Image
        with Image.open(self.color_paths[index]) as im:
            color = np.array(im.convert("RGB"), dtype=np.uint8)
        depth = self.read_depth(index)
        return color, depth

    def read_depth(self, index: int):
        """depth u16 or fp32 [Hd, Wd] as decoded, a host array (read_raw's second value)"""
        from PIL import Image
        depth_path = self.depth_paths[index]
        if ".png" in depth_path:
            with Image.open(depth_path) as im:
                depth = np.array(im)
            if depth.ndim != 2:
                raise ValueError(f"{depth_path}: a depth image has one channel (got shape {depth.shape})")
            if depth.dtype != np.uint16:
                if depth.min() < 0 or depth.max() > 65535:
                    raise ValueError(f"{depth_path}: depth values outside 16 bits")
                depth = depth.astype(np.uint16)
        elif ".exr" in depth_path:
            depth = read_exr_depth(depth_path)
        else:
            raise ValueError(f"{depth_path}: depth images are .png or .exr")
        return depth

    def _decode_png_files(self, data, ks, mode, kinds):
        """{k: the device pixels of data[k]} for the k in ``ks`` whose file the PNG decoder takes, of one of ``kinds``, and whose
        stream the device found whole; the files of one size and kind go in one call"""
        from . import png
        groups, out, parsed = {}, {}, {}
        for k in ks:
            try:
                p = parsed[k] = png.parse_png(data[k])             # the one chunk walk and CRC pass of the file
            except png.PngRefused:
                continue
            if p["kind"] in kinds:
                groups.setdefault((p["height"], p["width"], p["kind"]), []).append(k)
        for group in groups.values():
            frames, status = png.decode_png_status([parsed[k] for k in group], mode=mode, engine=self.prep.E)
            for j, k in enumerate(group):
                if status[j] == 0:
                    out[k] = frames[j]
        return out

    def read_depth_gpu(self, indices: Sequence[int]) -> torch.Tensor:
        """The frames' depth [B, Hd, Wd] on the device, u16 as its bytes in int16 (``FramePreparer.prepare`` takes them as they
        are): the compressed bytes of the .png files are uploaded and decoded there (nice_slam_amd.png), 8-bit grey widened as
        ``read_depth`` does.  A file the decoder does not take (``png.probe_png`` says why) or whose stream the device reports
        damaged goes through ``read_depth`` and is counted in ``png_fallbacks``; an .exr file is ``read_depth``'s as before."""
        data = {}
        for k, i in enumerate(indices):
            if ".png" in self.depth_paths[i]:
                with open(self.depth_paths[i], "rb") as fh:
                    data[k] = fh.read()
        done = self._decode_png_files(data, list(data), None, ("grey8", "grey16"))       # (the kinds read_depth accepts)
        out = []
        for k, i in enumerate(indices):
            if k in done:
                t = done[k]
                out.append(t.view(torch.int16) if t.dtype != torch.uint8 else t.to(torch.int16))
                continue
            if k in data:
                self.png_fallbacks += 1
            d = self.read_depth(i)
            out.append(torch.from_numpy(d.view(np.int16) if d.dtype == np.uint16 else d).to(self.device))
        return torch.stack(out)

    def read_color_gpu(self, indices: Sequence[int]) -> torch.Tensor:
        """u8 [B, Hc, Wc, 3] RGB on the device of the frames' colour files, decoded there (nice_slam_amd.jpeg): the files' bytes are
        uploaded, not their pixels.  A file the decoder does not take (not a JPEG, progressive, ...; ``jpeg.probe_jpeg`` says why)
        or whose stream the device reports damaged goes through PIL as in ``read_raw`` -- the pixels are the same either way,
        and PIL's error is the error of a file nobody can read -- and is counted in ``decode_fallbacks``.  With
        ``png_decoder="gpu"`` a file that starts with the PNG signature goes to nice_slam_amd.png instead, whatever ``decoder``
        is, and is counted in ``png_fallbacks`` when it comes back from there; with ``decoder="pil"`` every other file is PIL's."""
        from PIL import Image

        from . import jpeg, png
        data = []
        for i in indices:
            with open(self.color_paths[i], "rb") as fh:
                data.append(fh.read())
        out = [None] * len(data)

        def through_pil(k):
            with Image.open(self.color_paths[indices[k]]) as im:
                out[k] = torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8)).to(self.device)

        pngs = [k for k, d in enumerate(data) if self.png_decoder == "gpu" and d[:8] == png.SIGNATURE]
        for k, frame in self._decode_png_files(data, pngs, "RGB", ("grey8", "rgb8", "rgba8")).items():
            out[k] = frame
        for k in pngs:
            if out[k] is None:
                self.png_fallbacks += 1
                through_pil(k)
        rest = [k for k in range(len(data)) if out[k] is None]
        if self.decoder == "gpu":
            info = {k: jpeg.probe_jpeg(data[k]) for k in rest}
            groups = {}                            # frames of one size and sampling decode in one call
            for k, p in info.items():
                if p["supported"]:
                    groups.setdefault((p["height"], p["width"], p["sampling"]), []).append(k)
            for ks in groups.values():
                frames, status = jpeg.decode_jpeg_status([data[k] for k in ks], engine=self.prep.E)
                for j, k in enumerate(ks):
                    if status[j] == 0:
                        out[k] = frames[j]
        for k in rest:
            if out[k] is None:
                if self.decoder == "gpu":
                    self.decode_fallbacks += 1
                through_pil(k)
        return torch.stack(out)

    def _depth_batch(self, indices):
        return self.read_depth_gpu(indices) if self.png_decoder == "gpu" else np.stack([self.read_depth(i) for i in indices])

    def load_batch(self, indices: Sequence[int]):
        """(indices, colour [B, H, W, 3], depth [B, H, W], c2w [B, 4, 4]) of several frames, prepared by one launch"""
        indices = [int(i) for i in indices]
        if self.decoder == "gpu" or self.png_decoder == "gpu":
            color, depth = self.prep.prepare(self.read_color_gpu(indices), self._depth_batch(indices), bgr=False)
            return indices, color, depth, torch.stack([self.poses[i] for i in indices]).to(self.device)
        raw = [self.read_raw(i) for i in indices]
        color, depth = self.prep.prepare(np.stack([r[0] for r in raw]), np.stack([r[1] for r in raw]), bgr=False)
        return indices, color, depth, torch.stack([self.poses[i] for i in indices]).to(self.device)

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < self.n_img:
            raise IndexError(index)
        if self.png_decoder == "gpu":
            color, depth = self.prep.prepare(self.read_color_gpu([index])[0], self.read_depth_gpu([index])[0], bgr=False)
        elif self.decoder == "gpu":
            color, depth = self.prep.prepare(self.read_color_gpu([index])[0], self.read_depth(index), bgr=False)
        else:
            color, depth = self.prep.prepare(*self.read_raw(index), bgr=False)
        return index, color, depth, self.poses[index].to(self.device)


class Replica(BaseDataset):
    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine=None, decoder=None, png_decoder=None):
        super().__init__(cfg, input_folder, scale, device, engine, decoder, png_decoder)
        self.color_paths = sorted(glob.glob(f"{self.input_folder}/results/frame*.jpg"))
        self.depth_paths = sorted(glob.glob(f"{self.input_folder}/results/depth*.png"))
        with open(f"{self.input_folder}/traj.txt", "r") as f:
            lines = f.readlines()
        for i in range(len(self.color_paths)):
            self.poses.append(_flip_yz(np.array(list(map(float, lines[i].split()))).reshape(4, 4)))
        self._finish()


class Azure(BaseDataset):
    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine=None, decoder=None, png_decoder=None):
        super().__init__(cfg, input_folder, scale, device, engine, decoder, png_decoder)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, "color", "*.jpg")))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, "depth", "*.png")))
        path = os.path.join(self.input_folder, "scene", "trajectory.log")
        if os.path.exists(path):
            with open(path) as f:
                content = f.readlines()
            for i in range(0, len(content), 5):           # "%d (src) %d (tgt) %f (fitness)", then 4 rows of the pose
                self.poses.append(_flip_yz(np.array(list(map(float, "".join(content[i + 1:i + 5]).strip().split()))).reshape(4, 4)))
        else:
            self.poses = [torch.eye(4) for _ in self.color_paths]
        self._finish()


class ScanNet(BaseDataset):
    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine=None, decoder=None, png_decoder=None):
        super().__init__(cfg, input_folder, scale, device, engine, decoder, png_decoder)
        self.input_folder = os.path.join(self.input_folder, "frames")

        def number(p):
            return int(os.path.basename(p)[:-4])

        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, "color", "*.jpg")), key=number)
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, "depth", "*.png")), key=number)
        for pose_path in sorted(glob.glob(os.path.join(self.input_folder, "pose", "*.txt")), key=number):
            with open(pose_path, "r") as f:
                rows = [list(map(float, line.split(" "))) for line in f.readlines()]
            self.poses.append(_flip_yz(np.array(rows).reshape(4, 4)))
        self._finish()


class CoFusion(BaseDataset):
    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine=None, decoder=None, png_decoder=None):
        super().__init__(cfg, input_folder, scale, device, engine, decoder, png_decoder)
        self.color_paths = sorted(glob.glob(os.path.join(self.input_folder, "colour", "*.png")))
        self.depth_paths = sorted(glob.glob(os.path.join(self.input_folder, "depth_noise", "*.exr")))
        self.poses = [torch.eye(4) for _ in self.color_paths]      # the reference's proxy: the frames could not be aligned
        self._finish()


class TUM_RGBD(BaseDataset):
    def __init__(self, cfg, input_folder=None, scale=None, device="cuda:0", engine=None, decoder=None, png_decoder=None):
        super().__init__(cfg, input_folder, scale, device, engine, decoder, png_decoder)
        self.color_paths, self.depth_paths, self.poses = self.loadtum(self.input_folder, frame_rate=32)
        self._finish()

    @staticmethod
    def parse_list(filepath, skiprows=0):
        import warnings
        with warnings.catch_warnings():           # (a skipped row that is a comment line: numpy says it does not count it)
            warnings.simplefilter("ignore", UserWarning)
            return np.loadtxt(filepath, delimiter=" ", dtype=str, skiprows=skiprows)

    @staticmethod
    def associate_frames(tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
        """pair images, depths and poses by nearest timestamp within max_dt (datasets.py:248-265)"""
        associations = []
        for i, t in enumerate(tstamp_image):
            j = np.argmin(np.abs(tstamp_depth - t))
            if tstamp_pose is None:
                if np.abs(tstamp_depth[j] - t) < max_dt:
                    associations.append((i, j))
            else:
                k = np.argmin(np.abs(tstamp_pose - t))
                if np.abs(tstamp_depth[j] - t) < max_dt and np.abs(tstamp_pose[k] - t) < max_dt:
                    associations.append((i, j, k))
        return associations

    @staticmethod
    def pose_matrix_from_quaternion(pvec):
        from scipy.spatial.transform import Rotation
        pose = np.eye(4)
        pose[:3, :3] = Rotation.from_quat(pvec[3:]).as_matrix()
        pose[:3, 3] = pvec[:3]
        return pose

    def loadtum(self, datapath, frame_rate=-1):
        """(colour paths, depth paths, poses) of a sequence in the TUM RGB-D layout (datasets.py:267-312): frames thinned to
        ``frame_rate``, poses relative to the first kept frame's"""
        pose_list = None
        for name in ("groundtruth.txt", "pose.txt"):
            if os.path.isfile(os.path.join(datapath, name)):
                pose_list = os.path.join(datapath, name)
                break
        if pose_list is None:
            raise FileNotFoundError(f"{datapath}: neither groundtruth.txt nor pose.txt")
        image_data = self.parse_list(os.path.join(datapath, "rgb.txt"))
        depth_data = self.parse_list(os.path.join(datapath, "depth.txt"))
        pose_data = self.parse_list(pose_list, skiprows=1)
        pose_vecs = pose_data[:, 1:].astype(np.float64)
        tstamp_image = image_data[:, 0].astype(np.float64)
        tstamp_depth = depth_data[:, 0].astype(np.float64)
        tstamp_pose = pose_data[:, 0].astype(np.float64)
        associations = self.associate_frames(tstamp_image, tstamp_depth, tstamp_pose)
        kept = [0]
        for i in range(1, len(associations)):
            t0 = tstamp_image[associations[kept[-1]][0]]
            t1 = tstamp_image[associations[i][0]]
            if t1 - t0 > 1.0 / frame_rate:
                kept += [i]
        images, depths, poses = [], [], []
        inv_pose = None
        for ix in kept:
            i, j, k = associations[ix]
            images += [os.path.join(datapath, image_data[i, 1])]
            depths += [os.path.join(datapath, depth_data[j, 1])]
            c2w = self.pose_matrix_from_quaternion(pose_vecs[k])
            if inv_pose is None:
                inv_pose = np.linalg.inv(c2w)
                c2w = np.eye(4)
            else:
                c2w = inv_pose @ c2w
            poses += [_flip_yz(c2w)]
        return images, depths, poses


dataset_dict = {"replica": Replica, "scannet": ScanNet, "cofusion": CoFusion, "azure": Azure, "tumrgbd": TUM_RGBD}


def get_dataset(cfg, input_folder=None, scale=None, device="cuda:0", engine: Optional[Engine] = None, decoder: Optional[str] = None,
                png_decoder: Optional[str] = None) -> BaseDataset:
    """The reader of ``cfg['dataset']`` (datasets.py:47-48).  ``input_folder``: instead of ``cfg['data']['input_folder']``
    (the reference's ``args.input_folder``); ``scale``: instead of ``cfg['scale']``.  ``decoder``: "pil" (the default; also
    ``cfg['data']['decoder']``) decodes the colour files on the host, "gpu" on the device (``BaseDataset.read_color_gpu``); the
    tensors are the same.  ``png_decoder``: "pil" (the default; also ``cfg['data']['png_decoder']``) or "gpu", a switch of its own
    for the PNG files -- every .png depth image and every colour file that is a PNG (``BaseDataset.read_depth_gpu``,
    ``read_color_gpu``); again the same tensors."""
    return dataset_dict[cfg["dataset"]](cfg, input_folder, scale, device, engine, decoder, png_decoder)
