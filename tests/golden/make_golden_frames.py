#!/usr/bin/env python3
"""Mint ``tests/golden/frames.npz`` by executing the UNMODIFIED reference ``BaseDataset.__getitem__`` (src/utils/datasets.py:77-113),
the Replica / ScanNet / Azure pose loaders (:116-209) and ``NICE_SLAM.update_cam`` (src/NICE_SLAM.py:113-135) on tiny sequences
written with PIL.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frames.py /path/to/the/reference/checkout

OpenCV is absent, so a stub ``cv2`` module stands in, as the caller goldens stub their I/O: ``imread`` decodes with PIL and
returns BGR (IMREAD_UNCHANGED: the file's own array), ``cvtColor`` flips the channels, ``resize`` accepts equal sizes only and
returns its input.  None of them does arithmetic.  The decoded arrays are recorded as the fixture's INPUTS, so nothing depends
on the JPEG decoder.

What this cannot mint, and what therefore rests on the restatement of tests/frames_reference.py alone: ``cv2.undistort``, and
``cv2.resize`` between different sizes (no OpenCV); the TUM loader, which does not run under the installed numpy
(``np.unicode_`` is gone).

Per case (replica / scannet / azure) the file holds: ``cfg`` (JSON), ``raw_color`` u8 RGB and ``raw_depth`` u16 as decoded, in
the loader's order; ``color`` fp64, ``depth`` fp32 and ``pose`` fp32 as ``ds[i]`` returned them on the FIRST access of each
frame; ``pose_twice``: frame 0's pose on a second access (the reference scales the translation again); ``cam``: update_cam's
(H, W, fx, fy, cx, cy).
"""
import json
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.path.insert(1, os.path.join(ROOT, "tests"))

import numpy as np
from PIL import Image

import frames_reference as R                                # noqa: E402

for _m in ("cv2", "colorama", "open3d", "skimage", "skimage.measure", "trimesh", "mathutils", "matplotlib", "matplotlib.pyplot"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
sys.modules["colorama"].Fore = types.SimpleNamespace(GREEN="", MAGENTA="", RED="")
sys.modules["colorama"].Style = types.SimpleNamespace(RESET_ALL="")
cv2 = sys.modules["cv2"]
cv2.IMREAD_UNCHANGED, cv2.COLOR_BGR2RGB = -1, 4


def _imread(path, flag=None):
    with Image.open(path) as im:
        if flag == cv2.IMREAD_UNCHANGED:
            return np.asarray(im).copy()
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def _cvt(img, code):
    assert code == cv2.COLOR_BGR2RGB
    return np.ascontiguousarray(img[..., ::-1])


def _resize(img, size):
    assert (img.shape[1], img.shape[0]) == tuple(size), "the stub resizes between equal sizes only"
    return img


cv2.imread, cv2.cvtColor, cv2.resize = _imread, _cvt, _resize

from src.utils import datasets as ref_datasets             # noqa: E402
from src.NICE_SLAM import NICE_SLAM                        # noqa: E402

CASES = {   # layout -> (frames, H, W, make_cfg keywords, ScanNet file numbers)
    "replica": (3, 24, 40, dict(scale=0.7, png_depth_scale=6553.5), None),
    "scannet": (5, 20, 28, dict(scale=1.3, png_depth_scale=1000.0, crop_edge=3), [0, 1, 2, 9, 10]),
    "azure": (3, 24, 32, dict(scale=1.0, png_depth_scale=1000.0, crop_size=(18, 26), crop_edge=2), None),
}


def main():
    out = {}
    for layout, (n, H, W, kw, numbers) in CASES.items():
        colors, depths = R.make_frames(n, (H, W), (H, W), seed=len(layout))
        poses = R.make_poses(n, seed=len(layout))
        with tempfile.TemporaryDirectory() as tmp:
            folder = os.path.join(tmp, layout)
            R.write_sequence(layout, folder, colors, depths, poses, numbers)
            cfg = R.make_cfg(H, W, dataset=layout, input_folder=folder, **kw)
            ds = ref_datasets.get_dataset(cfg, types.SimpleNamespace(input_folder=None), cfg["scale"], device="cpu")
            assert len(ds) == n
            out[f"{layout}/raw_color"] = np.stack([_imread(p)[..., ::-1] for p in ds.color_paths])
            out[f"{layout}/raw_depth"] = np.stack([_imread(p, cv2.IMREAD_UNCHANGED) for p in ds.depth_paths])
            assert out[f"{layout}/raw_depth"].dtype == np.uint16
            got = [ds[i] for i in range(n)]
            out[f"{layout}/color"] = np.stack([g[1].numpy() for g in got])
            out[f"{layout}/depth"] = np.stack([g[2].numpy() for g in got])
            out[f"{layout}/pose"] = np.stack([g[3].numpy().copy() for g in got])
            out[f"{layout}/pose_twice"] = ds[0][3].numpy().copy()
            assert out[f"{layout}/color"].dtype == np.float64 and out[f"{layout}/depth"].dtype == np.float32
        me = types.SimpleNamespace(cfg=cfg, H=cfg["cam"]["H"], W=cfg["cam"]["W"], fx=cfg["cam"]["fx"], fy=cfg["cam"]["fy"],
                                   cx=cfg["cam"]["cx"], cy=cfg["cam"]["cy"])
        NICE_SLAM.update_cam(me)
        out[f"{layout}/cam"] = np.array([me.H, me.W, me.fx, me.fy, me.cx, me.cy], np.float64)
        cfg["data"]["input_folder"] = ""
        out[f"{layout}/cfg"] = np.array(json.dumps(cfg))
    path = os.path.join(HERE, "frames.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
