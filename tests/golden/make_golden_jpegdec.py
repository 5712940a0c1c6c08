#!/usr/bin/env python3
"""Writes tests/golden/jpeg_decode.npz: a dozen small JPEG files as Pillow (with libjpeg-turbo) writes them and Pillow's own pixels
of each -- ``np.array(Image.open(f).convert("RGB"))`` -- so that the gate against libjpeg-turbo's decoder does not depend on the
Pillow of the machine that runs the tests.  ``<name>.jpg`` holds a file's bytes (uint8), ``<name>.rgb`` its pixels; ``versions``
names what wrote them.  The last two are files the decoder refuses (a progressive one, and RGB data with Adobe transform 0): they come
with pixels too, for the dataset readers' PIL path.

    python tests/golden/make_golden_jpegdec.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpegdec_reference as D  # noqa: E402

CASES = {
    "default_33x49_420": (D.recipe_image(33, 49, seed=1), dict(quality=90)),
    "optimize_50x70_420": (D.recipe_image(50, 70, seed=2), dict(quality=75, optimize=True)),
    "optimize_noise_17x23_444": (D.noise_image(17, 23, seed=3), dict(quality=100, optimize=True, subsampling="4:4:4")),
    "rows_50x70_444": (D.recipe_image(50, 70, seed=4), dict(quality=90, subsampling="4:4:4", restart_marker_rows=1)),
    "blocks3_50x70_420": (D.recipe_image(50, 70, seed=5), dict(quality=90, restart_marker_blocks=3)),
    "blocks1_17x23_422": (D.noise_image(17, 23, seed=6), dict(quality=30, subsampling="4:2:2", restart_marker_blocks=1)),
    "grey_33x49": (D.recipe_image(33, 49, seed=7)[..., 1].copy(), dict(quality=90)),
    "h2v1_33x49_422": (D.recipe_image(33, 49, seed=8), dict(quality=90, subsampling="4:2:2")),
    "q1_16x16_420": (D.recipe_image(16, 16, seed=9), dict(quality=1)),
    "one_pixel_444": (D.recipe_image(1, 1, seed=10), dict(quality=90, subsampling="4:4:4")),
    "refused_progressive_33x49": (D.recipe_image(33, 49, seed=11), dict(quality=90, progressive=True)),
    "refused_rgb_adobe0_17x23": (D.recipe_image(17, 23, seed=12), dict(quality=90, keep_rgb=True)),
}


def main():
    out = {"versions": np.array(f"Pillow {Image.__version__}, libjpeg-turbo {features.version('libjpeg_turbo')}, jpg {features.version('jpg')}")}
    for name, (img, options) in CASES.items():
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", **options)
        data = buf.getvalue()
        out[name + ".jpg"] = np.frombuffer(data, np.uint8)
        out[name + ".rgb"] = D.pil_pixels(data)
        print(name, len(data), D.verdict(data))
    path = os.path.join(HERE, "jpeg_decode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
