"""Mint tests/golden/plasma_lut.npy from matplotlib: the 256 x 3 byte table floor(plasma.colors * 255), which is what
``plasma(x, bytes=True)`` returns for the 256 entries.  With ``--header`` also print the table as the rows of kPlasmaLut in
nice_slam_amd/csrc/nsr_figure.h.  Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_plasma.py [--header]"""
import os
import sys

import numpy as np
from matplotlib import colormaps

lut = np.floor(np.asarray(colormaps["plasma"].colors, np.float64) * 255.0).astype(np.uint8)
assert lut.shape == (256, 3)
assert np.array_equal(lut, colormaps["plasma"](np.arange(256), bytes=True)[:, :3])
np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "plasma_lut.npy"), lut)
print("wrote plasma_lut.npy", lut.shape, lut.dtype)
if "--header" in sys.argv:
    for i in range(0, 256, 8):
        print("    " + " ".join("{%d,%d,%d}," % tuple(int(v) for v in lut[j]) for j in range(i, i + 8)))
