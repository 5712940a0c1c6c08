"""No entry writes beyond the workspace size its size entry reports: the smallest emulator case of every module with a
multi-piece workspace (nsr_api.cpp: the *_carve functions) runs through the module's own Python function on an engine whose
library reports every workspace 64 bytes larger than it is, fills those 64 bytes with a pattern when an entry is first handed
the workspace, and looks at them again after every call that was handed it (no other call has the pointer).  The case's own
check of its outputs runs as in its module.

The negative control places the band 16 bytes INSIDE the true size -- host memory that belongs to the workspace, so nothing
overflows: every module whose last piece is written to its end must then report a damaged band.

CPU only: device memory cannot be looked at between calls without machinery of its own."""
import ctypes as C

import numpy as np
import pytest

import bound_reference as BR
import emu_harness
import test_bound_emu as TB
import test_jpeg_emu as TJ
import test_jpegdec_emu as TD
import test_meshdist_emu as TM
import test_mesher_emu as TMC
import test_raster_emu as TR
import test_recon_emu as TN
import test_view_emu as TV
from nice_slam_amd import bound
from nice_slam_amd.engine import Engine

BAND, PATTERN = 64, 0xA5
# size entries that return the byte count, and those that write it through their k-th argument
SIZE_ENTRIES = ("nsr_mc_workspace_bytes", "nsr_tsdf_workspace_bytes", "nsr_nn_workspace_bytes", "nsr_meshdist_workspace_bytes",
                "nsr_raster_workspace_bytes", "nsr_view_workspace_bytes")
SIZE_BY_POINTER = {"nsr_jpeg_size": 4, "nsr_jpegdec_size": 6}
# the workspace argument of every entry that takes one of these workspaces (include/nsr.h)
WS_ARG = {"nsr_mc_count": 5, "nsr_mc_emit": 7, "nsr_tsdf_touch_count": 12, "nsr_tsdf_touch_emit": 12, "nsr_tsdf_surface_count": 1,
          "nsr_tsdf_surface_emit": 1, "nsr_nn_build": 6, "nsr_nn_query": 5, "nsr_meshdist_build": 13, "nsr_meshdist_query": 5,
          "nsr_raster_bin": 14, "nsr_raster_depth": 14, "nsr_view_mesh": 14, "nsr_jpeg_encode": 6, "nsr_jpegdec_decode": 7}


class GuardedLib:
    """The library as an Engine holds it (``call`` and the size entries), with a guard band behind every workspace; ``inside``:
    bytes by which the band starts before the true size (the negative control)."""

    def __init__(self, lib, inside=0):
        self.lib, self.inside = lib, inside
        self.pending = None                 # the true size of the last workspace measured, until an entry is handed it
        self.band = {}                      # workspace pointer -> address of its band
        self.checked, self.damaged = [], []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        return (lambda *args: self.measured(fn(*args))) if name in SIZE_ENTRIES else fn

    def measured(self, true):
        if true < 0:
            return true
        self.pending = true
        return true + BAND

    def call(self, name, *args):
        if name in SIZE_BY_POINTER:
            self.lib.call(name, *args)
            cell = args[SIZE_BY_POINTER[name]]._obj
            cell.value = self.measured(cell.value)
            return
        ws = args[WS_ARG[name]] if name in WS_ARG else None
        if ws and self.pending is not None and self.pending >= self.inside:
            self.band[ws] = ws + self.pending - self.inside
            C.memset(self.band[ws], PATTERN, BAND)
            self.pending = None
        self.lib.call(name, *args)
        if ws:
            assert ws in self.band, f"{name}: a workspace that no size entry measured"
            self.checked.append(name)
            if bytes((C.c_ubyte * BAND).from_address(self.band[ws])) != bytes([PATTERN]) * BAND:
                self.damaged.append(name)


def tsdf_case(E):
    """the three-frame scene of test_bound_emu.py and its checks of the touched units and the surface points"""
    kfs = BR.room_keyframes(3, TB.H, TB.W, TB.FX, TB.FY, TB.CX, TB.CY, seed=3)
    depth = np.stack([k["depth"] for k in kfs])
    c2w, w2c, cams = BR.poses(kfs)
    vl, tr = 4 * TB.SCALE / 512, 0.04 * TB.SCALE
    units, touch = BR.touched(depth, c2w, TB.FX, TB.FY, TB.CX, TB.CY, vl, tr)
    ts, ws = BR.integrate(units, touch, depth, w2c, TB.FX, TB.FY, TB.CX, TB.CY, vl, tr)
    scene = dict(kfs=kfs, units=units, touch=touch, tsdf=ts, weight=ws, vl=vl, surf=BR.surface(units, ts, ws, vl),
                 vol=bound.tsdf_fuse(kfs, TB.H, TB.W, TB.FX, TB.FY, TB.CX, TB.CY, TB.SCALE, engine=E))
    TB.test_touched_units_exact(scene)
    TB.test_surface_points_exact_in_order(scene)


# module -> (its smallest case with the case's own checks, the entries that must have been handed a guarded workspace)
CASES = {
    "marching_cubes": (lambda E: TMC.test_mc_matches_restatement(E, "plane"), {"nsr_mc_count", "nsr_mc_emit"}),
    "tsdf": (tsdf_case, {"nsr_tsdf_touch_count", "nsr_tsdf_touch_emit", "nsr_tsdf_surface_count", "nsr_tsdf_surface_emit"}),
    "nearest_neighbour": (lambda E: TN.check_nn(E, *TN.cases()["one_point"]), {"nsr_nn_build", "nsr_nn_query"}),
    "mesh_distance": (lambda E: TM.check_mesh(E, *TM.CASES["one_face"]), {"nsr_meshdist_build", "nsr_meshdist_query"}),
    "raster": (TR.test_depth_matches_restatement, {"nsr_raster_bin", "nsr_raster_depth"}),
    "view": (TV.test_duplicated_face_is_owned_by_the_smaller_id, {"nsr_raster_bin", "nsr_view_mesh"}),
    "jpeg_encode": (lambda E: TJ.test_bytes_equal_the_restatement(E, "small1x1", "4:4:4"), {"nsr_jpeg_encode"}),
    "jpeg_decode": (lambda E: TD.test_emulator_equals_restatement(E, (1, 1), "grey", 16), {"nsr_jpegdec_decode"}),
}
# the last piece of these is written to its last 16 bytes by the case (the kernels that do it, in nsr_api.cpp's *_carve order):
#   marching cubes   blk [nblocks][2]          mc_count_kernel writes every block's two totals
#   nearest neighbour cbox [ncoarse][6]        nn_box_kernel writes the box of every coarse cell
#   raster, view     tile_start [K ntiles + 1] raster_scan_view_kernel writes the total into the last element
#   JPEG encode      ftot [n]                  jpeg_offsets_kernel writes every frame's byte count
#   JPEG decode      cstat [n][M]              jpegdec_huffman_kernel writes every chain's status
WRITTEN_TO_THE_END = ("marching_cubes", "nearest_neighbour", "raster", "view", "jpeg_encode", "jpeg_decode")


@pytest.mark.parametrize("module", list(CASES))
def test_nothing_written_beyond_the_reported_size(module):
    run, entries = CASES[module]
    lib = GuardedLib(emu_harness.emu_lib())
    run(Engine(lib, "cpu"))
    assert entries <= set(lib.checked), (entries, set(lib.checked))
    assert not lib.damaged, lib.damaged


@pytest.mark.parametrize("module", WRITTEN_TO_THE_END)
def test_a_band_inside_the_workspace_is_seen_damaged(module):
    lib = GuardedLib(emu_harness.emu_lib(), inside=16)
    CASES[module][0](Engine(lib, "cpu"))
    assert lib.damaged, "the guard band does not see writes"
