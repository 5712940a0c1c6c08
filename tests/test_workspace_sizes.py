"""What every size entry of the library reports (nsr_*_workspace_bytes, nsr_jpeg_size, ...), held to
tests/golden/workspace_sizes.json: a record of the commit BEFORE the workspaces were described once each, by a function that
both measures and binds them (nsr_api.cpp: Carve).  For every such entry: shapes where no piece's byte count is a multiple of
16 (as far as its element sizes allow), the largest sizes it accepts, and every rejection; and a few shapes of the entries
that change did not touch.  tests/golden/make_golden_workspace_sizes.py mints the file through ``collect``.

These are host functions that launch nothing: the same table is asked of the emulator library and of libnsr.so."""
import ctypes as C
import json
import os

import pytest

import emu_harness
from nice_slam_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")
I31 = 2147483647


def nn_plan(nd, cells=None, lo=(0.0, 0.0, 0.0), h=0.5):
    """a plan as nsr_nn_plan writes it (nsr_recon.h: kNnLo ..), for a grid of nd cells; ``cells``: a wrong cell count"""
    nc = [-(-n // 8) for n in nd]
    hi = [lo[d] + h * nd[d] for d in range(3)]
    ncell = nd[0] * nd[1] * nd[2] if cells is None else cells
    return (C.c_double * 16)(*lo, *hi, h, *nd, *nc, ncell, nc[0] * nc[1] * nc[2], 1e-12)


def planned(lib, entry, n):
    """the plan the library makes for n items in the unit cube"""
    plan = (C.c_double * 16)()
    lib.call(entry, (C.c_double * 6)(0, 0, 0, 1, 1, 1), n, plan)
    return plan


def frame_desc(color=(17, 13), depth=(17, 13), distortion=1, **kw):
    d = _capi.NsrFrameDesc()
    d.color_h, d.color_w, d.depth_h, d.depth_w = *color, *depth
    d.has_distortion, d.fx, d.fy, d.png_depth_scale, d.scale = distortion, 600.0, 600.0, 6553.5, 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def by_pointer(lib, entry, args, n_out):
    """an entry that returns an error code and writes its sizes through pointers: [rc, the sizes | the error message]"""
    out = [C.c_int64(-7) for _ in range(n_out)]
    rc = getattr(lib, entry)(*args, *[C.byref(o) for o in out])
    return [rc] + ([o.value for o in out] if rc == 0 else [lib.nsr_last_error().decode()])


def collect(lib):
    """{"entry(arguments)": what it returns}"""
    out = {}

    def put(entry, *args, label=None, value=None):
        key = f"{entry}({', '.join(str(a) for a in args) if label is None else label})"
        assert key not in out, key
        out[key] = int(getattr(lib, entry)(*args)) if value is None else value

    # ---- marching cubes: 27 and 693 points, 2^31 points, every dimension below 2, more than 2^31 points
    for shape in [(3, 3, 3), (7, 9, 11), (2, 2, 2), (2048, 1024, 1024), (1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 0, 0), (2048, 1024, 1025)]:
        put("nsr_mc_workspace_bytes", *shape)
    # ---- TSDF unit bitmap: 27 bits, 1155 bits (37 words), 257 word blocks + 1 word, 2^31 bits; empty, too long, too many, no box
    for box in [(0, 0, 0, 2, 2, 2), (-4, 1, 2, 28, 5, 8), (0, 0, 0, 65536, 31, 0), (0, 0, 0, 2097151, 1023, 0),
                (0, 0, 0, -1, 2, 2), (0, 0, 0, 2, 2, 1 << 21), (0, 0, 0, 2097151, 1023, 1)]:
        put("nsr_tsdf_workspace_bytes", (C.c_int32 * 6)(*box), label=str(box))
    put("nsr_tsdf_workspace_bytes", None)
    # ---- nearest neighbour: 5 points over 27 cells, 77 over 3 x 11 x 9 (two coarse cells), the largest reference set
    put("nsr_nn_workspace_bytes", nn_plan((3, 3, 3)), 5, label="3x3x3, 5")
    put("nsr_nn_workspace_bytes", nn_plan((3, 11, 9)), 77, label="3x11x9, 77")
    put("nsr_nn_workspace_bytes", planned(lib, "nsr_nn_plan", I31 - 1), I31 - 1, label="planned, 2^31 - 2")
    # rejections: no plan, no points, more cells than 4 m + 64, a cell count that is not the product, an open box, a zero cell
    put("nsr_nn_workspace_bytes", None, 5, label="null, 5")
    put("nsr_nn_workspace_bytes", nn_plan((3, 3, 3)), 0, label="3x3x3, 0")
    put("nsr_nn_workspace_bytes", nn_plan((9, 9, 9)), 5, label="9x9x9, 5")
    put("nsr_nn_workspace_bytes", nn_plan((3, 3, 3), cells=28), 5, label="3x3x3 of 28 cells, 5")
    put("nsr_nn_workspace_bytes", nn_plan((3, 3, 3), lo=(0.0, float("inf"), 0.0)), 5, label="3x3x3 from inf, 5")
    put("nsr_nn_workspace_bytes", nn_plan((3, 3, 3), h=0.0), 5, label="3x3x3 of h = 0, 5")
    put("nsr_nn_workspace_bytes", nn_plan((0, 3, 3)), 5, label="0x3x3, 5")
    put("nsr_nn_workspace_bytes", nn_plan(((1 << 20) + 1, 1, 1)), 1 << 20, label="(2^20 + 1)x1x1, 2^20")
    # ---- mesh distance: the same grids for faces, with pair and oversize counts that are no multiple of four
    put("nsr_meshdist_workspace_bytes", nn_plan((3, 3, 3)), 3, 7, 1, label="3x3x3, 3, 7, 1")
    put("nsr_meshdist_workspace_bytes", nn_plan((3, 11, 9)), 77, 5 * 77 + 3, 7, label="3x11x9, 77, 388, 7")
    put("nsr_meshdist_workspace_bytes", nn_plan((3, 3, 3)), 3, 0, 0, label="3x3x3, 3, 0, 0")
    nf = I31 // 3
    put("nsr_meshdist_workspace_bytes", planned(lib, "nsr_meshdist_plan", nf), nf, I31 - 1, nf, label="planned, (2^31 - 1) / 3, 2^31 - 2, nf")
    for lab, plan, m, npairs, nover in [("null", None, 3, 7, 1), ("no faces", nn_plan((3, 3, 3)), 0, 0, 0), ("too many cells", nn_plan((9, 9, 9)), 3, 7, 1),
                                        ("negative pairs", nn_plan((3, 3, 3)), 3, -1, 1), ("negative oversize", nn_plan((3, 3, 3)), 3, 7, -1),
                                        ("oversize > nf", nn_plan((3, 3, 3)), 3, 7, 4), ("pairs > 32 nf", nn_plan((3, 3, 3)), 3, 97, 1),
                                        ("pairs = 32 nf", nn_plan((3, 3, 3)), 3, 96, 3),
                                        ("pairs >= 2^31 - 1", planned(lib, "nsr_meshdist_plan", nf), nf, I31, 0)]:
        put("nsr_meshdist_workspace_bytes", plan, m, npairs, nover, label=f"{lab}: {m}, {npairs}, {nover}")
    # ---- raster and view: 5 vertices, 3 faces, one 9 x 9 view; several views, tiles and chunks; the largest mesh and image
    shapes = [(5, 3, 1, 9, 9), (301, 517, 3, 45, 70), (1, 1, 1, 1, 1), (I31, I31, 1, 1024, 1024),
              (0, 3, 1, 9, 9), (5, 0, 1, 9, 9), (5, 3, 0, 9, 9), (5, 3, 1, 0, 9), (5, 3, 1, 9, 0), (5, 3, 1, 1025, 9), (5, 3, 1, 9, 1025),
              (I31 + 1, 3, 1, 9, 9), (5, I31 + 1, 1, 9, 9)]
    for s in shapes:
        put("nsr_raster_workspace_bytes", *s)
    for s in shapes[:2] + shapes[3:5] + shapes[9:10]:
        put("nsr_view_workspace_bytes", *s)
    # ---- JPEG encode: three 17 x 13 frames, both samplings; the most blocks one call takes (10 frames of 65535 x 65535)
    for a in [(3, 17, 13, 0), (3, 17, 13, 2), (1, 1, 1, 0), (0, 17, 13, 2), (10, 65535, 65535, 0), (65535, 1024, 1024, 2),
              (-1, 17, 13, 0), (65536, 17, 13, 0), (3, 0, 13, 0), (3, 17, 0, 0), (3, 65536, 13, 0), (3, 17, 65536, 0), (3, 17, 13, 1),
              (3, 17, 13, 3), (11, 65535, 65535, 0), (65535, 65535, 8, 0)]:
        put("nsr_jpeg_size", *a, value=by_pointer(lib, "nsr_jpeg_size", a, 2))
    one = C.c_int64()
    put("nsr_jpeg_size", label="3, 17, 13, 0, null, out", value=[lib.nsr_jpeg_size(3, 17, 13, 0, None, C.byref(one)), lib.nsr_last_error().decode()])
    put("nsr_jpeg_size", label="3, 17, 13, 0, ws, null", value=[lib.nsr_jpeg_size(3, 17, 13, 0, C.byref(one), None), lib.nsr_last_error().decode()])
    # ---- JPEG decode: the four samplings; the most blocks one call takes, in colour and in grey (the block limit is met before
    # the pixel limit at every sampling)
    for a in [(3, 17, 13, 0, 1000, 16), (3, 17, 13, 1, 1000, 16), (3, 17, 13, 2, 1000, 1024), (3, 17, 13, 3, 0, 20), (5, 33, 47, 2, 1 << 28, 16),
              (0, 17, 13, 0, 1000, 16), (10, 65535, 65535, 0, 1 << 28, 1024), (31, 65535, 65535, 3, 1000, 16),
              (-1, 17, 13, 0, 1000, 16), (65536, 17, 13, 0, 1000, 16), (3, 0, 13, 0, 1000, 16), (3, 17, 65536, 0, 1000, 16),
              (3, 17, 13, -1, 1000, 16), (3, 17, 13, 4, 1000, 16), (3, 17, 13, 0, 1000, 12), (3, 17, 13, 0, 1000, 18), (3, 17, 13, 0, 1000, 1028),
              (3, 17, 13, 0, -1, 16), (3, 17, 13, 0, (1 << 28) + 1, 16), (11, 65535, 65535, 0, 1000, 16), (32, 65535, 65535, 3, 1000, 16)]:
        put("nsr_jpegdec_size", *a, value=by_pointer(lib, "nsr_jpegdec_size", a, 1))
    put("nsr_jpegdec_size", label="3, 17, 13, 0, 1000, 16, null", value=[lib.nsr_jpegdec_size(3, 17, 13, 0, 1000, 16, None), lib.nsr_last_error().decode()])
    # ---- image metrics: one tile, 2 x 3 tiles, the largest batch of the largest images
    for a in [(3, 17, 13), (5, 43, 75), (0, 17, 13), (1, 11, 11), (65535, 32768, 32768),
              (-1, 17, 13), (65536, 17, 13), (3, 10, 13), (3, 17, 10), (3, 32769, 13), (3, 17, 32769)]:
        put("nsr_image_metrics_workspace_bytes", *a)
    # ---- frame preparation: only distortion needs a workspace
    put("nsr_frame_workspace_bytes", C.byref(frame_desc()), 3, label="17x13 distorted, 3")
    put("nsr_frame_workspace_bytes", C.byref(frame_desc(distortion=0)), 3, label="17x13, 3")
    put("nsr_frame_workspace_bytes", C.byref(frame_desc()), 0, label="17x13 distorted, 0")
    put("nsr_frame_workspace_bytes", C.byref(frame_desc(color=(32768, 32768), depth=(32768, 32768))), 65535, label="32768x32768 distorted, 65535")
    put("nsr_frame_workspace_bytes", C.byref(frame_desc()), -1, label="17x13 distorted, -1")
    put("nsr_frame_workspace_bytes", None, 3, label="null, 3")
    for lab, kw in [("colour side 0", dict(color=(0, 13))), ("depth side 32769", dict(depth=(17, 32769))), ("crop_h alone", dict(crop_h=8)),
                    ("negative crop", dict(crop_h=-1, crop_w=-1)), ("depth_type 2", dict(depth_type=2)), ("crop_edge 7", dict(crop_edge=7)),
                    ("negative crop_edge", dict(crop_edge=-1)), ("png_depth_scale 0", dict(png_depth_scale=0.0)), ("fx 0", dict(fx=0.0)),
                    ("fy inf", dict(fy=float("inf")))]:
        put("nsr_frame_workspace_bytes", C.byref(frame_desc(**kw)), 3, label=lab + ", 3")
    # ---- depth error partials
    for a in [(1, 117), (3, 1), (7, 70001), (65535, 1 << 40), (0, 117), (1, 0)]:
        put("nsr_depth_error_partial_doubles", *a)
    # ---- entries that are not described by a Carve: unchanged, a few shapes each
    for a in [(0, 96, 48), (3, 96, 48), (3, 1001, 64), (1, 0, 1), (4, 96, 48), (3, -1, 48), (3, 96, 65), (3, 96, 0)]:
        put("nsr_acts_floats", *a)
    for a in [(0, 96, 48, 0), (3, 96, 48, 0), (3, 1001, 64, 7), (2, 5000, 40, 300), (4, 96, 48, 0), (3, 96, 65, 0)]:
        put("nsr_bwd_workspace_floats", *a)
    for a in [(0,), (27,), (256,), (1000001,), (-1,)]:
        put("nsr_frustum_workspace_floats", *a)
        put("nsr_sample_workspace_bytes", *a)
        put("nsr_recon_partial_doubles", *a)
    for a in [(27, 10, 3), (1000, 1000, 1), (0, 1, 0), (27, 0, 3), (-1, 10, 3), (27, 10, -1)]:
        put("nsr_point_masks_workspace_floats", *a)
    put("nsr_hull_partial_doubles")
    return out


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)["sizes"]


def check(lib, gold):
    got = collect(lib)
    assert list(got) == list(gold)
    wrong = {k: (got[k], gold[k]) for k in gold if got[k] != gold[k]}
    assert not wrong, wrong


def test_sizes_as_parent_emu(gold):
    check(emu_harness.emu_lib(), gold)


@pytest.mark.gpu
def test_sizes_as_parent_device(gold):
    check(_capi.get_lib(), gold)
