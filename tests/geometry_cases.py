"""TEST INFRASTRUCTURE: the launch geometries of the split backward as a table of named cases.

``render_bwd_split`` / ``split_geo`` (nice_slam_amd/csrc/nsr_api.cpp) decide per call: waves per dX block (1..12), blocks per decoder
pass (from the persistent-grid cap ``Renderer.bwd_max_blocks``), the contiguous range of tiles a block owns, the 64-tile live-mask chunks,
the DMA ring of the dW kernel, the hot-voxel LDS table and whether the coarse gradient grid sits in LDS.  ``CASES`` names one input per
geometry; tests/test_hip_geometry.py runs every case on the GPU against the oracle, tests/test_geometry_cases.py checks the table itself
(what geometry a case reaches, that its reference is quiet enough for the 1e-4 gate) and runs the small cases on the CPU emulator.

``expected_geo`` restates ``split_geo`` from its header comment, so that a case can SAY which geometry it is there for; a change of the
policy constants then fails a precondition instead of silently moving the coverage.
"""
import collections
import json
import os

import numpy as np
import torch

import scene_util as su
from oracle import nice_oracle as orc

# ---- the launch policy, restated (nsr_api.cpp: kDefaultBwdBlocks, nsr::kTile, nsr::kDxMaxWaves, nsr::kDbPart, kHotCells, kHotSlotCap, kLdsLimit)
DEFAULT_BLOCKS = 256
TILE = 16
MAX_WAVES = 12
DB_PART = 288
HOT_CELLS = 6
HOT_SLOT_CAP = 512
LDS_BYTES = 160 * 1024
C_DIM = 32
MASK_CHUNK = 64                       # tiles per live-mask chunk of a block's tile sequence
PASSES = {"coarse": 1, "middle": 1, "fine": 2, "color": 3}
LDS_GRID_VOXELS = LDS_BYTES // (4 * C_DIM)        # 1280: a coarse gradient grid with more voxels cannot sit in LDS whatever else is there

ALL = ("grids", "params", "rays")
NOISE_BOUND = 5e-5                    # fp32 oracle vs fp64 oracle, per tensor off the `everywhere` list: half the 1e-4 gate
NOISE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_reference_noise.json")


def expected_geo(stage, n_rays, S, cap):
    """``split_geo``: the dX kernel runs ``nb`` blocks of ``waves`` waves per decoder pass, the dW kernel ``nimg`` blocks per pass.
    -> dict(tiles, passes, per_pass, waves, nb, nimg, tiles_per_block) -- tiles_per_block: the longest tile sequence of a dX block."""
    passes = PASSES[stage]
    tiles = (n_rays * S + TILE - 1) // TILE
    per_pass = max(1, (cap if cap > 0 else DEFAULT_BLOCKS) // passes)
    waves = min(MAX_WAVES, max(1, (tiles + per_pass - 1) // per_pass))
    nb = min(per_pass, max(1, (tiles + waves - 1) // waves))
    nimg = max(1, min(per_pass, tiles))
    return dict(tiles=tiles, passes=passes, per_pass=per_pass, waves=waves, nb=nb, nimg=nimg, tiles_per_block=(tiles + nb - 1) // nb)


def workspace_floats(stage, n_rays, S, cap, max_params):
    """``nsr_bwd_workspace_floats`` from ``expected_geo``: ``nimg`` partial images of the gradient blob and ``nb`` d _B partials per pass."""
    g = expected_geo(stage, n_rays, S, cap)
    return g["passes"] * (g["nimg"] * max_params + g["nb"] * DB_PART)


Case = collections.namedtuple("Case", "name group scene seed n_rays stage samples with_depth cap want depth_range edge fine_scale expect")


def _case(group, n_rays, stage, cap, seed, scene="small", samples=(32, 16), with_depth=True, want=ALL, depth_range=None, edge=False,
          fine_scale=100.0, **expect):
    name = "%s-%s-n%d-s%d+%d%s-cap%d" % (group, stage, n_rays, samples[0], samples[1], "" if with_depth else "nodepth", cap)
    if want != ALL:
        name += "-" + "+".join(want)
    if scene != "small":
        name += "-" + scene
    return Case(name, group, scene, seed, n_rays, stage, tuple(samples), with_depth, cap, tuple(want), depth_range, edge, fine_scale, expect)


def samples_per_ray(case):
    guided = case.with_depth and case.stage != "coarse"
    return case.samples[0] + (case.samples[1] if guided else 0)


def case_geo(case):
    return expected_geo(case.stage, case.n_rays, samples_per_ray(case), case.cap)


def ref_key(case):
    """Cases with the same key share scene, rays and reference result: they differ in cap and gradient subset only."""
    return (case.scene, case.seed, case.n_rays, case.stage, case.samples, case.with_depth, case.depth_range, case.edge, case.fine_scale)


def case_scene(case):
    sc = su.make_scene(seed=case.seed, n_rays=case.n_rays, scene=case.scene, fine_scale=case.fine_scale, depth_range=case.depth_range)
    if case.edge:                               # the three edits of test_hip_parity.py::test_edge_cases
        assert case.n_rays >= 3
        sc["gt_depth"][0] = 0.0                 # zero-depth ray -> surface samples spread over [0.001, max]
        sc["gt_depth"][1] = 50.0                # far beyond the box: most samples out of bound -> occ forced to 100
        sc["rays_d"][2] = torch.tensor([0.0, 0.0, -1.0])      # axis-aligned ray: divisions by zero in far_bb
    return sc


def case_oracle(case, sc, lo=torch.float32):
    return su.oracle_render(sc, case.stage, backward=True, with_depth=case.with_depth, lo=lo,
                            n_samples=case.samples[0], n_surface=case.samples[1])


def wanted_keys(case, ref):
    """The keys of the oracle's result that a product call with the case's gradient subset returns."""
    keep = {"d_rays": "rays", "d_grid": "grids", "dparam": "params"}
    return [k for k in ref if k in su.PRIMARY_ONLY or keep[k[:6]] in case.want]


def sample_points(case, sc):
    """The oracle's sample depths [n, S] and positions [n * S, 3] (fp64)."""
    gd = sc["gt_depth"] if case.with_depth else None
    z = orc.sample_depths(sc["rays_o"], sc["rays_d"], gd, sc["bound"], case.stage, case.samples[0], case.samples[1])
    pts = sc["rays_o"][:, None, :].double() + sc["rays_d"][:, None, :].double() * z[:, :, None]
    return z, pts.reshape(-1, 3)


def touched_voxels(sc, grid, pts):
    """How many voxels of feature grid ``grid`` the trilinear lookups of ``pts`` touch (the eight corners of each point's cell)."""
    Z, Y, X = sc["grids"][grid].shape[2:]
    b = sc["bound"]
    u = ((pts - b[:, 0]) / (b[:, 1] - b[:, 0])).numpy() * np.array([X - 1, Y - 1, Z - 1], dtype=np.float64)
    i0 = np.floor(u).astype(np.int64)
    seen = set()
    for corner in range(8):
        c = i0 + np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])
        c = np.clip(c, 0, [X - 1, Y - 1, Z - 1])
        seen.update(((c[:, 2] * Y + c[:, 1]) * X + c[:, 0]).tolist())
    return len(seen)


def hot_depth(sc, grid):
    """``RenderParams.hot_z`` of a grid: samples closer to their ray's origin than HOT_CELLS times the grid's largest cell edge use
    the dX block's hot-voxel table."""
    Z, Y, X = sc["grids"][grid].shape[2:]
    ext = (sc["bound"][:, 1] - sc["bound"][:, 0]).tolist()
    return HOT_CELLS * max(e / (n - 1) for e, n in zip(ext, (X, Y, Z)) if n > 1)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# Seeds: one per ray count and group, so that a case whose reference turns out noisy (a sample on a relu kink or on the bound
# override: fp32 vs fp64 oracle beyond NOISE_BOUND, tests/test_geometry_cases.py) is moved alone.  SEED_OF overrides the default.
SEED_OF = {(500, 28): 1528, (500, 29): 1529, (500, 114): 2614, (500, 199): 2699, (500, 227): 4727, (500, 256): 4756, (500, 312): 3812,
           (500, 341): 4841, (600, 21): 1621, (600, 43): 1643, (600, 5): 2605, (700, 23): 4723, (800, 64): 1864, (800, 300): 1271, (900, 22): 17922,
           (900, 23): 3923}


def _seed(group_base, n_rays):
    return SEED_OF.get((group_base, n_rays), group_base + n_rays)


def _build():
    cases = []
    # every wave count of a dX block: colour stage, S = 48, default cap -> 85 blocks per pass; 1, 2, ... 12 waves, then 12 waves with
    # more tiles than waves
    wave_rays = (28, 29, 57, 86, 114, 142, 171, 199, 227, 256, 284, 312, 341)
    for i, n in enumerate(wave_rays):
        exp = dict(waves=min(i + 1, 12))
        if i == 12:
            exp["min_tiles_per_block"] = 13
        cases.append(_case("waves", n, "color", 0, _seed(500, n), **exp))
    for n, w in ((57, 1), (171, 3), (341, 4)):              # one pass: 256 blocks
        cases.append(_case("waves", n, "middle", 0, _seed(500, n), waves=w))
    for n, w in ((86, 3), (199, 5), (312, 8)):              # two passes: 128 blocks each
        cases.append(_case("waves", n, "fine", 0, _seed(500, n), waves=w))
    # one block per pass: it owns every tile of its pass; 22 rays x 48 samples = 66 tiles cross the 64-tile live-mask chunk inside one
    # block, 43 rays = 129 tiles cross it twice, and the dW kernel's ring wraps many times.  (Cap 3 leaves the one-pass stages three
    # blocks: same inputs, the other deal.)
    for stage in ("color", "fine", "middle", "coarse"):
        for cap in (1, 3):
            for n in (1, 2, 3, 21, 22, 43):
                exp = dict(nb=1) if cap // PASSES[stage] <= 1 else {}
                if stage != "coarse" and exp and n in (22, 43):
                    exp["min_tiles_per_block"] = {22: MASK_CHUNK + 1, 43: 2 * MASK_CHUNK + 1}[n]
                cases.append(_case("oneblock", n, stage, cap, _seed(600, n), **exp))
    # two blocks per pass: block i of n owns the tiles [T i / n, T (i + 1) / n) (nsr_bwd2.h); 5 rays = 15 tiles split 7 + 8 (the boundary
    # inside a ray), 22 rays = 66 tiles split 33 + 33 (the boundary between two rays)
    for n in (5, 22):
        for stage, cap in (("color", 6), ("color", 7), ("fine", 4)):
            cases.append(_case("twoblocks", n, stage, cap, _seed(600, n), nb=2))
    # other sample counts: S = 1, 2, 16, 25 (a tile straddles two rays), 64, and 33 without depth
    for ns, nsurf, wd in ((1, 0, True), (1, 1, True), (16, 0, True), (20, 5, True), (40, 24, True), (33, 0, False)):
        for n in (7, 23):
            caps = (0, 3) if (ns, nsurf) in ((20, 5), (40, 24)) else (0,)
            for cap in caps:
                cases.append(_case("samples", n, "color", cap, _seed(700, n), samples=(ns, nsurf), with_depth=wd))
    # gradient subsets: the dX <STAGE, RAYS> instantiations and the light-pass block deal
    for stage in ("color", "fine", "middle", "coarse"):
        for want in (("rays",), ("grids",), ("params",), ("grids", "params")):
            for cap in (0, 2):
                cases.append(_case("subsets", 37, stage, cap, _seed(700, 37), want=want))
    # hot-voxel table under pressure: Replica room0 shapes, every sample a candidate of the table (closer to the camera than six cells of
    # the fine grid; with the grid's own cell edges, bound / (n - 1), that is 1.006 m: within the nominal 6 x 0.16 m = 0.96 m this
    # camera's frustum holds only ~500 fine voxels, fewer than the slot cap), more candidate voxels than the cap of 512 slots; one block
    # per pass (cap 3) must evict or fall back to memory atomics.  Cap 0: the uncontended counterpart.
    for cap in (3, 0):
        cases.append(_case("hot", 300, "color", cap, _seed(800, 300), scene="replica_room0", depth_range=(0.25, 0.83), fine_scale=1.0,
                           hot_voxels=HOT_SLOT_CAP + 1))
    # a coarse-stage backward whose gradient grid cannot sit in LDS
    cases.append(_case("coarselds", 64, "coarse", 0, _seed(800, 64), scene="coarse_dense", coarse_voxels=LDS_GRID_VOXELS + 1))
    cases.append(_case("coarselds", 1, "coarse", 1, _seed(800, 1), scene="coarse_dense", coarse_voxels=LDS_GRID_VOXELS + 1, nb=1))
    # ragged and degenerate rays inside these geometries: zero depth, depth far outside the box, an axis-aligned direction
    cases.append(_case("edge", 22, "color", 1, _seed(900, 22), edge=True, nb=1, min_tiles_per_block=MASK_CHUNK + 1))
    for cap in (0, 3):
        cases.append(_case("edge", 23, "color", cap, _seed(900, 23), samples=(20, 5), edge=True))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
GROUPS = sorted({c.group for c in CASES})


def cap_families():
    """Cases that share scene, rays, S and gradient subset and differ only in cap: [(first, [others ...])]."""
    fam = collections.OrderedDict()
    for c in CASES:
        fam.setdefault((ref_key(c), c.want), []).append(c)
    return [(v[0], v[1:]) for v in fam.values() if len(v) > 1]


def reference_noise(case, sc=None, ref=None):
    """The reference's own fp32 rounding on this case: fp32 oracle against the fp64 oracle on the same sample positions, the largest
    max|a-b| / max|b| over the tensors that are NOT on the `everywhere` list of tests/golden/secondary_gate.json.  -> (value, tensor)"""
    sc = sc or case_scene(case)
    ref = ref or case_oracle(case, sc)
    truth = case_oracle(case, sc, lo=torch.float64)
    everywhere = su._gate_table()["everywhere"]
    return max((su.rel_err(ref[k], truth[k]), k) for k in ref if k not in everywhere)


def committed_noise():
    return json.load(open(NOISE_FILE))["cases"]


if __name__ == "__main__":          # python tests/geometry_cases.py: measure every case's reference noise again and rewrite NOISE_FILE
    done, table = {}, collections.OrderedDict()
    for c_ in CASES:
        if ref_key(c_) not in done:
            done[ref_key(c_)] = reference_noise(c_)
        v_, t_ = done[ref_key(c_)]
        table[c_.name] = {"fp32_vs_fp64": float("%.3e" % v_), "tensor": t_}
        print("%-64s %.2e %s%s" % (c_.name, v_, t_, "" if v_ < NOISE_BOUND else "   <-- beyond NOISE_BOUND: change the seed"))
    json.dump({"_comment": "per case of tests/geometry_cases.py: the largest max|a-b|/max|b| between the fp32 and the fp64 oracle over the "
               "tensors that are not on the `everywhere` list of secondary_gate.json, and the tensor it is on; must stay below 5e-5 "
               "(tests/test_geometry_cases.py).  Rewritten by `python tests/geometry_cases.py`.", "cases": table}, open(NOISE_FILE, "w"), indent=1)
