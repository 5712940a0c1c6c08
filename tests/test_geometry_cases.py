"""CPU: the case table of tests/geometry_cases.py checked before it reaches a GPU -- the restated launch geometry against the
library's own workspace size, every precondition a case states (which geometry it reaches), the reference's fp32 noise on every case
(half the 1e-4 gate at most, tests/golden/geometry_reference_noise.json), and the cases of the `small` scene with at most 64 rays
through the CPU emulator of the kernel sources against the oracle.

Left out of the emulator run, which would otherwise take two and a half minutes: the `waves` group (28..341 rays), the 43-ray cases
of `oneblock` but the colour-stage cap-1 one (129 tiles in one block: the live-mask chunk crossed twice), the cap-0 half of `subsets` (37 rays; the cap-2 half runs), `hot` (300 rays at Replica shapes) and `coarselds` (another
scene).  The emulator suite reaches their logic at small sizes through its variant builds (tests/test_emu_parity.py)."""
import shutil
import os

import numpy as np
import pytest
import torch

import geometry_cases as gc
import scene_util as su
from nice_slam_amd import _capi

_REFS = {}


def _reference(case):
    """(scene, fp32 oracle result) of a case, shared by the cases with the same rays (never modified)."""
    k = gc.ref_key(case)
    if k not in _REFS:
        sc = gc.case_scene(case)
        _REFS[k] = (sc, gc.case_oracle(case, sc))
    return _REFS[k]


@pytest.fixture(scope="module")
def emu():
    if not (os.path.exists("/opt/rocm/lib/llvm/bin/clang++") or shutil.which("clang++")):
        pytest.skip("no host clang++ for the emulator build")
    from emu_harness import emu_lib
    return emu_lib()


def test_expected_geo_matches_the_library(emu):
    """nsr_bwd_workspace_floats = passes * (nimg * max_params + nb * 288): ``nimg`` and ``nb`` of split_geo enter with different
    weights, and they move differently with the ray count, so a restatement that is wrong in either shows over the sweep (two stages
    with different `max_params`, every pass count)."""
    n_checked = 0
    for stage in gc.PASSES:
        max_params = emu.nsr_param_count(0 if stage == "coarse" else 2)
        for S in (1, 2, 16, 25, 32, 33, 48, 64):
            for cap in (0, 1, 2, 3, 4, 6, 7, 85, 256, 1000):
                for n in list(range(0, 60)) + [85, 86, 171, 256, 341, 342, 1000, 1365, 1366, 5000, 100000]:
                    got = emu.nsr_bwd_workspace_floats(_capi.STAGE_ID[stage], n, S, cap)
                    assert got == gc.workspace_floats(stage, n, S, cap, max_params), (stage, n, S, cap, got, gc.expected_geo(stage, n, S, cap))
                    n_checked += 1
    assert n_checked > 20000
    for c in gc.CASES:                                       # ... and at every case of the table
        max_params = emu.nsr_param_count(0 if c.stage == "coarse" else 2)
        S = gc.samples_per_ray(c)
        assert emu.nsr_bwd_workspace_floats(_capi.STAGE_ID[c.stage], c.n_rays, S, c.cap) == gc.workspace_floats(c.stage, c.n_rays, S, c.cap, max_params), c.name


def test_wave_counts_are_covered():
    """the `waves` group reaches every block size of the dX kernel, and a 12-wave block with more tiles than waves"""
    geos = [gc.case_geo(c) for c in gc.CASES if c.group == "waves" and c.stage == "color"]
    assert {g["waves"] for g in geos} == set(range(1, gc.MAX_WAVES + 1))
    assert all(g["per_pass"] == 85 for g in geos)
    assert any(g["waves"] == gc.MAX_WAVES and g["tiles_per_block"] > gc.MAX_WAVES for g in geos)
    for stage in ("middle", "fine"):
        assert len({gc.case_geo(c)["waves"] for c in gc.CASES if c.group == "waves" and c.stage == stage}) == 3
    # sample counts: S = 1, 2, 16, 25, 64 and 33; S = 25: a 16-point tile straddles two rays
    assert {gc.samples_per_ray(c) for c in gc.CASES if c.group == "samples"} == {1, 2, 16, 25, 64, 33}
    # every <STAGE, RAYS> instantiation of the dX kernel, with and without parameter gradients
    for stage in gc.PASSES:
        wants = {c.want for c in gc.CASES if c.group == "subsets" and c.stage == stage}
        assert wants == {("rays",), ("grids",), ("params",), ("grids", "params")}
    # two blocks per pass: an odd tile count (unequal ranges) and an even one
    assert {gc.case_geo(c)["tiles"] % 2 for c in gc.CASES if c.group == "twoblocks"} == {0, 1}


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.expect])
def test_case_reaches_its_geometry(name):
    c = gc.BY_NAME[name]
    geo = gc.case_geo(c)
    exp = dict(c.expect)
    for k in ("waves", "nb"):
        if k in exp:
            assert geo[k] == exp.pop(k), (name, k, geo)
    if "min_tiles_per_block" in exp:
        assert geo["tiles_per_block"] >= exp.pop("min_tiles_per_block"), (name, geo)
    if "hot_voxels" in exp:
        # every sample is a candidate of the hot-voxel table, and the voxels they touch outnumber the largest table a block can have
        sc = _reference(c)[0]
        z, pts = gc.sample_points(c, sc)
        assert float(z.max()) < gc.hot_depth(sc, "grid_fine") <= gc.hot_depth(sc, "grid_middle"), (float(z.max()), gc.hot_depth(sc, "grid_fine"))
        assert gc.touched_voxels(sc, "grid_fine", pts) >= exp.pop("hot_voxels"), gc.touched_voxels(sc, "grid_fine", pts)
        assert sc["grids"]["grid_color"].shape == sc["grids"]["grid_fine"].shape
    if "coarse_voxels" in exp:
        sc = _reference(c)[0]
        Z, Y, X = sc["grids"]["grid_coarse"].shape[2:]
        assert Z * Y * X >= exp.pop("coarse_voxels") and sc["grids"]["grid_coarse"].shape[1] == gc.C_DIM
    assert not exp, (name, exp)


def _first_of_each_reference():
    seen = {}
    for c in gc.CASES:
        seen.setdefault(gc.ref_key(c), c)
    return list(seen.values())


def test_noise_table_is_complete():
    noise = gc.committed_noise()
    assert set(noise) == {c.name for c in gc.CASES}
    for name, e in noise.items():
        assert 0.0 <= e["fp32_vs_fp64"] < gc.NOISE_BOUND, (name, e)


@pytest.mark.parametrize("name", [c.name for c in _first_of_each_reference()])
def test_reference_is_quiet_enough_for_the_gate(name):
    """The gate of the GPU test is 1e-4 against the fp32 oracle.  That is fair where the fp32 oracle itself sits within half of it
    of the fp64 oracle (same sample positions) on every tensor that may not take the secondary gate: the product is left as much
    room again as the reference's own rounding takes.  A case that fails has a sample on a relu kink or on the bound override:
    change its seed (geometry_cases.SEED_OF), not the bound."""
    c = gc.BY_NAME[name]
    sc, ref = _reference(c)
    val, tensor = gc.reference_noise(c, sc, ref)
    print("%s: fp32 vs fp64 oracle %.2e (%s)" % (name, val, tensor))
    assert val < gc.NOISE_BOUND, (name, tensor, val)
    noise = gc.committed_noise()
    for other in gc.CASES:                                  # the committed value of every case on these rays is this measurement,
        if gc.ref_key(other) == gc.ref_key(c):              # to a factor of two: the oracle's fp32 rounding moves with the host's BLAS,
            e = noise[other.name]                           # a case whose seed or shape was edited moves by far more
            assert e["tensor"] in ref and e["fp32_vs_fp64"] < gc.NOISE_BOUND, (other.name, e)
            assert 0.5 * val <= e["fp32_vs_fp64"] <= 2.0 * val, (other.name, e, val, "stale: run `python tests/geometry_cases.py`")


EMU_CASES = [c for c in gc.CASES if c.scene == "small" and (c.n_rays <= 23 or (c.group == "subsets" and c.cap == 2) or
                                                             (c.group == "oneblock" and c.n_rays == 43 and c.stage == "color" and c.cap == 1))]


@pytest.mark.parametrize("name", [c.name for c in EMU_CASES])
def test_case_on_the_emulator(emu, name):
    """the case as the GPU test runs it -- same scene, sample counts, cap and gradient subset -- through the kernel sources on the CPU"""
    from emu_harness import HostScene
    c = gc.BY_NAME[name]
    sc, ref = _reference(c)
    hs = HostScene(emu, sc["grids"], sc["params"], sc["bound"].numpy(), 2.0, n_samples=c.samples[0], n_surface=c.samples[1])
    fwd = hs.forward(c.stage, sc["rays_o"].numpy(), sc["rays_d"].numpy(), sc["gt_depth"].numpy() if c.with_depth else None)
    assert fwd["raw"].shape[1] == gc.samples_per_ray(c)
    w = sc["w"]
    res = hs.backward(c.stage, fwd, w["depth"].numpy(), w["var"].numpy(), w["rgb"].numpy(), want_grid="grids" in c.want,
                      want_params="params" in c.want, want_rays="rays" in c.want, max_blocks=c.cap)
    got = dict(res, depth=fwd["depth"], var=fwd["var"], rgb=fwd["rgb"])
    keys = gc.wanted_keys(c, ref)
    assert set(keys) <= set(got), sorted(set(keys) - set(got))
    bad = su.parity_failures(got, sc, c.stage, tol=1e-4, with_depth=c.with_depth, ref={k: ref[k] for k in keys}, tag="geo/" + name,
                             n_samples=c.samples[0], n_surface=c.samples[1])
    assert not bad, (name, bad)
    for k in set(got) - set(keys):
        assert k not in ref and float(np.abs(got[k]).max()) == 0.0, (name, k)
