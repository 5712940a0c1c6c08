"""CPU: the local parity gate of tests/local_gate.py checked on the reference alone, before it is asked of the product
(tests/test_hip_local_parity.py) -- every element of a grid gradient against its own mass s_v, every ray against its own scale.

* the reference's noise rho_ref per case and tensor (fp32 oracle and three one-ulp-perturbed draws against the fp64 oracle) is the
  committed one of tests/golden/local_gate_noise.json to a factor of 2 (only another BLAS's summation order may move it; regenerate
  with ``python tests/local_gate.py`` or NSR_LOCAL_GATE_REGEN=1);
* the gate has power: faults planted into the fp32 oracle's result -- the low-mass band of a grid gradient dropped, the band scaled by
  1.001, the boundary planes dropped, the shortest rays' outputs and the lowest-scale ray gradients scaled by 1.001 -- stand at least ten
  times above the gate 2 * rho_ref, and at least 1 % of a grid gradient's touched elements lie in the band.  A case that does not meet
  this is given another seed (``local_gate.SEED_OF``), never an exemption;
* the scale bounds the truth, |truth_v| <= s_v, and every case reaches the geometry it is there for.
"""
import math
import os

import numpy as np
import pytest
import torch

import geometry_cases as gc
import local_gate as lg
from oracle import nice_oracle as orc

NAMES = [c.name for c in lg.CASES]
_DATA = {}


@pytest.fixture(scope="module", autouse=True)
def _regenerate():
    if os.environ.get(lg.REGEN_ENV) == "1":
        lg.write_noise(lg.measure_all(verbose=False))
    yield


def _data(name):
    """(scene, fp64 truth, scales, fp32 oracle result) of a case: computed once, never modified"""
    if name not in _DATA:
        lc = lg.BY_NAME[name]
        sc = lg.case_scene(lc)
        truth, S = lg.case_truth(lc, sc)
        _DATA[name] = (sc, truth, S, lg.case_oracle(lc, sc))
    return _DATA[name]


def test_table_and_committed_file_agree():
    doc = lg.committed()
    assert set(doc) == {"_comment", "cases", "allowed"}
    assert set(doc["cases"]) == set(NAMES) and len(NAMES) <= 16
    for name in NAMES:
        lc = lg.BY_NAME[name]
        assert lc.case.n_rays <= 300 and lc.case.want == gc.ALL
        grids = ["d_grid_coarse"] if lc.case.stage == "coarse" else ["d_grid_middle", "d_grid_fine", "d_grid_color"][:gc.PASSES[lc.case.stage]]
        assert set(doc["cases"][name]) == set(lg.FORWARD + lg.RAY_GRADS) | set(grids), name
        for k, v in doc["cases"][name].items():
            assert (v == 0.0) == (k == "rgb" and lc.case.stage != "color"), (name, k, v)
            assert 0.0 <= v < 0.5 * lg.FAULT / lg.POWER, (name, k, v)        # else a 1.001 fault cannot stand 10 x above 2 rho_ref
    for e in doc["allowed"]:                                 # a tensor BY NAME with its measured ratio, never a blanket margin
        assert e["case"] in NAMES and e["tensor"] in doc["cases"][e["case"]] and e["argument"]
        assert lg.MARGIN < e["margin"] <= 2.0 * e["measured_ratio"], e
    assert {lg.BY_NAME[n].case.stage for n in NAMES if n.startswith("stage-")} == set(gc.PASSES)


def test_local_err_and_the_exact_zero_rule():
    t = np.array([[1.0, 1e-3], [0.0, -2.0]])
    S = np.array([[1.0, 1e-3], [0.0, 2.0]])
    x = t.copy()
    x[0, 1] *= 1.1                                          # 10 % off on the element at 5e-4 of the maximum: the max-norm sees 5e-5
    e, i = lg.local_err(x, t, S)
    assert i == (0, 1) and math.isclose(e, 1e-4 / (1e-3 + 2e-5), rel_tol=1e-12)
    x = t.copy()
    x[1, 0] = 1e-6                                          # an element nothing reaches: its error is measured against PHI * max S
    e, i = lg.local_err(x, t, S)
    assert i == (1, 0) and math.isclose(e, 1e-6 / 2e-5, rel_tol=1e-12)
    z = np.zeros((2, 3))
    assert lg.local_err(z, z, z) == (0.0, (0, 0))
    assert lg.local_err(-z, z, z)[0] == 0.0                 # a negative zero is a zero
    x = z.copy()
    x[1, 2] = 1e-30
    assert lg.local_err(x, z, z) == (float("inf"), (1, 2))


def test_the_oracle_is_restored_after_a_failed_run():
    orig = orc.trilinear
    sc = dict(_data("s1")[0])
    sc["w"] = None                                          # the loss fails after the forward has run through the wrapper
    with pytest.raises(Exception):
        lg.truth_and_scales(sc, "color", True, 1, 0)
    assert orc.trilinear is orig


@pytest.mark.parametrize("name", NAMES)
def test_scale_bounds_the_truth(name):
    sc, truth, S, ref = _data(name)
    lc = lg.BY_NAME[name]
    plain = gc.case_oracle(lc.case, sc, lo=torch.float64)   # the wrapper changes nothing: same numbers as the unwrapped fp64 oracle
    for k in lg.gated(truth):
        assert torch.equal(truth[k], plain[k]), (name, k)
        assert np.isfinite(S[k]).all() and (S[k] >= 0).all(), (name, k)
    for k in (k for k in truth if lg.is_grid(k)):
        t = np.abs(lg._np(truth[k]))
        assert (t <= S[k] * (1.0 + 1e-12)).all(), (name, k, float((t - S[k]).max()))
        assert (S[k] == S[k][:, :1]).all(), (name, k)       # one scale per voxel
        assert (t[S[k] == 0] == 0).all() and (S[k] > 0).any(), (name, k)
    for k in lg.RAY_GRADS:
        assert (S[k] > 0).all(), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_reference_noise_is_the_committed_one(name):
    sc, truth, S, ref = _data(name)
    rho = lg.reference_noise(lg.BY_NAME[name], sc, truth, S, ref)
    want = lg.committed_noise(name)
    print("%s: %s" % (name, "  ".join("%s %.2e (committed %.2e)" % (k, rho[k], want[k]) for k in rho)))
    assert list(rho) == lg.gated(truth) and set(rho) == set(want)
    for k, v in rho.items():
        if want[k] == 0.0:
            assert v == 0.0, (name, k, v)
        else:
            assert 0.5 * want[k] <= v <= 2.0 * want[k], (name, k, v, want[k], "stale: run `python tests/local_gate.py`")


@pytest.mark.parametrize("name", NAMES)
def test_planted_faults_stand_above_the_gate(name):
    """against the COMMITTED rho_ref, the one the product is held to"""
    sc, truth, S, ref = _data(name)
    lc = lg.BY_NAME[name]
    for k in lg.gated(truth):
        if float(S[k].max()) > 0.0:
            line = ", ".join("(%s) %.2e" % (f, lg.local_err(y, truth[k], S[k])[0]) for f, y in lg.planted(k, ref[k], truth, S).items())
            band = "band %d of %d touched, " % (lg.band_mask(S[k]).sum(), (S[k] > 0).sum()) if lg.is_grid(k) else ""
            print("%s %-14s gate %.2e  %s%s" % (name, k, lg.MARGIN * lg.committed_noise(name)[k], band, line))
    bad = lg.conditions(lc, sc, truth, S, ref, lg.committed_noise(name))
    assert not bad, (name, bad, "choose another seed in local_gate.SEED_OF")


def _inside(sc, pts):
    b = sc["bound"]
    return ((pts > b[:, 0]) & (pts < b[:, 1])).all(-1)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_geometry(name):
    lc = lg.BY_NAME[name]
    c = lc.case
    sc, truth, S, ref = _data(name)
    geo = gc.case_geo(c)
    z, pts = gc.sample_points(c, sc)
    if c.cap == 0:
        assert geo["nb"] > 1, geo
    if name.startswith("cap1") or name == "hot":
        assert geo["nb"] == 1 and geo["tiles_per_block"] == geo["tiles"] > gc.MASK_CHUNK, geo
    if name == "s1":
        assert gc.samples_per_ray(c) == 1 and c.n_rays > gc.TILE        # a full tile of sixteen rays and a ragged one
    if name == "s25":
        assert gc.samples_per_ray(c) == 25                  # tile 1 holds the last nine samples of ray 0 and the first seven of ray 1
    if name == "s64":
        assert gc.samples_per_ray(c) == 64
    if name == "nodepth":
        assert not c.with_depth and gc.samples_per_ray(c) == c.samples[0]
    if name == "hot":
        assert float(z.max()) < gc.hot_depth(sc, "grid_fine") <= gc.hot_depth(sc, "grid_middle")
        assert gc.touched_voxels(sc, "grid_fine", pts) >= c.expect["hot_voxels"] and sc["grids"]["grid_color"].shape == sc["grids"]["grid_fine"].shape
    if name == "coarselds":
        Z, Y, X = sc["grids"]["grid_coarse"].shape[2:]
        assert Z * Y * X > gc.LDS_GRID_VOXELS
    if name == "pastbound":
        out = ~_inside(sc, pts)
        assert 0.02 < float(out.double().mean()) < 0.5 and float(sc["gt_depth"].max()) > 1.28
        for k in ("d_grid_middle", "d_grid_fine", "d_grid_color"):
            assert lg.plane_mask(S[k]).any(), k
    if name == "halfzero":
        assert 0.35 < float((sc["gt_depth"] == 0).double().mean()) < 0.65
    if name == "short":
        # every ray ends within 5 % of the shortest bound edge ... and the batch maximum says little about the shortest of them
        d = lg._np(truth["depth"])
        assert float(sc["gt_depth"].max()) <= 0.05 * 1.28 * 1.01 and d.max() > 2.0 * d.min()
