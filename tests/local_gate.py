"""TEST INFRASTRUCTURE: a parity gate that holds every voxel and every ray of the render backward to its OWN scale.

The gates of ``scene_util.parity_failures`` are one number per tensor, max|a-b| / max|b|.  For a grid gradient [1,32,Z,Y,X] that number
is set by the few voxels in front of the surface; the voxels behind it, on a boundary plane or reached by one trilinear corner of
small weight carry 1e-2 .. 1e-5 of the maximum and may be 10 % wrong, or missing, under a 1e-4 gate.  Here the error of an element is
divided by what that element could have been:

* grid gradient, voxel v:   s_v = sum_m W[m,v] * ||dc_m||_inf  -- W the trilinear weight of point m at voxel v, dc_m the fp64 gradient
  with respect to the 32 features sampled at m.  The weights are non-negative, so s is the vector-Jacobian product of
  ``oracle.nice_oracle.trilinear`` on a zero fp64 grid leaf with the cotangent ||dc_m||_inf broadcast over the channels; |truth_v| <= s_v,
  and s_v = 0 exactly where no sample reaches.
* depth, var, rgb:          |truth|, per ray and channel (depth and var are sums of non-negative terms).
* d_rays_o:                 sum_i |dp_{r,i}| per component over the ray's samples, dp the fp64 gradient of the sample positions.
* d_rays_d:                 sum_i z_{r,i} |dp_{r,i}|, z_{r,i} = ||p_{r,i} - o_r|| / ||d_r||.
  (The sample depths' own dependence on the rays is not in these two sums; what it adds is in the reference's noise as well.)

``local_err`` = max |x - truth| / (S + PHI * max S).  The product is held to TWICE what the fp32 oracle and its one-ulp-perturbed draws
reach under the same statistic (``reference_noise``; the rule of ``parity_failures``).  The decoder-parameter gradients are dense sums
over all points, every element within a few orders of the maximum: the max-norm gate binds there and they are not gated here.

``CASES`` is the short table both test files run: tests/test_local_gate.py (CPU: the committed noise, the power of the gate against
planted faults) and tests/test_hip_local_parity.py (GPU: the product).  ``python tests/local_gate.py`` measures the reference noise of
every case again and rewrites tests/golden/local_gate_noise.json (NSR_LOCAL_GATE_REGEN=1 does the same from the CPU test).
"""
import collections
import json
import os

import numpy as np
import torch

import geometry_cases as gc
import scene_util as su
from oracle import nice_oracle as orc

PHI = 1e-5                      # floor of the scale, relative to the tensor's largest scale
MARGIN = 2.0                    # the product may be twice as noisy as the reference (parity_failures), not more
N_DRAWS = 3                     # ulp_perturbed draws next to the fp32 oracle, seeds 1234 + i as in parity_failures
BAND_HI = 1e-2                  # the low-mass band of the planted faults: PHI * max s < s_v < BAND_HI * max s
FORWARD = ("depth", "var", "rgb")
RAY_GRADS = ("d_rays_o", "d_rays_d")
NOISE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_gate_noise.json")
REGEN_ENV = "NSR_LOCAL_GATE_REGEN"


def _np(x):
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float64)


def is_grid(k):
    return k.startswith("d_grid")


def gated(keys):
    """The tensors of an oracle result that the local gate covers, in a fixed order."""
    return [k for k in FORWARD + RAY_GRADS if k in keys] + sorted(k for k in keys if is_grid(k))


# ---- truth and scales --------------------------------------------------------------------------------------------------------------
def truth_and_scales(sc, stage, with_depth=True, n_samples=32, n_surface=16):
    """One fp64 oracle backward.  -> (truth, S): the oracle's result dict and, per gated tensor, a float64 array of the tensor's shape."""
    records = []
    orig = orc.trilinear

    def recording(grid, p, bound, lo=orc.F32):
        out = orig(grid, p, bound, lo)
        if out.requires_grad:
            out.retain_grad()
        if p.requires_grad:
            p.retain_grad()
        records.append((p, bound, out))
        return out

    orc.trilinear = recording
    try:
        truth = su.oracle_render(sc, stage, backward=True, with_depth=with_depth, lo=torch.float64, n_samples=n_samples, n_surface=n_surface)
    finally:
        orc.trilinear = orig
    # call order: coarse; or middle, fine, color (the fine decoder reads the middle features detached: no record of its own)
    names = ["grid_coarse"] if stage == "coarse" else ["grid_middle", "grid_fine", "grid_color"][:gc.PASSES[stage]]
    assert len(records) == len(names), (stage, len(records))
    S = {}
    for name, (p, bound, out) in zip(names, records):
        assert out.grad is not None and out.dtype == torch.float64, name
        leaf = torch.zeros(sc["grids"][name].shape, dtype=torch.float64, requires_grad=True)
        cot = out.grad.abs().max(dim=1, keepdim=True)[0].expand_as(out)
        orig(leaf, p.detach(), bound, torch.float64).backward(cot)
        S["d_" + name] = leaf.grad.numpy()
    for k in FORWARD:
        S[k] = np.abs(_np(truth[k]))
    p = records[0][0]
    n = sc["rays_o"].shape[0]
    dp = p.grad.abs().reshape(n, -1, 3)
    o, d = sc["rays_o"].double(), sc["rays_d"].double()
    z = (p.detach().reshape(n, -1, 3) - o[:, None, :]).norm(dim=-1) / d.norm(dim=-1)[:, None]
    S["d_rays_o"] = dp.sum(1).numpy()
    S["d_rays_d"] = (z[:, :, None] * dp).sum(1).numpy()
    for k in gated(truth):
        assert S[k].shape == tuple(truth[k].shape), (k, S[k].shape, tuple(truth[k].shape))
    return truth, S


def local_err(x, truth, S, phi=PHI):
    """max |x - truth| / (S + phi * max S) over the elements -> (value, index of the worst element).  A tensor whose scale is zero
    everywhere must be exactly zero: 0.0 if it is, inf at its largest element if not."""
    x, truth, S = _np(x), _np(truth), np.asarray(S, dtype=np.float64)
    assert x.shape == truth.shape == S.shape, (x.shape, truth.shape, S.shape)
    top = float(S.max()) if S.size else 0.0
    if top == 0.0:
        i = np.unravel_index(int(np.argmax(np.abs(x))), x.shape)
        return (0.0 if float(np.abs(x[i])) == 0.0 else float("inf")), tuple(int(v) for v in i)
    q = np.abs(x - truth) / (S + phi * top)
    i = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[i]), tuple(int(v) for v in i)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
LCase = collections.namedtuple("LCase", "name case zero_frac origin_u edge")

# Seeds are chosen on the CPU so that the reference alone meets the conditions of tests/test_local_gate.py (its noise does not swallow
# a planted fault, 1 % of the touched elements lie in the low-mass band).  A case that stops meeting them is given another seed HERE.
SEED_OF = {"stage-coarse": 9064, "stage-middle": 9169, "stage-fine": 9265, "stage-color": 9335, "nodepth": 9438, "s1": 9524, "s64": 9625, "s25": 9726,
           "hot": 9999, "cap1-fine": 9843, "cap1-color": 9829, "pastbound": 9753, "halfzero": 9919, "short": 9993}

# S = 1: the one sample of a ray sits 0.01 * gt_depth in front of the camera, every point in the cell that holds the camera.  At the
# bound's centre that is a voxel of the fine grid and the middle of a cell of the middle grid: no low-mass voxel.  The rays' origin is
# put at these coordinates of the `small` scene's fine grid (9 x 9 x 7 voxels, in cells, x y z) instead: 0.03 of a cell from a fine voxel on
# every axis, and, the middle grid having 4 x 4 x 3 voxels over the same box, at 1.864, 1.864 and 1.01 of the middle grid: corner
# weights from 0.9 down to 3e-5 in the fine and colour grids, down to 2e-4 in the middle one.
S1_ORIGIN = (4.97, 4.97, 3.03)


def _l(label, case, zero_frac=0.02, origin_u=None, edge=None):
    return LCase(label, case, zero_frac, origin_u, edge)


def _seed(label):
    return SEED_OF[label]


def _build():
    ext = 1.28                                              # the `small` scene's shortest bound edge (make_scene's depth unit)
    cases = [
        # one per stage: all gradients, default cap, 32 + 16 samples
        _l("stage-coarse", gc._case("local", 64, "coarse", 0, _seed("stage-coarse"))),
        _l("stage-middle", gc._case("local", 64, "middle", 0, _seed("stage-middle"))),
        _l("stage-fine", gc._case("local", 64, "fine", 0, _seed("stage-fine"))),
        _l("stage-color", gc._case("local", 32, "color", 0, _seed("stage-color"))),
        # uniform samples only: the longest dead tails behind the surface
        _l("nodepth", gc._case("local", 32, "color", 0, _seed("nodepth"), with_depth=False)),
        # S = 1: a tile holds sixteen rays; S = 64: four whole tiles a ray (sample counts of geometry_cases' `samples` group)
        _l("s1", gc._case("local", 17, "color", 0, _seed("s1"), samples=(1, 0)), origin_u=S1_ORIGIN),
        _l("s64", gc._case("local", 23, "color", 0, _seed("s64"), samples=(40, 24))),
        # S = 25: a 16-sample tile straddles two rays, the gradients of its rows go to different rays
        _l("s25", gc._case("local", 23, "color", 0, _seed("s25"), samples=(20, 5))),
        # the hot-voxel table with more candidates than slots, one block per pass.  Not geometry_cases' `hot` case: at Replica coordinates
        # the reference's fp32 sines put rho_ref at 1.4e-4 .. 1.7e-3 on every tensor, which swallows a 1e-3 fault; scene `hot_wide` has the
        # same overflow (tests/test_local_gate.py checks it like test_geometry_cases.py does) at coordinates below 1 m
        _l("hot", gc._case("local", 64, "color", 3, _seed("hot"), scene="hot_wide", depth_range=(0.15, 0.40), hot_voxels=gc.HOT_SLOT_CAP + 1, nb=1)),
        # a coarse gradient grid that cannot sit in LDS: global atomics
        _l("coarselds", gc.BY_NAME["coarselds-coarse-n64-s32+16-cap0-coarse_dense"]),
        # cap 1: one block per pass walks every tile (43 rays = 129 tiles, the 64-tile live-mask chunk crossed twice)
        _l("cap1-fine", gc._case("local", 43, "fine", 1, _seed("cap1-fine"))),
        _l("cap1-color", gc._case("local", 22, "color", 1, _seed("cap1-color"))),
        # depths up to 1.5 x the shortest bound edge from a camera at the centre: surface samples leave the box, take the border clamp
        # (their colour gradient lands on the boundary planes), and the uniform samples run to the box's far side
        _l("pastbound", gc._case("local", 32, "color", 0, _seed("pastbound"), depth_range=(0.3 * ext, 1.5 * ext)), edge="pastbound"),
        # half the rays without a depth measurement: their surface samples spread over [0.001, max gt_depth]
        _l("halfzero", gc._case("local", 64, "color", 0, _seed("halfzero")), zero_frac=0.5, edge="halfzero"),
        # short rays: depth, var and rgb where the batch maximum says little
        _l("short", gc._case("local", 32, "color", 0, _seed("short"), depth_range=(0.02 * ext, 0.05 * ext))),
    ]
    assert len(cases) <= 16 and len({c.name for c in cases}) == len(cases)
    assert all(c.case.n_rays <= 300 for c in cases)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
EDGE_SCENES = tuple(c.name for c in CASES if c.edge)


def case_scene(lc):
    c = lc.case
    assert not c.edge
    sc = su.make_scene(seed=c.seed, n_rays=c.n_rays, scene=c.scene, fine_scale=c.fine_scale, depth_range=c.depth_range, zero_frac=lc.zero_frac)
    if lc.origin_u is not None:
        Z, Y, X = sc["grids"]["grid_fine"].shape[2:]
        b = sc["bound"]
        cell = (b[:, 1] - b[:, 0]) / torch.tensor([X - 1, Y - 1, Z - 1], dtype=torch.float64)
        sc["rays_o"] = (b[:, 0] + torch.tensor(lc.origin_u, dtype=torch.float64) * cell).float().expand_as(sc["rays_o"]).contiguous()
    return sc


def samples_of(lc):
    return dict(n_samples=lc.case.samples[0], n_surface=lc.case.samples[1])


def case_truth(lc, sc):
    return truth_and_scales(sc, lc.case.stage, lc.case.with_depth, **samples_of(lc))


def case_oracle(lc, sc):
    return gc.case_oracle(lc.case, sc)


def reference_noise(lc, sc=None, truth=None, S=None, ref=None):
    """rho_ref per gated tensor: the largest ``local_err`` over the fp32 oracle and N_DRAWS one-ulp-perturbed draws of it."""
    sc = sc or case_scene(lc)
    if truth is None:
        truth, S = case_truth(lc, sc)
    draws = [ref or case_oracle(lc, sc)] + [gc.case_oracle(lc.case, su.ulp_perturbed(sc, 1234 + i)) for i in range(N_DRAWS)]
    return {k: max(local_err(d[k], truth[k], S[k])[0] for d in draws) for k in gated(truth)}


# ---- planted faults: what the gate must see ----------------------------------------------------------------------------------------
POWER = 10.0                    # a planted fault must stand this far above the gate MARGIN * rho_ref
FAULT = 1e-3                    # relative size of the multiplicative faults
BAND_MIN = 0.01                 # at least this share of a grid gradient's touched elements lies in the low-mass band


def band_mask(S):
    """the low-mass voxels of a grid gradient: PHI * max s < s_v < BAND_HI * max s"""
    return (S > PHI * S.max()) & (S < BAND_HI * S.max())


def plane_mask(S):
    """the voxels on the six boundary planes of a [1,C,Z,Y,X] grid that carry mass: s_v > PHI * max s"""
    m = np.zeros(S.shape, dtype=bool)
    m[:, :, 0] = m[:, :, -1] = m[:, :, :, 0] = m[:, :, :, -1] = m[..., 0] = m[..., -1] = True
    return m & (S > PHI * S.max())


def planted(k, x, truth, S):
    """Faulty copies of the fp32 oracle's tensor ``x`` -> {fault name: array}.  A grid gradient: (a) the band zeroed, (b) the band times
    1 + FAULT, (c) the boundary planes zeroed (left out where no boundary voxel carries mass).  A forward output: 1 + FAULT on the
    shortest tenth of the rays; a ray gradient: 1 + FAULT on the tenth of its elements with the lowest scale."""
    x = _np(x)
    out = collections.OrderedDict()
    if is_grid(k):
        band, planes = band_mask(S[k]), plane_mask(S[k])
        out["a"] = np.where(band, 0.0, x)
        out["b"] = np.where(band, x * (1.0 + FAULT), x)
        if planes.any():
            out["c"] = np.where(planes, 0.0, x)
        return out
    m = np.zeros(x.shape, dtype=bool)
    if k in FORWARD:
        m[np.argsort(_np(truth["depth"]), kind="stable")[:max(1, x.shape[0] // 10)]] = True
    else:
        flat = np.argsort(S[k].reshape(-1), kind="stable")[:max(1, S[k].size // 10)]
        m.reshape(-1)[flat] = True
    out["short" if k in FORWARD else "lowscale"] = np.where(m, x * (1.0 + FAULT), x)
    return out


def conditions(lc, sc, truth, S, ref, rho):
    """What a case must meet on the reference alone to be worth running -> list of (tensor, what is wrong); empty: the case stands."""
    bad = []
    for k in gated(truth):
        if float(S[k].max()) == 0.0:                        # rgb below the colour stage: exactly zero, nothing to plant
            if not (k == "rgb" and lc.case.stage != "color"):
                bad.append((k, "no scale at all"))
            continue
        need = POWER * MARGIN * rho[k]
        if is_grid(k):
            touched = int((S[k] > 0).sum())
            band = int(band_mask(S[k]).sum())
            if band < BAND_MIN * touched or band == 0:
                bad.append((k, "band holds %d of %d touched elements" % (band, touched)))
            if not (np.abs(_np(truth[k])) <= S[k] * (1.0 + 1e-12)).all():
                bad.append((k, "|truth| exceeds its scale"))
        faults = planted(k, ref[k], truth, S)
        if is_grid(k) and lc.edge and "c" not in faults:
            bad.append((k, "no boundary voxel carries mass in an edge scene"))
        for f, y in faults.items():
            e = local_err(y, truth[k], S[k])[0]
            if not e >= need:
                bad.append((k, "fault (%s) gives %.2e, below %g x rho_ref = %.2e" % (f, e, POWER * MARGIN, need)))
    return bad


def committed():
    return json.load(open(NOISE_FILE))


def committed_noise(name):
    return committed()["cases"][name]


def margin(name, tensor):
    """MARGIN, or the per-tensor margin of the `allowed` list of the committed file (a tensor named there with its measured ratio)."""
    for e in committed().get("allowed", []):
        if e["case"] == name and e["tensor"] == tensor:
            return float(e["margin"])
    return MARGIN


def write_noise(table):
    old = committed() if os.path.exists(NOISE_FILE) else {}
    doc = collections.OrderedDict()
    doc["_comment"] = ("per case of tests/local_gate.py and per gated tensor: rho_ref, the largest local_err = max|x - truth| / (S + 1e-5 max S) "
                       "of the fp32 oracle and three one-ulp-perturbed draws against the fp64 oracle.  A fresh measurement must lie within "
                       "a factor of 2 (tests/test_local_gate.py); the GPU product is held to twice these values (tests/test_hip_local_parity.py).  "
                       "Rewritten by `python tests/local_gate.py`.  `allowed`: tensors BY NAME whose rho_got / rho_ref on the MI355X is above 2 for a stated fp32 "
                       "reason; they take `margin` (at most twice `measured_ratio`) instead of 2.")
    doc["cases"] = table
    doc["allowed"] = old.get("allowed", [])
    json.dump(doc, open(NOISE_FILE, "w"), indent=1)


def measure_all(verbose=True):
    table = collections.OrderedDict()
    for lc in CASES:
        rho = reference_noise(lc)
        table[lc.name] = collections.OrderedDict((k, float("%.3e" % v)) for k, v in rho.items())
        if verbose:
            print("%-14s %s" % (lc.name, "  ".join("%s %.1e" % (k, v) for k, v in rho.items())))
    return table


if __name__ == "__main__":
    write_noise(measure_all())
