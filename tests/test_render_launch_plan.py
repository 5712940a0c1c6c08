"""Every launch of the render entries -- nsr_render_fwd, nsr_render_bwd, nsr_eval_points_fwd, nsr_pack_params -- held to
tests/golden/render_launch_plan.json: kernel, grid, block, LDS bytes and the plan fields the host writes into RenderParams
(block ranges of the decoder passes, hot-table size, activation-buffer offsets, ...) and into the finalize jobs.

The golden is a record of the commit BEFORE the host code of these entries was restated (one stage description, one block deal,
one stage dispatch, one layout of `acts`); tests/golden/make_golden_render_launch_plan.py mints it through ``collect``.  The
emulator's launch log (tests/emu/nsr_dev.h: nsr_emu_launch_log) records every launch; in its dry mode the kernels do not run, the
host code reads no device memory, and so every pointer argument here is one small dummy buffer and large batches are free.

A kernel is named by the symbol at its address, so the record does not depend on how the host code spells the launch."""
import ctypes as C
import json
import os

import pytest

import emu_harness
import geometry_cases as gc
import scene_util as su
from nice_slam_amd import _capi
from nice_slam_amd.layout import stage_slots
from oracle import nice_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_launch_plan.json")
STAGES = ("coarse", "middle", "fine", "color")
# a launch is ["kernel", grid x, grid y, block x, LDS bytes] + [PLAN] for a RenderParams, + [[JOB] * 3] for the finalize jobs
PLAN = (["rays_per_block", "tiles_per_block", "n_groups", "act_tiles", "partial_stride"] + ["pass_beg[%d]" % i for i in range(4)] +
        ["dx_beg[%d]" % i for i in range(4)] + ["dw_beg[%d]" % i for i in range(4)] + ["hot_slots"] + ["hot_z[%d] bits" % i for i in range(4)] +
        ["lds_grid_floats", "draw_scaled", "skip_masked", "s_magic", "dy - acts", "draw - acts", "pf - acts", "pd - acts", "dbpart - partials"])
JOB = ["kind", "nimg", "ndx", "images - workspace", "dbpart - workspace"]
VARIANTS = {"fwd_full_blocks": "-DNSR_TEST_FWD_SMALL=0", "hot_0_dflt": "-DNSR_TEST_HOT_CELLS=0",
            "hot_64_16": "-DNSR_TEST_HOT_CELLS=64 -DNSR_TEST_HOT_SLOTS=16"}

_DUMMY = (C.c_char * 4096)()
PTR = C.addressof(_DUMMY)


def scene_grids(scene, coarse_shape=None):
    """{slot: ((Z, Y, X), lo, hi)} of a scene of scene_util.SCENES, as scene_util.make_scene and emu_harness.HostScene place them"""
    bound_cfg, grid_len, _ = su.SCENES[scene]
    bound = orc.scene_bound(bound_cfg, 1.0, 0.32)
    shapes = orc.grid_shapes(bound, grid_len, 2.0)
    out = {}
    for s in STAGES:
        b = bound.numpy() * (2.0 if s == "coarse" else 1.0)
        out[s] = (shapes["grid_" + s], b[:, 0].tolist(), b[:, 1].tolist())
    if coarse_shape is not None:
        out["coarse"] = (coarse_shape,) + out["coarse"][1:]
    return out


def render_args(stage, n_rays, samples, with_depth, grids, acts=True, fused=False):
    a = _capi.NsrRenderArgs()
    a.stage, a.n_rays = _capi.STAGE_ID[stage], n_rays
    a.n_samples, a.n_surface = samples
    a.rays_o = a.rays_d = a.depth = a.var = a.rgb = a.raw = a.zvals = PTR
    if with_depth:
        a.gt_depth = a.gt_max = PTR
    if acts:
        a.acts = PTR
    if fused:
        a.gt_color = a.loss = a.dl_depth = a.dl_rgb = a.keep = PTR         # the mapper's fused loss, masked rays out of the batch
        a.skip_masked = 1
    for i in range(3):
        a.bound_lo[i], a.bound_hi[i] = grids["middle"][1][i], grids["middle"][2][i]
    for s in stage_slots(stage):
        i = _capi.SLOT_NAMES.index(s)
        (a.grid[i].Z, a.grid[i].Y, a.grid[i].X), lo, hi = grids[s]
        a.grid[i].feat = a.dec[i].params = a.dec[i].packed = PTR
        for d in range(3):
            a.grid[i].lo[d], a.grid[i].hi[d] = lo[d], hi[d]
    return a


class Recorder:
    def __init__(self, lib):
        self.lib = lib
        self.log = lib.cdll.nsr_emu_launch_log
        self.log.restype, self.log.argtypes = C.c_char_p, [C.c_int]

    def start(self):
        self.log(2)

    def stop(self):
        return json.loads(self.log(0).decode())

    def fwd_bwd(self, stage, n_rays, samples=(32, 16), with_depth=True, cap=0, want=gc.ALL, scene="small", coarse_shape=None,
                from_forward=False, dparams=None):
        """the saving forward, then the backward; ``dparams``: the slots whose decoders want parameter gradients (default: all,
        if ``want`` has "params")"""
        lib, grids = self.lib, scene_grids(scene, coarse_shape)
        guided = with_depth and stage != "coarse"
        S = samples[0] + (samples[1] if guided else 0)
        a = render_args(stage, n_rays, samples, with_depth, grids, fused=from_forward)
        self.start()
        lib.check(lib.nsr_render_fwd(C.byref(a), None), "fwd")
        b = _capi.NsrBwdArgs()
        b.d_depth = b.depth = PTR
        if from_forward:
            b.loss_grads_from_forward = 1
            b.d_rgb = PTR if stage == "color" else None
        else:
            b.d_var = b.d_rgb = PTR
        if "rays" in want:
            b.d_rays_o = b.d_rays_d = PTR
        for s in stage_slots(stage):
            i = _capi.SLOT_NAMES.index(s)
            if "grids" in want:
                a.grid[i].dfeat = PTR
            if "params" in want and (dparams is None or s in dparams):
                a.dec[i].dparams = PTR
        b.workspace, b.max_blocks = PTR, cap
        b.workspace_floats = lib.nsr_bwd_workspace_floats(a.stage, n_rays, S, cap)
        lib.check(lib.nsr_render_bwd(C.byref(a), C.byref(b), None), "bwd")
        return self.stop()

    def fwd(self, stage, n_rays, S, acts):
        a = render_args(stage, n_rays, (S, 0), False, scene_grids("small"), acts=acts)
        self.start()
        self.lib.check(self.lib.nsr_render_fwd(C.byref(a), None), "fwd")
        return self.stop()

    def eval_points(self, stage, n_points):
        a = render_args(stage, 0, (32, 16), False, scene_grids("small"), acts=False)
        self.start()
        self.lib.check(self.lib.nsr_eval_points_fwd(C.byref(a), PTR, n_points, PTR, None), "eval_points")
        return self.stop()

    def pack(self, slot):
        self.start()
        self.lib.check(self.lib.nsr_pack_params(slot, PTR, PTR, None), "pack")
        return self.stop()


def geometry_case(rec, c):
    return rec.fwd_bwd(c.stage, c.n_rays, c.samples, c.with_depth, c.cap, c.want, c.scene)


# the cases that are also run against the variant builds of tests/test_emu_parity.py (other launch-policy constants)
VARIANT_GEOMETRY = ("hot-color-n300-s32+16-cap3-replica_room0", "subsets-fine-n37-s32+16-cap0-grids", "waves-color-n341-s32+16-cap0",
                    "oneblock-coarse-n43-s32+16-cap1")


def collect(lib, variant=False):
    """{"case": [launch, ...]}; a backward case's geometry (for the deal's bound) is ``backward_geo(name)``"""
    rec, out = Recorder(lib), {}
    for c in gc.CASES:
        if not variant or c.name in VARIANT_GEOMETRY:
            out["geometry/" + c.name] = geometry_case(rec, c)
    for stage in STAGES:
        if not variant:
            # the backward's flags at 37 rays: d raw from the forward (no comp_bwd launch), no parameter gradients (no dW, no finalize),
            # rays off, one decoder's parameters alone (zero dW weights for the others), a coarse gradient grid that does not fit in LDS
            out["flags/%s/from_forward" % stage] = rec.fwd_bwd(stage, 37, from_forward=True)
            out["flags/%s/given" % stage] = rec.fwd_bwd(stage, 37)
            out["flags/%s/no_params" % stage] = rec.fwd_bwd(stage, 37, want=("grids", "rays"))
            out["flags/%s/no_rays" % stage] = rec.fwd_bwd(stage, 37, want=("grids", "params"))
            for s in stage_slots(stage):
                out["flags/%s/params_of_%s" % (stage, s)] = rec.fwd_bwd(stage, 37, dparams=(s,))
                out["flags/%s/params_of_%s_alone" % (stage, s)] = rec.fwd_bwd(stage, 37, want=("params",), dparams=(s,))
            # the three-launch forward at the wave-count and clamp boundaries: S = 16, one tile per ray
            for tiles in (1, 255, 256, 257, 12 * 256, 12 * 256 + 1):
                out["fwd3/%s/tiles%d" % (stage, tiles)] = rec.fwd(stage, tiles, 16, True)
            for n in (1, 16, 193, 12 * 16 * 2048 + 1):
                out["eval_points/%s/n%d" % (stage, n)] = rec.eval_points(stage, n)
        # the one-launch forward across the regimes of the small-block rule
        for S, rays in ((48, (1, 200, 255, 256, 257, 3072, 100000)), (1, (1, 200, 3072, 100000)), (64, (1, 200, 3072, 100000))):
            for n in rays:
                if not variant or n in (200, 3072):
                    out["fwd1/%s/n%d-S%d" % (stage, n, S)] = rec.fwd(stage, n, S, False)
    if not variant:
        out["flags/coarse/grid_in_lds"] = rec.fwd_bwd("coarse", 37, coarse_shape=(8, 8, 20))                 # 1280 voxels = all of LDS: still out
        out["flags/coarse/grid_small"] = rec.fwd_bwd("coarse", 37, coarse_shape=(3, 4, 5))
        out["flags/coarse/grid_1281_voxels"] = rec.fwd_bwd("coarse", 37, coarse_shape=(3, 7, 61))
        for slot in range(4):
            out["pack/%d" % slot] = rec.pack(slot)
    return out


def backward_geo(name):
    """the ``expected_geo`` of a backward case of ``collect``, None for the others"""
    kind, _, rest = name.partition("/")
    if kind == "geometry":
        return gc.case_geo(gc.BY_NAME[rest])
    if kind == "flags":
        stage = rest.split("/")[0]
        return gc.expected_geo(stage, 37, 32 if stage == "coarse" else 48, 0)
    return None


def differences(got, gold):
    """["case, launch i: field: got != gold", ...]"""
    out = []
    if list(got) != list(gold):
        out.append("cases: %s" % sorted(set(got) ^ set(gold)))
    for name in gold:
        g, w = got.get(name, []), gold[name]
        if [l[0] for l in g] != [l[0] for l in w]:
            out.append("%s: kernels %s != %s" % (name, [l[0] for l in g], [l[0] for l in w]))
            continue
        for i, (lg, lw) in enumerate(zip(g, w)):
            if lg == lw:
                continue
            for f, x, y in zip(["kernel", "grid.x", "grid.y", "block.x", "lds"], lg, lw):
                if x != y:
                    out.append("%s, launch %d (%s): %s: %s != %s" % (name, i, lw[0], f, x, y))
            if lg[5:] != lw[5:]:
                names = PLAN if not isinstance(lw[5][0], list) else None
                if names:
                    out += ["%s, launch %d (%s): %s: %s != %s" % (name, i, lw[0], f, x, y) for f, x, y in zip(names, lg[5], lw[5]) if x != y]
                else:
                    out.append("%s, launch %d (%s): jobs %s != %s  (%s)" % (name, i, lw[0], lg[5], lw[5], JOB))
    return out


@pytest.fixture(scope="module")
def gold():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return collect(emu_harness.emu_lib())


def test_every_launch_as_parent(got, gold):
    assert gold["plan_fields"] == PLAN and gold["job_fields"] == JOB
    diff = differences(got, gold["cases"])
    assert not diff, "\n".join(diff[:40])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_launch_as_parent_variant_builds(gold, variant):
    lib = _capi.Lib(emu_harness.build_emu(variant=variant, defs=VARIANTS[variant]))
    diff = differences(collect(lib, variant=True), gold["variants"][variant])
    assert not diff, "\n".join(diff[:40])


def test_the_record_covers_what_it_is_there_for(gold):
    """kernels and regimes the cases are chosen to reach are in the record (a golden minted from too thin a table would pass the rest)"""
    cases = gold["cases"]
    kernels = {l[0] for launches in cases.values() for l in launches}
    for st in range(4):
        for k in ("render_fwd_kernel<%d>" % st, "render_fwd_pass_kernel<%d, true>" % st, "fwd_composite_kernel<%d>" % st, "eval_points_kernel<%d>" % st,
                  "render_bwd_dx_kernel<%d, true>" % st, "render_bwd_dx_kernel<%d, false>" % st, "render_bwd_dw_kernel<%d>" % st, "pack_kernel<%d>" % st):
            assert any(k + "(" in name for name in kernels), (k, sorted(kernels))
    assert any("comp_bwd_kernel" in k for k in kernels) and any("bwd_finalize_kernel" in k for k in kernels)
    names = lambda case: [l[0].split("(")[0].split("::")[-1].split("<")[0] for l in cases[case]]
    assert "comp_bwd_kernel" not in names("flags/color/from_forward") and "comp_bwd_kernel" in names("flags/color/given")
    assert names("flags/color/no_params")[-1] == "render_bwd_dx_kernel"
    lds_grid = PLAN.index("lds_grid_floats")
    dx = lambda case: [l for l in cases[case] if "render_bwd_dx_kernel" in l[0]][0]
    assert dx("flags/coarse/grid_small")[5][lds_grid] == 3 * 4 * 5 * gc.C_DIM and dx("flags/coarse/grid_1281_voxels")[5][lds_grid] == 0
    dw = [l for l in cases["flags/color/params_of_fine_alone"] if "render_bwd_dw_kernel" in l[0]][0][5]
    b = PLAN.index("dw_beg[0]")
    assert dw[b] == dw[b + 1] == 0 and dw[b + 2] > 0 and dw[b + 3] == dw[b + 2]           # zero weights for the other two decoders
    assert set(gold["variants"]) == set(VARIANTS)


def test_block_deals_stay_inside_the_workspace(got):
    """nsr_render_bwd refuses a dX deal beyond passes * nb blocks (the workspace's d _B partials) and a dW deal beyond passes * nimg
    (its partial images): with the present launch-policy constants neither happens, for every backward recorded here"""
    dx3, dw3, seen = PLAN.index("dx_beg[3]"), PLAN.index("dw_beg[3]"), 0
    for name, launches in got.items():
        geo = backward_geo(name)
        if geo is None:
            continue
        for l in launches:
            if "render_bwd_dx_kernel" in l[0] or "render_bwd_dw_kernel" in l[0]:
                assert l[5][dx3] <= geo["passes"] * geo["nb"], (name, l)
                assert l[5][dw3] <= geo["passes"] * geo["nimg"], (name, l)
                assert l[1] == (l[5][dx3] if "_dx_" in l[0] else l[5][dw3])
                seen += 1
    assert seen >= len(gc.CASES)


def test_a_wrong_expectation_fails(got, gold):
    """negative control: one block more in one dX range, one byte of LDS, one kernel swapped"""
    name = "geometry/" + gc.CASES[0].name
    for edit in ("plan", "lds", "kernel"):
        wrong = json.loads(json.dumps(gold["cases"]))
        i = [k for k, l in enumerate(wrong[name]) if "render_bwd_dx_kernel" in l[0]][0]
        if edit == "plan":
            wrong[name][i][5][PLAN.index("dx_beg[2]")] += 1
        elif edit == "lds":
            wrong[name][i][4] += 1
        else:
            wrong[name][i][0] = wrong[name][i][0].replace("true", "false")
        assert differences(got, wrong), edit
