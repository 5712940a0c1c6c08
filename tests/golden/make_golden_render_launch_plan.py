"""Mint tests/golden/render_launch_plan.json: every launch of the render entries for the cases of
tests/test_render_launch_plan.py::collect, from the default emulator build and from the variant builds of the launch-policy hooks.

The file is a record of commit a1346fc ("One sample placement and one compositor for the render kernels"), the last one in which
the host code of nsr_render_fwd / nsr_render_bwd / nsr_eval_points_fwd spelled its block deals, stage dispatches and buffer
layouts several times each: it was written with that commit's nice_slam_amd/csrc and include/ checked out under these tests and
this commit's tests/emu (the launch log), on the CPU emulator.  Minting it again from a later commit would compare the one
statement with itself; do that only to add cases, and say from which commit.

The emulators are rebuilt by force first (see make_golden_workspace_sizes.py).

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=tests python tests/golden/make_golden_render_launch_plan.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_render_launch_plan as T  # noqa: E402

MINTED_FROM = "a1346fc"


def dump_cases(f, cases, indent):
    """one launch per line"""
    f.write("{\n")
    for i, (name, launches) in enumerate(cases.items()):
        f.write("%s%s: [%s]%s\n" % (indent, json.dumps(name), (",\n " + indent).join(json.dumps(l, separators=(",", ":")) for l in launches),
                                   "," if i + 1 < len(cases) else ""))
    f.write(indent[:-1] + "}")


if __name__ == "__main__":
    import emu_harness
    from nice_slam_amd import _capi
    cases = T.collect(_capi.Lib(emu_harness.build_emu(force=True)))
    variants = {v: T.collect(_capi.Lib(emu_harness.build_emu(force=True, variant=v, defs=d)), variant=True) for v, d in sorted(T.VARIANTS.items())}
    with open(T.GOLDEN, "w") as f:
        f.write('{"minted_from": %s,\n "plan_fields": %s,\n "job_fields": %s,\n "cases": ' % tuple(json.dumps(x) for x in (MINTED_FROM, T.PLAN, T.JOB)))
        dump_cases(f, cases, "  ")
        f.write(',\n "variants": {\n')
        for i, (v, c) in enumerate(variants.items()):
            f.write("  %s: " % json.dumps(v))
            dump_cases(f, c, "   ")
            f.write(",\n" if i + 1 < len(variants) else "\n")
        f.write(" }\n}\n")
    json.load(open(T.GOLDEN))
    print("wrote render_launch_plan.json:", len(cases), "cases,", sum(len(c) for c in cases.values()), "launches,", os.path.getsize(T.GOLDEN), "bytes")
