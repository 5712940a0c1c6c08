"""Mint tests/golden/workspace_sizes.json: what every size entry of the library returns for the cases of
tests/test_workspace_sizes.py::collect.

The file is a record of commit 2757677 ("One cell-grid walk for the point search and the mesh-distance search"), the last one
in which every workspace was described twice -- once by the entry that reports its size, once by the code that places typed
pointers in it: it was written with that commit's nice_slam_amd/csrc and include/ checked out under these tests, on the CPU
emulator.  Minting it again from a later commit would compare the one description with itself; do that only to add cases, and
say from which commit.

The emulator is rebuilt by force first: emu_harness.build_emu judges a built library stale by the modification times of some
of the headers only, and a checkout of another commit's sources does not reliably move them.

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=tests python tests/golden/make_golden_workspace_sizes.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_workspace_sizes as T  # noqa: E402

MINTED_FROM = "2757677"

if __name__ == "__main__":
    import emu_harness
    from nice_slam_amd import _capi
    sizes = T.collect(_capi.Lib(emu_harness.build_emu(force=True)))
    with open(os.path.join(HERE, "workspace_sizes.json"), "w") as f:
        json.dump({"minted_from": MINTED_FROM, "sizes": sizes}, f, indent=1)
        f.write("\n")
    print("wrote workspace_sizes.json:", len(sizes), "cases")
