"""Mint tests/golden/grid_walk_counts.npz: the candidates every query examines (``ncand`` of ``query(with_candidates=True)``)
for every case of tests/test_recon_emu.py::cases() and tests/test_meshdist_emu.py::CASES, and the workspace byte counts of
three plans, as tests/test_grid_walk.py computes them.

The file is a record of commit 201e767 ("Point-to-mesh distance on the GPU: exact recon metrics, F-score, normals"), the last
one in which nn_query_kernel and md_query_kernel each had a walk of their own: it was written with that commit's
nice_slam_amd/csrc checked out under these tests, on the CPU emulator.  Minting it again from a later commit would compare
the walk with itself; do that only to add cases, and say from which commit.

    keys   nn/<case>, mesh/<case>   int32 [N]   candidates per query, in query order
           bytes/<case>             int64 [2]   nsr_nn_workspace_bytes, nsr_meshdist_workspace_bytes (test_grid_walk.workspace_bytes)
           device/nn/<case>, ...                only where that commit's libnsr.so on an MI355X counted differently from its
                                                emulator (--device: an .npz of the same keys written on the device)

Every case was also run on an MI355X against that commit's libnsr.so; the counts equal the emulator's for all of them, so the
file holds no device/ key.

Usage:  PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=tests python tests/golden/make_golden_grid_walk.py [--device counts.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_grid_walk as T  # noqa: E402


def collect(E, byte_counts=True):
    out = {"nn/" + k: T.nn_counts(E, k) for k in T.NN_CASES}
    out.update({"mesh/" + k: T.mesh_counts(E, k) for k in T.MESH_CASES})
    if byte_counts:
        out.update({"bytes/" + k: T.workspace_bytes(E, k) for k in T.BYTE_PLANS})
    return out


if __name__ == "__main__":
    import emu_harness
    from nice_slam_amd.engine import Engine
    out = collect(Engine(emu_harness.emu_lib(), "cpu"))
    if "--device" in sys.argv:
        dev = np.load(sys.argv[sys.argv.index("--device") + 1])
        for k in dev.files:
            if not np.array_equal(dev[k], out[k]):
                out["device/" + k] = dev[k]
                print("device differs from the emulator:", k)
    np.savez_compressed(os.path.join(HERE, "grid_walk_counts.npz"), **out)
    print("wrote grid_walk_counts.npz:", len(out), "arrays,", sum(v.size for v in out.values()), "values")
