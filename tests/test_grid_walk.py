"""Which cells the grid walk visits (nsr_recon.h: nn_walk, shared by the point search and the mesh-distance search), pinned by
the number of candidates every query examines.  The brute-force checks of test_recon_emu.py / test_meshdist_emu.py hold the
answers bit for bit, but a walk that prunes less stays correct and only gets slower, and one that prunes more is wrong only for
rare queries: so ``ncand`` of every case of both modules must equal tests/golden/grid_walk_counts.npz, recorded from the commit
BEFORE the two walks became one (tests/golden/make_golden_grid_walk.py), on the emulator and on the device.  The same file
holds that commit's workspace byte counts for three plans."""
import os

import numpy as np
import pytest

import emu_harness
import test_meshdist_emu as TM
import test_recon_emu as TN
from nice_slam_amd import recon
from nice_slam_amd.engine import Engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_walk_counts.npz")
NN_CASES, MESH_CASES = TN.cases(), TM.CASES
BYTE_PLANS = ("one_cell", "plane", "far")                          # of NN_CASES: one cell, a planar set, 2000 points


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def emu():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def dev():
    from nice_slam_amd.engine import on
    return on("cuda:0")


def nn_counts(E, name):
    """through check_nn: the counts belong to answers that are right"""
    return TN.check_nn(E, *NN_CASES[name]).astype(np.int32)


def mesh_counts(E, name):
    return TM.check_mesh(E, *MESH_CASES[name])[2].astype(np.int32)


def workspace_bytes(E, name):
    """(nsr_nn_workspace_bytes, nsr_meshdist_workspace_bytes) for the plan of NN case ``name``; the mesh entry takes the same
    plan as one for M faces, with pair and oversize counts that are no multiple of the tables' alignment"""
    idx = recon.NNIndex(NN_CASES[name][1], E)
    return np.array([E.lib.nsr_nn_workspace_bytes(idx.plan, idx.m),
                     E.lib.nsr_meshdist_workspace_bytes(idx.plan, idx.m, 5 * idx.m + 3, 7)], np.int64)


@pytest.mark.parametrize("name", list(NN_CASES))
def test_nn_counts_emu(emu, gold, name):
    assert np.array_equal(nn_counts(emu, name), gold["nn/" + name])


@pytest.mark.parametrize("name", list(MESH_CASES))
def test_mesh_counts_emu(emu, gold, name):
    assert np.array_equal(mesh_counts(emu, name), gold["mesh/" + name])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NN_CASES))
def test_nn_counts_device(dev, gold, name):
    assert np.array_equal(nn_counts(dev, name), gold.get("device/nn/" + name, gold["nn/" + name]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MESH_CASES))
def test_mesh_counts_device(dev, gold, name):
    q, v, f = MESH_CASES[name]
    assert len(f) <= 2000 and len(q) <= 600
    assert np.array_equal(mesh_counts(dev, name), gold.get("device/mesh/" + name, gold["mesh/" + name]))


def cells_of(plan, x):
    """the clamped fine cell of every point, as nn_cell"""
    lo, h, nd = np.array(plan[0:3]), plan[6], np.array(plan[7:10])
    return np.clip(np.floor((np.asarray(x, np.float64) - lo) / h), 0, nd - 1).astype(np.int64)


def check_ragged_plan(plan):
    nd, nc = np.array(plan[7:10]), np.array(plan[10:13])
    assert nc.prod() >= 2                                           # more than one coarse cell
    assert (nd % 8 != 0).any()                                      # ... the last of which, along some axis, is not full


def test_coarse_route_over_ragged_grid(emu):
    """queries that the shell walk leaves open go through the coarse cells of a grid whose last coarse cells are partial: they
    still prune (fewer candidates than a scan of everything); the cases' answers are held to brute force by check_nn and
    check_mesh in their own modules, and their counts to the parent's above"""
    q, ref = NN_CASES["far_ragged"]
    idx = recon.NNIndex(ref, emu)
    check_ragged_plan(idx.plan)
    d, i, nc = idx.query(q, with_candidates=True)
    # the answer's cell is beyond the three shells around the query's cell: only the coarse route finds it
    assert (np.abs(cells_of(idx.plan, ref[i.numpy()[:TN.INSIDE]]) - cells_of(idx.plan, q[:TN.INSIDE])).max(1) > 2).all()
    assert (nc.numpy()[:TN.FAR_RAGGED] < len(ref)).all() and (nc.numpy()[:TN.FAR_RAGGED] >= 1).all()
    q, v, f = MESH_CASES["far_ragged"]
    midx = recon.MeshIndex(v, f, emu)
    check_ragged_plan(midx.plan)
    d, fi, x, nc = midx.query(q, with_candidates=True)
    assert (np.abs(cells_of(midx.plan, x.numpy()[:TM.INSIDE]) - cells_of(midx.plan, q[:TM.INSIDE])).max(1) > 2).all()
    # faces are counted once per cell they are examined in: a route that does not prune examines the whole pair table
    assert (nc.numpy()[:TM.FAR_RAGGED] < midx.npairs).all() and (nc.numpy()[:TM.FAR_RAGGED] >= 1).all()


@pytest.mark.parametrize("name", BYTE_PLANS)
def test_workspace_bytes_as_parent(emu, gold, name):
    assert np.array_equal(workspace_bytes(emu, name), gold["bytes/" + name])
