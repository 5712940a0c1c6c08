"""GPU: the split backward (fwd_sample -> render_fwd_pass -> fwd_composite, then comp_bwd -> dX -> dW -> finalize) held to the
CPU oracle at every launch geometry of tests/geometry_cases.py -- 1 to 12 waves per dX block, one / two / many blocks per decoder
pass (``Renderer.bwd_max_blocks``), tile sequences across the 64-tile live-mask chunks, S = 1, 2, 16, 25, 33, 64, every gradient
subset, a hot-voxel table with more candidates than slots, a coarse gradient grid that does not fit in LDS -- through the public
path: ``Renderer`` from a cfg, ``renderer.bwd_max_blocks``, ``requires_grad`` on grids, decoders and rays.

Gate: max|a-b| / max|b| <= 1e-4 against the fp32 oracle for every forward output and gradient (``parity_failures``; only the
`everywhere` tensors of tests/golden/secondary_gate.json may take the secondary gate: the case seeds are chosen so that the
reference's own fp32 noise is below half the gate, tests/test_geometry_cases.py).

201 tests: 128 cases, 47 cap families, 26 cap-1 cases.  On the MI355X the file takes 4.0 s (the slowest test 0.34 s) and no tensor
takes the secondary gate; the largest rel_err per group against the fp32 oracle (any tensor / forward outputs; run with -s):
waves 5.7e-5 / 6.2e-6, oneblock 2.5e-5 / 1.6e-5, twoblocks 1.9e-5 / 2.9e-6, samples 7.0e-5 / 1.4e-5, subsets 2.7e-5 / 6.1e-6,
hot 6.7e-6 / 5.7e-6, coarselds 1.2e-6 / 3.0e-7, edge 4.3e-6 / 2.7e-6 -- each time on a decoder-parameter gradient; between caps at
most 4.1e-6, between two backward runs at cap 1 at most 8.6e-7.
"""
import pytest
import torch

import geometry_cases as gc
from scene_util import PRIMARY_ONLY, build_product, hip_render, parity_failures, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
REORDER_TOL = 1e-5          # the same sums in another order (test_hip_parity.py::test_forward_kernels_agree_and_oversized_batches_are_chunked)
DEV = "cuda:0"

_REFS, _PRODUCTS, _GOT = {}, {}, {}


def _reference(case):
    """(scene, fp32 oracle result) of a case: computed once, shared by the cases on the same rays, never modified"""
    k = gc.ref_key(case)
    if k not in _REFS:
        sc = gc.case_scene(case)
        _REFS[k] = (sc, gc.case_oracle(case, sc))
    return _REFS[k]


def _product(case, sc):
    """Renderer / decoders / grids, built once per (scene, sample counts)"""
    k = (case.scene, case.seed, case.fine_scale, case.samples)
    if k not in _PRODUCTS:
        _PRODUCTS[k] = build_product(sc, DEV, n_samples=case.samples[0], n_surface=case.samples[1])
    return _PRODUCTS[k]


def _render(case, twice=False):
    sc, _ = _reference(case)
    prod = _product(case, sc)
    prod[0].bwd_max_blocks = case.cap
    try:
        return hip_render(sc, case.stage, device=DEV, backward=True, with_depth=case.with_depth, product=prod, want=case.want, twice=twice)
    finally:
        prod[0].bwd_max_blocks = 0


def _got(case):
    if case.name not in _GOT:
        _GOT[case.name] = _render(case)
    return _GOT[case.name]


def _is_ray_grad(k):
    return k in ("d_rays_o", "d_rays_d")


@pytest.mark.parametrize("name", [c.name for c in gc.CASES])
def test_case_against_the_oracle(name):
    c = gc.BY_NAME[name]
    sc, ref = _reference(c)
    got = _got(c)
    keys = gc.wanted_keys(c, ref)
    assert set(keys) <= set(got), (name, sorted(set(keys) - set(got)))
    errs = {k: rel_err(got[k], ref[k]) for k in keys}
    worst = max(errs, key=errs.get)
    print("geo/%s [%s] %s: max rel_err %.2e (%s), forward %.2e" % (name, c.group, gc.case_geo(c), errs[worst], worst,
                                                                   max(errs[k] for k in PRIMARY_ONLY)))
    for k in PRIMARY_ONLY:
        assert errs[k] < TOL, (name, k, errs[k])
    bad = parity_failures(got, sc, c.stage, tol=TOL, with_depth=c.with_depth, ref={k: ref[k] for k in keys}, tag="geo/" + name,
                          n_samples=c.samples[0], n_surface=c.samples[1])
    assert not bad, (name, bad)
    for k in set(got) - set(keys):
        # outside the subset the product returns nothing (hip_render keeps only the gradients that are not None) ...
        group = "rays" if _is_ray_grad(k) else ("grids" if k.startswith("d_grid") else "params")
        assert group in c.want, (name, k, "a gradient outside the requested subset")
        # ... and what it returns beyond the oracle's gradients is exactly zero
        assert k not in ref and float(got[k].abs().max()) == 0.0, (name, k)


def _reordered(k):
    """Gradients whose sum has no fixed order, whatever the cap.  Grid gradients are float atomics from every block.  So are the RAY
    gradients, other than one might expect of a per-ray sum: the dX kernel adds a ray's share with `atomic_add_global` once per
    16-sample tile (per sample where a tile straddles rays) and once per decoder pass (nsr_bwd2.h, the RAYS branch); the passes are
    different blocks that run side by side, and the waves of a block draw their tiles from a counter in LDS, so which share arrives
    first differs from launch to launch -- also with one block per pass.  The embedding-matrix gradient `embedder._B` is summed per
    wave over the tiles that wave happened to draw, then over the waves: again arrival order.  These are held to REORDER_TOL; the
    weight and bias gradients, one partial image per dW block summed in a fixed order, are held bit for bit where the test says so."""
    return k.startswith("d_grid") or _is_ray_grad(k) or k.endswith("embedder._B")


@pytest.mark.parametrize("name", [first.name for first, _ in gc.cap_families()])
def test_same_result_at_every_cap(name):
    """Cases that differ only in the persistent-grid cap: the forward does not depend on it (bit for bit); every gradient is the same
    sum in another order -- atomics (``_reordered``; the ray gradients among them, which is why they are not compared bit for bit)
    or another number of partial images of the dW kernel -- and agrees to REORDER_TOL."""
    first, others = next(f for f in gc.cap_families() if f[0].name == name)
    a = _got(first)
    for o in others:
        b = _got(o)
        assert set(a) == set(b), (name, o.name)
        errs = {k: rel_err(b[k], a[k]) for k in a}
        worst = max(errs, key=errs.get)
        print("caps/%s vs cap %d [%s]: max %.2e (%s), ray gradients %.2e" % (name, o.cap, first.group, errs[worst], worst,
                                                                             max([errs[k] for k in a if _is_ray_grad(k)] or [0.0])))
        for k in a:
            if k in PRIMARY_ONLY:
                assert torch.equal(a[k], b[k]), (name, o.name, k, errs[k])
            else:
                assert errs[k] < REORDER_TOL, (name, o.name, k, errs[k])


@pytest.mark.parametrize("name", [c.name for c in gc.CASES if c.cap == 1 and c.want == gc.ALL])
def test_cap_one_is_reproducible(name):
    """One block per pass, the backward run twice over the same saved forward: one partial image of the dW kernel per pass, one order
    of its sums -- the weight and bias gradients of the two runs agree bit for bit.  The gradients summed in arrival order
    (``_reordered``: the ray gradients and `embedder._B` among them) agree to REORDER_TOL."""
    c = gc.BY_NAME[name]
    a, b = _render(c, twice=True)
    assert set(a) == set(b)
    errs = {k: rel_err(b[k], a[k]) for k in a}
    print("twice/%s [%s]: %s" % (name, c.group, ", ".join("%s %.2e" % (k, e) for k, e in sorted(errs.items()) if e > 0.0) or "all bit for bit"))
    for k in a:
        if _reordered(k):
            assert errs[k] < REORDER_TOL, (name, k, errs[k])
        else:
            assert torch.equal(a[k], b[k]), (name, k, errs[k])
