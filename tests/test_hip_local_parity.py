"""GPU: every voxel of the grid gradients and every ray of the forward outputs and ray gradients held to its OWN scale
(tests/local_gate.py), where the other parity files hold a tensor to its largest element.

Per case of ``local_gate.CASES`` the product runs through the public path (``build_product``, ``hip_render(..., backward=True)`` with
all gradients, ``renderer.bwd_max_blocks`` for the cap cases) and one fp64 oracle backward gives the truth and the scales.  For every
gated tensor: local_err = max |got - truth| / (S + 1e-5 max S) <= 2 * rho_ref, rho_ref the reference's own noise under the same
statistic as committed in tests/golden/local_gate_noise.json (a tensor on that file's `allowed` list takes the margin stated there);
and a grid element that no sample reaches (s = 0) is exactly zero.  Each test prints rho_got / rho_ref per tensor (run with -s).

On the MI355X (15 tests, 2.7 s) the largest rho_got / rho_ref per tensor class:
  forward outputs   2.03 (s64 depth, ray 16), then 1.95 (halfzero rgb), 1.90 (pastbound rgb)
  ray gradients     3.43 / 3.42 (s64 d_rays_o / d_rays_d, the same ray 16), 2.60 (s25 d_rays_d, one element), then 1.94
  grid gradients    5.82 (s64 d_grid_middle: the four voxels behind a nearly opaque sample), 2.00 (stage-middle d_grid_middle, one
                    element), then 1.81; d_grid_fine at most 1.80, d_grid_color 1.17, d_grid_coarse 1.00
The six tensors above 2 are on the `allowed` list of the committed file, each with its ratio and the fp32 argument; no kernel
fault was found behind them (the CPU emulator of the kernel sources gives the same ratios to two digits, and other legitimate
fp32 evaluations of the REFERENCE miss the same gate on the same elements).  No element with s = 0 was touched in any case.
"""
import numpy as np
import pytest

import local_gate as lg
from scene_util import build_product, hip_render

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _describe(name, k, got, truth, S, ref, i, gate):
    """the worst element, and how the miss is spread: how many elements stand above the gate, and the error of the high-mass ones"""
    top = float(S[k].max())
    q = np.abs(lg._np(got[k]) - lg._np(truth[k])) / (S[k] + lg.PHI * top) if top > 0 else np.abs(lg._np(got[k]))
    heavy = S[k] >= lg.BAND_HI * top
    return ("%s %s: worst element %s, s / max s = %.2e, got %.9g, fp32 oracle %.9g, truth %.9g; %d of %d elements with s > 0 above the gate, "
            "local_err over the elements with s >= %g max s: %.2e" %
            (name, k, i, S[k][i] / top if top > 0 else 0.0, lg._np(got[k])[i], lg._np(ref[k])[i], lg._np(truth[k])[i],
             int((q > gate).sum()), int((S[k] > 0).sum()), lg.BAND_HI, float(q[heavy].max()) if heavy.any() else 0.0))


@pytest.mark.parametrize("name", [c.name for c in lg.CASES])
def test_every_element_at_its_own_scale(name):
    lc = lg.BY_NAME[name]
    c = lc.case
    sc = lg.case_scene(lc)
    truth, S = lg.case_truth(lc, sc)
    prod = build_product(sc, DEV, **lg.samples_of(lc))
    prod[0].bwd_max_blocks = c.cap
    got = hip_render(sc, c.stage, device=DEV, backward=True, with_depth=c.with_depth, product=prod, want=c.want)
    keys = lg.gated(truth)
    assert set(keys) <= set(got), (name, sorted(set(keys) - set(got)))
    rho_ref = lg.committed_noise(name)
    bad, ratios, ref = [], [], None
    for k in keys:
        e, i = lg.local_err(got[k], truth[k], S[k])
        ratios.append("%s %s" % (k, "%.2f" % (e / rho_ref[k]) if rho_ref[k] > 0 else ("0" if e == 0 else "inf")))
        gate = lg.margin(name, k) * rho_ref[k]
        miss, what = e > gate, "local_err %.2e against %.1f x rho_ref = %.2e" % (e, lg.margin(name, k), gate)
        if not miss and lg.is_grid(k) and (lg._np(got[k])[S[k] == 0] != 0).any():        # no sample reaches it: exactly zero
            miss, what, x = True, "not zero where no sample reaches", np.where(S[k] == 0, np.abs(lg._np(got[k])), 0.0)
            i = tuple(int(v) for v in np.unravel_index(int(np.argmax(x)), x.shape))
        if miss:
            ref = ref or lg.case_oracle(lc, sc)
            bad.append(what + "; " + _describe(name, k, got, truth, S, ref, i, gate))
    print("local/%s rho_got / rho_ref: %s" % (name, "  ".join(ratios)))
    assert not bad, "\n".join(bad)
