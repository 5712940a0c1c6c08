"""GPU, two devices in one process: every library entry launches on the CURRENT device, so a call on tensors of ``cuda:1`` while
``cuda:0`` is current has to make ``cuda:1`` current for its launches and put ``cuda:0`` back (nice_slam_amd/engine.py,
``Engine.call``) -- the reference lets tracking and mapping name different devices (configs/nice_slam.yaml:31,44).  The same calls
with everything on ``cuda:0`` are the reference: equal forward results (the mapper's atomically summed loss: equal to the rounding
of its fp64 sum), gradients equal to the noise of the gradient atomics.
Skips where the process sees one GPU; tests/test_host_logic.py holds the switching logic on a fake device layer."""
import numpy as np
import pytest
import torch

from scene_util import build_product, make_scene, rel_err

pytestmark = pytest.mark.gpu


def _here():
    assert torch.cuda.current_device() == 0


def run_calls(dev):
    """Every kind of library call of the render path on tensors of ``dev`` with cuda:0 current -> ({name: forward result}, {name: gradient})."""
    import nice_slam_amd as nsa
    from nice_slam_amd import _capi, bound
    dev = torch.device(dev)
    sc = make_scene(seed=6, n_rays=96, small=True)
    H, W, fx, fy, cx, cy = sc["intr"]
    renderer, dec, grids = build_product(sc, dev)
    depth_img, color_img, c2w = sc["depth_img"].to(dev), sc["color_img"].to(dev), sc["c2w"].to(dev)
    fwd, grad = {}, {}

    def leaves():
        for p in dec.parameters():
            p.requires_grad_(True)
            p.grad = None
        return {k: v.detach().clone(memory_format=torch.preserve_format).requires_grad_(True) for k, v in grids.items()}

    def collect(tag, c, poses=()):
        for k, v in c.items():
            if v.grad is not None:
                grad[f"{tag}/{k}"] = v.grad.clone()
        for k, p in dec.named_parameters():
            if p.grad is not None:
                grad[f"{tag}/param/{k}"] = p.grad.clone()
        for i, p in enumerate(poses):
            grad[f"{tag}/pose{i}"] = p.grad.clone()

    torch.manual_seed(5)                                                   # get_samples draws with torch.randint on `dev`
    o, d, gd, gc = nsa.get_samples(2, H - 2, 3, W - 3, 96, H, W, fx, fy, cx, cy, c2w, depth_img, color_img, dev)
    _here()
    fwd.update(gs_o=o, gs_d=d, gs_depth=gd, gs_color=gc)

    c = leaves()
    ro, rd = sc["rays_o"].to(dev).requires_grad_(True), sc["rays_d"].to(dev).requires_grad_(True)
    depth, var, rgb = renderer.render_batch_ray(c, dec, rd, ro, dev, "color", gt_depth=sc["gt_depth"].to(dev))
    _here()
    w = sc["w"]
    ((depth * w["depth"].to(dev)).sum() + (var * w["var"].to(dev)).sum() + (rgb * w["rgb"].to(dev)).sum()).backward()
    _here()
    fwd.update(r_depth=depth.detach(), r_var=var.detach(), r_rgb=rgb.detach())
    collect("render", c, (ro, rd))

    K, n = 2, 48
    idx = torch.randint(H * W, (K * n,), generator=torch.Generator().manual_seed(5))
    c = leaves()
    frames = [((c2w if k == 0 else c2w[:3].contiguous()).clone().requires_grad_(True), depth_img * (1.0 + 0.03 * k), color_img)
              for k in range(K)]
    out = {}
    loss = nsa.mapping_loss(renderer, c, dec, frames, n, "color", w_color=0.2, indices=idx, out=out)
    _here()
    nsa.backward(loss)
    _here()
    fwd.update(m_loss=loss.detach(), m_depth=out["depth"], m_color=out["color"], m_keep=out["keep"], m_kmax=out["kept_max"])
    collect("mapping", c, [f[0] for f in frames])

    c = leaves()
    pose = c2w.clone().requires_grad_(True)
    out = {}
    loss = nsa.tracking_loss(renderer, {k: v.detach() for k, v in c.items()}, dec, pose, depth_img, color_img, 96, 2, 3,
                             indices=idx[:96] % ((H - 4) * (W - 6)), out=out)
    _here()
    loss.backward()
    _here()
    fwd.update(t_loss=loss.detach(), t_depth=out["depth"], t_color=out["color"], t_keep=out["keep"])
    collect("tracking", {}, [pose])

    # the optimisers: the same gradients on both devices (Adam's first steps are +-lr by the gradient's SIGN: no tolerance fits them)
    g = torch.Generator().manual_seed(9)
    keys = ["grid_middle", "grid_fine"]
    for capturable in (False, True):
        cc = {k: grids[k].detach().clone(memory_format=torch.preserve_format) for k in keys}
        gg = {k: nsa.to_channels_last(torch.randn(cc[k].shape, generator=g).to(dev)) for k in keys}
        opt = nsa.MaskedGridAdam(cc, capturable=capturable)
        for _ in range(2):
            opt.step({k: 1e-2 for k in keys}, grads=gg)
            _here()
        fwd.update({f"adam{int(capturable)}/{k}": cc[k] for k in keys})
    cam = torch.randn((7,), generator=g).to(dev).requires_grad_(True)
    cam.grad = torch.randn((7,), generator=g).to(dev)
    fopt = nsa.FlatAdam([cam], lr=1e-2)
    for _ in range(2):
        fopt.step()
        _here()
    fwd["flat_adam"] = cam.detach()

    fwd["frustum"] = nsa.FrustumSelector(sc["bound"], H, W, fx, fy, cx, cy).voxel_mask(sc["c2w"], "grid_middle",
                                                                                       grids["grid_middle"].shape[2:], depth_img)
    _here()
    sel = nsa.KeyframeSelector(H, W, fx, fy, cx, cy)
    kfs = [sc["c2w"].clone() for _ in range(3)]
    for k, p in enumerate(kfs):
        p[:3, 3] += 0.05 * k
    fwd["overlap"] = sel.overlap(c2w, depth_img, kfs, indices=idx[:50])
    _here()
    with pytest.raises(_capi.NsrError):
        sel.overlap(c2w, depth_img[:-1], kfs, indices=idx[:50])
    _here()

    lo, hi = sc["bound"][:, 0].numpy(), sc["bound"][:, 1].numpy()
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float64)
    verts, _, faces, planes = bound.convex_hull(corners * 0.5 + corners.mean(0) * 0.5)
    pts = (torch.rand((257, 3), generator=g, dtype=torch.float64) * torch.from_numpy(hi - lo) + torch.from_numpy(lo)).to(dev)
    fwd["contains"] = bound.ConvexBound(verts, faces, planes).contains(pts)
    _here()
    assert fwd["contains"].device == dev and 0 < int(fwd["contains"].sum()) < 257
    torch.cuda.synchronize(dev)
    return fwd, grad


def compare(got_fwd, got_grad, ref_fwd, ref_grad):
    assert set(got_fwd) == set(ref_fwd) and set(got_grad) == set(ref_grad)
    for k, v in got_fwd.items():
        if k == "m_loss":
            # the mapper's loss is summed by the forward kernel with fp64 atomics, in the order the blocks arrive: n = 96 rays x
            # (1 depth + 3 colour) non-negative terms, so two orders differ by at most 2 (n - 1) 2^-53 of the sum
            assert abs(float(v) - float(ref_fwd[k])) <= 2 * (96 * 4 - 1) * 2.0 ** -53 * abs(float(ref_fwd[k])), (k, float(v), float(ref_fwd[k]))
        else:
            assert torch.equal(v.cpu(), ref_fwd[k].cpu()), k
    for k, v in got_grad.items():
        # two evaluations of one iteration differ by the order of the gradient atomics (tests/test_hip_mapping.py:199-201)
        assert rel_err(v, ref_grad[k]) < (2e-5 if "/param/" in k else 1e-5), k


def test_calls_on_another_device_than_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs in one process")
    with torch.cuda.device(0):
        ref_fwd, ref_grad = run_calls("cuda:0")
        got_fwd, got_grad = run_calls("cuda:1")
    assert all(v.device == torch.device("cuda", 1) for v in list(got_fwd.values()) + list(got_grad.values()))
    compare(got_fwd, got_grad, ref_fwd, ref_grad)
