"""CPU tests of the rendering figure (nice_slam_amd/csrc/nsr_figure.h, nice_slam_amd/imgeval.py): the kernel sources run on the
emulator against the numpy restatement (tests/figure_reference.py) byte for byte, the restatement against matplotlib itself,
then the properties that need no reference (batch independence, repeatability, white margins, the maxima and residual maps of
image_metrics), the colour map alone, the ABI's error paths, Visualizer over a stub renderer, the command line and
evaluate_rendering(figures=...)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emu_harness
import figure_reference as R
from nice_slam_amd import imgeval
from nice_slam_amd.engine import Engine


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def imgs():
    return R.main_case()


@pytest.fixture(scope="module")
def default_sheet(E, imgs):
    sheet, vmax = imgeval.figure_sheet(*imgs, engine=E, return_vmax=True)
    return sheet.numpy(), vmax.numpy()


# ---- 1. against the restatement, byte for byte ----------------------------------------------------------------------------------
def test_inputs_hold_their_cases(imgs):
    R.assert_main_case_holds_its_cases(imgs)


@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: "s%d_m%d_g%d" % l)
def test_sheet_matches_restatement(E, imgs, layout):
    got, vmax = imgeval.figure_sheet(*imgs, *layout, engine=E, return_vmax=True)
    want, want_vmax = R.expected_sheet(*imgs, *layout)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert vmax.numpy().tobytes() == want_vmax.tobytes() and float(vmax[1]) == 0.0
    diff = int((got.numpy() != want).sum())
    print(f"layout {layout}: sheet {want.shape}, {diff} differing bytes")
    assert diff == 0


@pytest.mark.parametrize("hw", R.SMALL, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("layout", R.LAYOUTS, ids=lambda l: "s%d_m%d_g%d" % l)
def test_small_images_match_restatement(E, hw, layout):
    im = R.make_images(3, *hw, seed=11)
    got = imgeval.figure_sheet(*im, *layout, engine=E)
    want, _ = R.expected_sheet(*im, *layout)
    assert tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want)


def test_one_frame_in_one_sheet_out(E, imgs):
    one = imgeval.figure_sheet(*(x[0] for x in imgs), 2, 5, 3, engine=E)
    want, _ = R.expected_sheet(*(x[:1] for x in imgs), 2, 5, 3)
    assert one.dim() == 3 and np.array_equal(one.numpy(), want[0])


# ---- 2. the restatement against matplotlib ----------------------------------------------------------------------------------------
def test_restatement_is_matplotlibs(imgs):
    matplotlib = pytest.importorskip("matplotlib")
    from matplotlib.colors import Normalize
    plasma = matplotlib.colormaps["plasma"]
    assert np.array_equal(R.LUT, np.floor(np.asarray(plasma.colors) * 255.0).astype(np.uint8))
    color, gt_color, depth, gt_depth = imgs
    H, W = depth.shape[1:]
    want, vmaxes = R.expected_sheet(*imgs, 1, 0, 0)
    for k in range(len(depth)):
        dres, _ = R.residuals(color[k], gt_color[k], depth[k], gt_depth[k])
        for c, x in enumerate((gt_depth[k], depth[k], dres)):
            with np.errstate(all="ignore"):
                ref = plasma(Normalize(0, vmaxes[k])(x), bytes=True)[..., :3]
            ours = want[k, :H, c * W:(c + 1) * W]
            keep = ~np.isnan(x)
            assert np.array_equal(ours[keep], ref[keep]), (k, c)
            assert (ours[~keep] == 255).all()


# ---- 3. properties ----------------------------------------------------------------------------------------------------------------
def test_frame_alone_equals_frame_in_batch_and_order_does_not_leak(E, imgs, default_sheet):
    sheet, vmax = default_sheet
    for k in range(3):
        one, v = imgeval.figure_sheet(*(x[k] for x in imgs), engine=E, return_vmax=True)
        assert np.array_equal(one.numpy(), sheet[k]) and v.numpy().tobytes() == vmax[k].tobytes()
    perm = [2, 0, 1]
    shuffled = imgeval.figure_sheet(*(x[perm] for x in imgs), engine=E)
    assert np.array_equal(shuffled.numpy(), sheet[perm])


def test_two_runs_are_bit_identical(E, imgs, default_sheet):
    assert np.array_equal(imgeval.figure_sheet(*imgs, engine=E).numpy(), default_sheet[0])


def test_margins_gaps_and_size(E, imgs, default_sheet):
    sheet, _ = default_sheet
    H, W = imgs[2].shape[1:]
    for layout in R.LAYOUTS:
        assert imgeval.figure_sheet_size(H, W, *layout, engine=E) == R.sheet_size(H, W, *layout)
    assert sheet.shape[1:3] == imgeval.figure_sheet_size(H, W, engine=E) == (2 * 8 + 2 * 37 + 8, 2 * 8 + 3 * 53 + 2 * 8)
    outside = ~R.panel_mask(H, W, 1, 8, 8)
    assert outside.any() and (sheet[:, outside] == 255).all()
    assert (sheet[:, ~outside] != 255).any()


def test_vmax_and_residual_panels_are_image_metrics(E, imgs, default_sheet):
    sheet, vmax = default_sheet
    m = imgeval.image_metrics(*imgs, residuals=True, engine=E)
    assert vmax.tobytes() == m["depth_max"].numpy().tobytes()
    H, W = imgs[2].shape[1:]
    for k in range(3):
        dres, cres = m["depth_residual"][k].numpy(), m["color_residual"][k].numpy()
        assert np.array_equal(sheet[k, 8:8 + H, 8 + 2 * (W + 8):8 + 2 * (W + 8) + W], R.colormap(dres, vmax[k]))
        assert np.array_equal(sheet[k, 16 + H:16 + 2 * H, 8 + 2 * (W + 8):8 + 2 * (W + 8) + W], R.rgb_bytes(cres))
        assert np.array_equal(imgeval.colorize_depth(m["depth_residual"][k], vmax=float(vmax[k]), engine=E).numpy(), R.colormap(dres, vmax[k]))


def test_no_vmax_buffer_gives_the_same_sheet(E, imgs):
    """the C entry without vmax_out keeps the maxima inside the sheet's own memory"""
    p = emu_harness.ptr
    for B, H, W, layout in ((3, 37, 53, (2, 5, 3)), (3, 37, 53, (1, 8, 8)), (5, 1, 1, (1, 0, 0)), (3, 11, 4, (3, 0, 0))):
        im = imgs if (H, W) == (37, 53) else R.make_images(B, H, W, seed=5)
        want, _ = R.expected_sheet(*im, *layout)
        out = np.zeros(want.shape, np.uint8)
        assert E.lib.nsr_figure_sheet(*(p(x) for x in im), B, H, W, *layout, None, p(out), None) == 0
        assert np.array_equal(out, want), (B, H, W, layout)


def test_colorize_depth(E, imgs):
    depth = imgs[2]
    own = imgeval.colorize_depth(depth, engine=E)
    assert own.dtype == torch.uint8 and tuple(own.shape) == depth.shape + (3,)
    for k in range(3):                                                   # frame 2: a NaN (white, and not the maximum) and a +inf (the maximum)
        assert np.array_equal(own[k].numpy(), R.colormap(depth[k], R.fold_max(depth[k]))), k
    assert np.isnan(depth[2]).any() and (own[2].numpy()[np.isnan(depth[2])] == 255).all()
    given = imgeval.colorize_depth(depth, vmax=2.5, engine=E)
    assert np.array_equal(given.numpy(), R.colormap(depth, 2.5))
    per = np.array([1.0, 0.0, 3.0], np.float32)
    each = imgeval.colorize_depth(depth, vmax=per, engine=E).numpy()
    for k in range(3):
        assert np.array_equal(each[k], R.colormap(depth[k], per[k])), k
    assert (each[1][~np.isnan(depth[1])] == R.LUT[0]).all()              # vmax = 0: every value at index 0
    one = imgeval.colorize_depth(depth[0], engine=E)
    assert one.dim() == 3 and np.array_equal(one.numpy(), own[0].numpy())
    tiny = np.array([[[1.0, 3.0]], [[2.0, np.nan]], [[0.0, 0.0]], [[-1.0, -2.0]]], np.float32)      # two pixels: no room for a maximum in the output
    got = imgeval.colorize_depth(tiny, engine=E).numpy()
    for k in range(len(tiny)):
        assert np.array_equal(got[k], R.colormap(tiny[k], R.fold_max(tiny[k]))), k
    with pytest.raises(ValueError):
        imgeval.colorize_depth(depth, vmax=[1.0, 2.0], engine=E)


# ---- 4. ABI error paths and the Python pieces ----------------------------------------------------------------------------------------
def test_abi_error_paths(E):
    lib, p = E.lib, emu_harness.ptr
    color, gt_color, depth, gt_depth = R.make_images(1, 5, 7, seed=3)
    SH, SW = R.sheet_size(5, 7, 2, 1, 1)
    sheet = np.zeros((1, SH, SW, 3), np.uint8)
    vm = np.zeros(1, np.float32)

    def call(c=color, g=gt_color, d=depth, gd=gt_depth, B=1, H=5, W=7, stride=2, margin=1, gap=1, v=vm, s=sheet):
        return lib.nsr_figure_sheet(p(c), p(g), p(d), p(gd), B, H, W, stride, margin, gap, p(v), p(s), None)

    assert call() == 0 and call(v=None) == 0
    for kw in ({"c": None}, {"g": None}, {"d": None}, {"gd": None}, {"s": None}):
        assert call(**kw) != 0 and b"null" in lib.nsr_last_error(), kw
    assert call(stride=0) != 0 and b"stride" in lib.nsr_last_error()
    assert call(margin=-1) != 0 and b"margin" in lib.nsr_last_error()
    assert call(gap=-1) != 0 and b"gap" in lib.nsr_last_error()
    assert call(H=0) != 0 and call(W=32769) != 0 and b"32768" in lib.nsr_last_error()
    assert call(margin=32769) != 0 and call(stride=32769) != 0
    assert call(H=32768, W=32768) != 0 and b"2^31" in lib.nsr_last_error()         # stride 2: 3 SH SW = 2.4e9 bytes
    assert call(B=-1) != 0 and call(B=65536) != 0
    odd = np.zeros(sheet.size + 1, np.uint8)[1:]
    assert call(s=odd) != 0 and b"aligned" in lib.nsr_last_error()
    before = sheet.copy()
    assert call(B=0) == 0 and call(B=0, c=None, s=None) == 0 and np.array_equal(sheet, before)

    sh, sw = C.c_int32(0), C.c_int32(0)
    assert lib.nsr_figure_sheet_size(5, 7, 2, 1, 1, C.byref(sh), C.byref(sw)) == 0 and (sh.value, sw.value) == (SH, SW)
    assert lib.nsr_figure_sheet_size(5, 7, 0, 1, 1, C.byref(sh), C.byref(sw)) != 0
    assert lib.nsr_figure_sheet_size(5, 7, 2, -1, 1, C.byref(sh), C.byref(sw)) != 0
    assert lib.nsr_figure_sheet_size(5, 7, 2, 1, 1, None, C.byref(sw)) != 0 and b"null" in lib.nsr_last_error()
    assert lib.nsr_figure_sheet_size(32768, 32768, 1, 0, 0, C.byref(sh), C.byref(sw)) != 0

    rgb = np.zeros((1, 5, 7, 3), np.uint8)
    assert lib.nsr_depth_colorize(p(depth), 1, 5, 7, p(vm), p(rgb), None) == 0 and lib.nsr_depth_colorize(p(depth), 1, 5, 7, None, p(rgb), None) == 0
    assert lib.nsr_depth_colorize(None, 1, 5, 7, None, p(rgb), None) != 0 and b"null" in lib.nsr_last_error()
    assert lib.nsr_depth_colorize(p(depth), 1, 5, 7, None, None, None) != 0
    assert lib.nsr_depth_colorize(p(depth), 1, 0, 7, None, p(rgb), None) != 0 and lib.nsr_depth_colorize(p(depth), -1, 5, 7, None, p(rgb), None) != 0
    assert lib.nsr_depth_colorize(None, 0, 5, 7, None, None, None) == 0
    with pytest.raises(ValueError):
        imgeval.figure_sheet(color, gt_color, depth[:, :4], gt_depth, engine=E)
    with pytest.raises(Exception):
        imgeval.figure_sheet(color, gt_color, depth, gt_depth, stride=0, engine=E)


class StubRenderer:
    """render_img returns the prepared images of the frame whose index the pose carries in its translation's x"""

    def __init__(self, color, depth):
        self.color, self.depth, self.calls, self.poses = color, depth, [], []

    def render_img(self, c, decoders, c2w, device, stage, gt_depth=None):
        assert tuple(c2w.shape) == (4, 4) and gt_depth is not None
        k = int(round(float(c2w[0, 3])))
        self.calls.append((k, stage, device))
        self.poses.append(c2w.clone())
        return torch.from_numpy(self.depth[k]).double(), None, torch.from_numpy(self.color[k])


def host_camera(t):
    """[R | T] of (quaternion, translation) on the host (get_camera_from_tensor itself runs on the GPU only)"""
    w, x, y, z = (float(v) for v in t[:4])
    rot = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float32)
    return torch.cat([rot, t[4:, None].float()], 1)


def test_visualizer_with_a_stub_renderer(E, imgs, tmp_path, monkeypatch):
    from PIL import Image
    seen = []
    monkeypatch.setattr(imgeval, "get_camera_from_tensor", lambda t: seen.append(t.clone()) or host_camera(t))
    color, gt_color, depth, gt_depth = imgs
    stub = StubRenderer(color, depth)
    vis_dir = tmp_path / "tracking_vis"
    vis = imgeval.Visualizer(2, 5, str(vis_dir), stub, False, "cpu", stride=1, margin=3, gap=2, engine=E)
    assert vis_dir.is_dir()
    gd, gc = torch.from_numpy(gt_depth[0]), torch.from_numpy(gt_color[0])
    pose = torch.eye(4)
    for idx in range(4):                                                 # the rule: idx % 2 == 0 and iter % 5 == 0
        for it in range(7):
            out = vis.vis(idx, it, gd, gc, pose, None, None)
            assert (out is not None) == (idx % 2 == 0 and it % 5 == 0)
    assert sorted(os.listdir(vis_dir)) == ["00000_0000.jpg", "00000_0005.jpg", "00002_0000.jpg", "00002_0005.jpg"]
    assert len(stub.calls) == 4 and stub.calls[0] == (0, "color", "cpu") and vis.drawn == 4
    SH, SW = R.sheet_size(37, 53, 1, 3, 2)
    with Image.open(vis_dir / "00002_0005.jpg") as im:
        assert im.size == (SW, SH) and im.mode == "RGB"
    # the camera-tensor path: a rotation about z and a translation whose x names frame 2
    cam = torch.tensor([np.cos(0.3), 0.0, 0.0, np.sin(0.3), 2.0, -0.5, 0.25], dtype=torch.float32)
    stub.poses.clear()
    sheet = vis.vis(4, 10, gd, gc, cam, None, None)
    want_pose = torch.cat([host_camera(cam), torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    assert len(seen) == 1 and torch.equal(seen[0], cam) and len(stub.poses) == 1 and torch.equal(stub.poses[0], want_pose) and stub.calls[-1][0] == 2
    want, _ = R.expected_sheet(color[2:3], gt_color[:1], depth[2:3], gt_depth[:1], 1, 3, 2)
    assert tuple(sheet.shape) == (1, SH, SW, 3) and np.array_equal(sheet[0].numpy(), want[0])
    assert (vis_dir / "00004_0010.jpg").is_file()
    # several poses of one frame: one launch, the due ones only, in the order given
    launches = []
    real = E.lib.nsr_figure_sheet
    E.lib.nsr_figure_sheet = lambda *a: launches.append(a[4]) or real(*a)
    try:
        poses = []
        for k in (1, 0, 2):
            t = torch.eye(4)
            t[0, 3] = k
            poses.append(t)
        sheets = vis.vis_many(6, [0, 3, 5], poses, gd, gc, None, None)
    finally:
        E.lib.nsr_figure_sheet = real
    assert launches == [2] and tuple(sheets.shape) == (2, SH, SW, 3)
    want, _ = R.expected_sheet(color[[1, 2]], gt_color[[0, 0]], depth[[1, 2]], gt_depth[[0, 0]], 1, 3, 2)
    assert np.array_equal(sheets.numpy(), want)
    assert (vis_dir / "00006_0000.jpg").is_file() and (vis_dir / "00006_0005.jpg").is_file() and not (vis_dir / "00006_0003.jpg").exists()
    assert vis.due_iters(6, 12) == [0, 5, 10] and vis.due_iters(7, 12) == []


def test_visualizer_off(E, imgs, tmp_path):
    stub = StubRenderer(imgs[0], imgs[2])
    for freq, inside in ((0, 5), (50, 0), (-1, -1)):
        vis = imgeval.Visualizer(freq, inside, str(tmp_path / f"v{freq}_{inside}"), stub, False, "cpu", engine=E)
        assert not vis.on and not vis.due(0, 0) and vis.due_iters(0, 10) == []
        assert vis.vis(0, 0, torch.from_numpy(imgs[3][0]), torch.from_numpy(imgs[1][0]), torch.eye(4), None, None) is None
        assert not (tmp_path / f"v{freq}_{inside}").exists()
    assert stub.calls == []


def test_command_line_figures(E, imgs, tmp_path, capsys, monkeypatch):
    from PIL import Image
    saved, real = {}, imgeval.save_sheet                                 # JPEG is lossy: the bytes are compared before the file is written
    monkeypatch.setattr(imgeval, "save_sheet", lambda sheet, path, **kw: saved.__setitem__(os.path.basename(path), sheet.numpy().copy()) or real(sheet, path, **kw))
    np.savez(tmp_path / "rendered.npz", color=imgs[0], depth=imgs[2])
    np.savez(tmp_path / "gt.npz", color=imgs[1], depth=imgs[3])
    out = tmp_path / "figs"
    assert imgeval.main([str(tmp_path / "rendered.npz"), str(tmp_path / "gt.npz"), "--figures", str(out)], engine=E) == 0
    assert [ln.split(":")[0] for ln in capsys.readouterr().out.strip().splitlines()] == ["PSNR", "SSIM", "Depth L1"]
    assert sorted(os.listdir(out)) == ["00000.jpg", "00001.jpg", "00002.jpg"]
    SH, SW = R.sheet_size(37, 53, 1, 8, 8)
    with Image.open(out / "00001.jpg") as im:
        assert im.size == (SW, SH) and im.mode == "RGB"
    want, _ = R.expected_sheet(*imgs)
    for k in range(3):
        assert np.array_equal(saved[f"{k:05d}.jpg"], want[k])


def test_evaluate_rendering_figures(E, imgs, tmp_path, monkeypatch):
    color, gt_color, depth, gt_depth = imgs
    frames = []
    for k in range(3):
        c2w = torch.eye(4)
        c2w[0, 3] = k
        frames.append((10 * k, torch.from_numpy(gt_color[k]), torch.from_numpy(gt_depth[k]), c2w))
    saved, real = {}, imgeval.save_sheet
    monkeypatch.setattr(imgeval, "save_sheet", lambda sheet, path, **kw: saved.__setitem__(os.path.basename(path), sheet.numpy().copy()) or real(sheet, path, **kw))
    out = imgeval.evaluate_rendering(StubRenderer(color, depth), None, None, frames, device="cpu", batch=2, engine=E,
                                     figures=str(tmp_path / "figs"))
    assert out["n_frames"] == 3
    assert sorted(os.listdir(tmp_path / "figs")) == ["00000.jpg", "00010.jpg", "00020.jpg"] == sorted(saved)
    want, _ = R.expected_sheet(*imgs)
    for k in range(3):
        assert np.array_equal(saved[f"{10 * k:05d}.jpg"], want[k])
