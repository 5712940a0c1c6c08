"""CPU tests of the frame preparation (nice_slam_amd/csrc/nsr_frame.h) and the sequence readers (nice_slam_amd/datasets.py): the
kernel sources run on the emulator against the restatement of tests/frames_reference.py under the gates derived there, against
what the unmodified reference returned (tests/golden/frames.npz), and the readers on folders written under tmp_path."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import emu_harness
import frames_reference as R
from conftest import GOLDEN
from nice_slam_amd import _capi, datasets, imgeval
from nice_slam_amd.datasets import FramePreparer, get_dataset
from nice_slam_amd.engine import Engine

LAYOUTS = ("replica", "scannet", "azure")


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "frames.npz"))
    return {k: z[k] for k in z.files}


def gold_cfg(gold, layout, folder=""):
    cfg = json.loads(str(gold[f"{layout}/cfg"]))
    cfg["data"]["input_folder"] = str(folder)
    return cfg


# --------------------------------------------------------------------------------------------------
# the kernels against the restatement
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_case_matches_restatement(E, name):
    R.run_and_check(E, name)


def test_restatement_flags_no_ties_and_sees_the_zero_border():
    for name, case in R.CASES.items():
        if "distortion" not in case[3]:
            continue
        cfg, color, depth, bgr = R.build_case(name)
        for k in range(color.shape[0]):
            ref = R.prepare(color[k], depth[k], cfg, bgr)
            assert not ref["ties"].any(), (name, k)                  # so the colour of every distortion case is compared
            if name == "undistort_zero_border":
                assert ref["outside_taps"] >= 20
                assert (ref["undistorted"][0, 0] == 0).all() and ref["undistorted"].any()


def test_cases_cover_the_paths():
    kinds = set()
    for name in R.CASES:
        cfg, color, depth, _ = R.build_case(name)
        cam = cfg["cam"]
        kinds.add(("distortion" in cam, color.shape[1:3] != depth.shape[1:3], "crop_size" in cam, cam["crop_edge"] > 0, depth.dtype == np.float32))
    assert (False, False, False, False, False) in kinds and (True, True, True, True, False) in kinds
    assert (False, False, False, True, False) in kinds and (False, False, False, False, True) in kinds and (False, False, True, False, True) in kinds


@pytest.mark.parametrize("name", ["identity_24x40", "all_stages"])
def test_frames_of_a_batch_equal_their_single_frame_results(E, name):
    cfg, color, depth, bgr = R.build_case(name)
    color, depth = np.concatenate([color, color[:1]]), np.concatenate([depth, depth[:1]])          # B = 3
    prep = FramePreparer(cfg, engine=E)
    bc, bd = prep.prepare(color, depth, bgr=bgr)
    assert bc.shape[0] == 3 and bc.dtype == torch.float32 and bd.dtype == torch.float32
    for k in range(3):
        c1, d1 = prep.prepare(color[k], depth[k], bgr=bgr)
        assert c1.dim() == 3 and d1.dim() == 2
        assert c1.numpy().tobytes() == bc[k].numpy().tobytes() and d1.numpy().tobytes() == bd[k].numpy().tobytes(), (name, k)
    assert bc[0].numpy().tobytes() == bc[2].numpy().tobytes()


def test_empty_batch(E):
    cfg, color, depth, bgr = R.build_case("all_stages")
    c, d = FramePreparer(cfg, engine=E).prepare(color[:0], depth[:0], bgr=bgr)
    assert tuple(c.shape) == (0, 20, 28, 3) and tuple(d.shape) == (0, 20, 28)


def test_input_forms(E):
    cfg, color, depth, bgr = R.build_case("crop_down_edge2")
    prep = FramePreparer(cfg, engine=E)
    want_c, want_d = (x.numpy().tobytes() for x in prep.prepare(color, depth, bgr=bgr))

    def same(c, d):
        gc, gd = prep.prepare(c, d, bgr=bgr)
        return gc.numpy().tobytes() == want_c and gd.numpy().tobytes() == want_d

    assert same(torch.from_numpy(color), torch.from_numpy(depth.view(np.int16)))
    if hasattr(torch, "uint16"):
        assert same(torch.from_numpy(color), torch.from_numpy(depth.view(np.int16)).view(torch.uint16))
    wide = np.zeros(color.shape[:2] + (2 * color.shape[2], 3), np.uint8)
    wide[:, :, ::2] = color
    assert same(torch.from_numpy(wide)[:, :, ::2], depth)                       # not contiguous
    assert same(color, depth.astype(np.float64)) and same(color, depth.astype(np.float32))      # u16 values are exact in fp32
    with pytest.raises(ValueError):
        prep.prepare(color.astype(np.float32), depth)
    with pytest.raises(ValueError):
        prep.prepare(color, depth.astype(np.int32))
    with pytest.raises(ValueError):
        prep.prepare(color, depth[:0])
    with pytest.raises(ValueError):
        prep.prepare(color[..., :2], depth)


# --------------------------------------------------------------------------------------------------
# against the unmodified reference
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_golden_frames(E, gold, layout):
    cfg = gold_cfg(gold, layout)
    raw_c, raw_d = gold[f"{layout}/raw_color"], gold[f"{layout}/raw_depth"]
    want64, want_d = gold[f"{layout}/color"], gold[f"{layout}/depth"]
    assert want64.dtype == np.float64 and raw_d.dtype == np.uint16
    prep = FramePreparer(cfg, engine=E)
    got_c, got_d = prep.prepare(R.guarded(raw_c), R.guarded(raw_d), bgr=False)
    got_c, got_d = got_c.numpy(), got_d.numpy()
    assert got_d.tobytes() == want_d.tobytes()
    if "crop_size" in cfg["cam"]:
        assert np.abs(got_c.astype(np.float64) - want64.astype(np.float32)).max() <= R.COLOR_TOL
    else:
        assert got_c.tobytes() == want64.astype(np.float32).tobytes()
    for k in range(len(raw_c)):                                        # the restatement is the reference's arithmetic
        ref = R.prepare(raw_c[k], raw_d[k], cfg, bgr=False)
        assert ref["color64"].tobytes() == want64[k].tobytes() and ref["depth"].tobytes() == want_d[k].tobytes()
    bgr_c, _ = prep.prepare(np.ascontiguousarray(raw_c[..., ::-1]), raw_d, bgr=True)          # what cv2.imread would have handed over
    assert bgr_c.numpy().tobytes() == got_c.tobytes()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_camera_is_update_cam(E, gold, layout):
    cfg = gold_cfg(gold, layout)
    prep = FramePreparer(cfg, engine=E)
    cam = prep.camera
    assert list(cam) == gold[f"{layout}/cam"].tolist() and isinstance(cam[0], int) and isinstance(cam[1], int)
    assert cam == R.update_cam(cfg) and prep.out_size == tuple(gold[f"{layout}/depth"].shape[1:])


# --------------------------------------------------------------------------------------------------
# the ABI's error paths
# --------------------------------------------------------------------------------------------------
def test_abi_error_paths(E):
    lib = E.lib
    cfg, color, depth, bgr = R.build_case("all_stages")
    prep = FramePreparer(cfg, engine=E)
    B = color.shape[0]
    p = emu_harness.ptr

    def desc(**kw):
        d = prep.desc(color.shape[1:3], depth.shape[1:3], False, bgr)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    good = desc()
    H, W = C.c_int32(), C.c_int32()
    assert lib.nsr_frame_out_size(C.byref(good), C.byref(H), C.byref(W)) == 0 and (H.value, W.value) == (20, 28)
    n = lib.nsr_frame_workspace_bytes(C.byref(good), B)
    assert n == color.size and lib.nsr_frame_workspace_bytes(C.byref(desc(has_distortion=0)), B) == 0
    assert lib.nsr_frame_workspace_bytes(C.byref(good), 0) == 0 and lib.nsr_frame_workspace_bytes(C.byref(good), -1) == -1
    assert lib.nsr_frame_workspace_bytes(C.byref(desc(color_h=0)), B) == -1 and lib.nsr_frame_workspace_bytes(None, B) == -1
    out_c, out_d = np.zeros((B, 20, 28, 3), np.float32), np.zeros((B, 20, 28), np.float32)
    ws = np.zeros(n, np.uint8)

    def call(d=good, c=color, dp=depth, B=B, oc=out_c, od=out_d, w=ws, nbytes=n):
        return lib.nsr_frame_prepare(p(c), p(dp), C.byref(d) if d is not None else None, B, p(oc), p(od), p(w), nbytes, None)

    def fails(msg, **kw):
        assert call(**kw) != 0, kw
        assert msg in lib.nsr_last_error(), (kw, lib.nsr_last_error())

    assert call() == 0 and out_c.any()
    before = out_c.copy()
    for kw in ({"c": None}, {"dp": None}, {"oc": None}, {"od": None}, {"w": None}, {"d": None}):
        fails(b"null", **kw)
    assert lib.nsr_frame_out_size(None, C.byref(H), C.byref(W)) != 0 and b"null" in lib.nsr_last_error()
    assert lib.nsr_frame_out_size(C.byref(good), None, C.byref(W)) != 0 and b"null" in lib.nsr_last_error()
    fails(b"negative", B=-1)
    for field in ("color_h", "color_w", "depth_h", "depth_w"):
        for v in (0, -3, 32769):
            fails(b"image sizes", d=desc(**{field: v}))
    for kw in ({"crop_h": 32769}, {"crop_w": -1}, {"crop_h": 0}, {"crop_w": 0}):
        fails(b"crop_h and crop_w", d=desc(**kw))
    fails(b"crop_edge", d=desc(crop_edge=12))                          # 2 e = Hs = 24
    fails(b"crop_edge", d=desc(crop_h=40, crop_w=32, crop_edge=16))    # 2 e = Ws
    fails(b"crop_edge", d=desc(crop_edge=-1))
    assert call(d=desc(crop_edge=11), oc=np.zeros((B, 2, 10, 3), np.float32), od=np.zeros((B, 2, 10), np.float32)) == 0
    for v in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
        fails(b"png_depth_scale", d=desc(png_depth_scale=v))
    fails(b"fx and fy", d=desc(fx=0.0))
    fails(b"fx and fy", d=desc(fy=0.0))
    assert call(d=desc(fx=0.0, has_distortion=0), w=None, nbytes=0) == 0          # the intrinsics are read with distortion only
    fails(b"depth_type", d=desc(depth_type=2))
    fails(b"workspace too small", nbytes=n - 1)
    out_c[:] = 5.0
    assert call(B=0) == 0 and call(B=0, c=None, dp=None, oc=None, od=None, w=None, nbytes=0) == 0 and (out_c == 5.0).all()
    fails(b"image sizes", B=0, d=desc(color_h=0))                      # an invalid description is one for an empty batch too
    assert call() == 0 and out_c.tobytes() == before.tobytes()


# --------------------------------------------------------------------------------------------------
# the sequence readers
# --------------------------------------------------------------------------------------------------
def written(layout, gold, tmp_path, numbers=None, poses=True):
    """the golden case's sequence, written again under tmp_path -> (cfg, the fp64 poses written)"""
    n = len(gold[f"{layout}/raw_color"])
    H, W = gold[f"{layout}/raw_color"].shape[1:3]
    colors, depths = R.make_frames(n, (H, W), (H, W), seed=len(layout))
    mats = R.make_poses(n, seed=len(layout))
    folder = tmp_path / layout
    R.write_sequence(layout, str(folder), colors, depths, mats if poses else None, numbers)
    return gold_cfg(gold, layout, folder), mats


def check_frames(ds, cfg, gold, layout):
    """every frame of the reader against the reference's tuple for the same files"""
    assert len(ds) == len(gold[f"{layout}/raw_color"]) and ds.camera == R.update_cam(cfg)
    for i in range(len(ds)):
        raw_c, raw_d = ds.read_raw(i)
        assert raw_c.dtype == np.uint8 and raw_d.dtype == np.uint16
        assert np.array_equal(raw_d, gold[f"{layout}/raw_depth"][i])                   # PNG is lossless: the loader's order
        idx, color, depth, c2w = ds[i]
        assert idx == i and color.dtype == torch.float32 and depth.dtype == torch.float32 and c2w.dtype == torch.float32
        ref = R.prepare(raw_c, raw_d, cfg, bgr=False)
        assert depth.numpy().tobytes() == ref["depth"].tobytes() == gold[f"{layout}/depth"][i].tobytes()
        assert np.abs(color.numpy().astype(np.float64) - ref["color"]).max() <= (R.COLOR_TOL if "crop_size" in cfg["cam"] else 0.0)
        assert tuple(color.shape[:2]) == ds.camera[:2]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reader_matches_the_reference(E, gold, tmp_path, layout):
    numbers = [0, 1, 2, 9, 10] if layout == "scannet" else None
    cfg, mats = written(layout, gold, tmp_path, numbers)
    ds = get_dataset(cfg, device="cpu", engine=E)
    assert type(ds).__name__ == {"replica": "Replica", "scannet": "ScanNet", "azure": "Azure"}[layout]
    if layout == "scannet":
        assert [os.path.basename(p) for p in ds.color_paths] == ["0.jpg", "1.jpg", "2.jpg", "9.jpg", "10.jpg"]
        assert [os.path.basename(p) for p in ds.depth_paths] == ["0.png", "1.png", "2.png", "9.png", "10.png"]
    check_frames(ds, cfg, gold, layout)
    scale = cfg["scale"]
    for i in range(len(ds)):
        want = mats[i].copy()
        want[:3, 1] *= -1                                              # the y / z flip of the loaders
        want[:3, 2] *= -1
        want = torch.from_numpy(want).float()
        want[:3, 3] *= scale
        first, second = ds[i][3], ds[i][3]
        assert first.numpy().tobytes() == want.numpy().tobytes() == gold[f"{layout}/pose"][i].tobytes()
        assert second.numpy().tobytes() == first.numpy().tobytes()     # the scale is applied once
    if scale != 1.0:                                                   # ... where the reference applies it on every access
        assert not np.array_equal(gold[f"{layout}/pose_twice"], gold[f"{layout}/pose"][0])
    idx, color, depth, c2w = ds.load_batch([2, 0])
    assert idx == [2, 0] and tuple(c2w.shape) == (2, 4, 4)
    for j, i in enumerate(idx):
        one = ds[i]
        assert color[j].numpy().tobytes() == one[1].numpy().tobytes() and depth[j].numpy().tobytes() == one[2].numpy().tobytes()
        assert torch.equal(c2w[j], one[3])
    with pytest.raises(IndexError):
        ds[len(ds)]


def test_input_folder_and_scale_arguments(E, gold, tmp_path):
    cfg, _ = written("replica", gold, tmp_path)
    folder, cfg["data"]["input_folder"] = cfg["data"]["input_folder"], "/nowhere"
    ds = get_dataset(cfg, input_folder=folder, scale=2.0, device="cpu", engine=E)
    base = get_dataset(dict(cfg, scale=1.0), input_folder=folder, device="cpu", engine=E)
    assert torch.equal(ds[1][3][:3, 3], base[1][3][:3, 3] * 2.0) and torch.equal(ds[1][3][:3, :3], base[1][3][:3, :3])
    assert torch.equal(ds[1][2], base[1][2] * 2.0)


def test_azure_without_a_trajectory_has_identity_poses(E, gold, tmp_path):
    cfg, _ = written("azure", gold, tmp_path, poses=False)
    ds = get_dataset(cfg, device="cpu", engine=E)
    assert len(ds) == 3 and all(torch.equal(ds[i][3], torch.eye(4)) for i in range(3))


def test_cofusion_needs_openexr_only_to_read(E, tmp_path):
    from PIL import Image
    color, _ = R.make_frames(2, (12, 16), (12, 16), seed=5)
    os.makedirs(tmp_path / "colour")
    os.makedirs(tmp_path / "depth_noise")
    for i in range(2):
        Image.fromarray(color[i]).save(tmp_path / "colour" / f"Color{i:04d}.png")
        (tmp_path / "depth_noise" / f"Depth{i:04d}.exr").write_bytes(b"\x76\x2f\x31\x01")
    cfg = R.make_cfg(12, 16, dataset="cofusion", input_folder=str(tmp_path), png_depth_scale=1.0)
    ds = get_dataset(cfg, device="cpu", engine=E)
    assert type(ds).__name__ == "CoFusion" and len(ds) == 2 and all(torch.equal(p, torch.eye(4)) for p in ds.poses)
    try:
        import OpenEXR  # noqa: F401
        import Imath  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="OpenEXR"):
            ds[0]


TUM_IMAGE_T = [0.00, 0.02, 0.04, 0.06, 0.10, 0.20, 0.30, 0.32, 0.40]
TUM_DEPTH_T = [0.005, 0.045, 0.105, 0.33, 0.41]
TUM_POSE_T = [0.0, 0.05, 0.1, 0.3, 0.35, 0.4]
# by hand: image 5 (t = 0.20) has no depth within 0.08; then frames closer than 1 / 32 s to the last kept one are thinned out
TUM_ASSOCIATIONS = [(0, 0, 0), (1, 0, 0), (2, 1, 1), (3, 1, 1), (4, 2, 2), (6, 3, 3), (7, 3, 3), (8, 4, 5)]
TUM_KEPT = [(0, 0, 0), (2, 1, 1), (4, 2, 2), (6, 3, 3), (8, 4, 5)]


def test_tum_association_by_hand():
    img, dep, pose = (np.array(t) for t in (TUM_IMAGE_T, TUM_DEPTH_T, TUM_POSE_T))
    got = datasets.TUM_RGBD.associate_frames(img, dep, pose)
    assert [tuple(int(v) for v in a) for a in got] == TUM_ASSOCIATIONS
    assert [tuple(int(v) for v in a) for a in datasets.TUM_RGBD.associate_frames(img, dep, None)] == [a[:2] for a in TUM_ASSOCIATIONS]
    assert datasets.TUM_RGBD.associate_frames(img, dep, pose, max_dt=0.004) == []


def test_tum_reader(E, tmp_path):
    from PIL import Image
    from scipy.spatial.transform import Rotation
    H, W = 14, 18
    colors, _ = R.make_frames(len(TUM_IMAGE_T), (H, W), (H, W), seed=3)
    _, depths = R.make_frames(len(TUM_DEPTH_T), (H, W), (H, W), seed=4)
    mats = R.make_poses(len(TUM_POSE_T), seed=9)
    os.makedirs(tmp_path / "rgb")
    os.makedirs(tmp_path / "depth")
    with open(tmp_path / "rgb.txt", "w") as f:
        f.write("# color images\n# file: 'hand made'\n# timestamp filename\n")
        for t, c in zip(TUM_IMAGE_T, colors):
            Image.fromarray(c).save(tmp_path / "rgb" / f"{t:.6f}.png")
            f.write(f"{t:.6f} rgb/{t:.6f}.png\n")
    with open(tmp_path / "depth.txt", "w") as f:
        f.write("# depth maps\n# file: 'hand made'\n# timestamp filename\n")
        for t, d in zip(TUM_DEPTH_T, depths):
            Image.fromarray(d).save(tmp_path / "depth" / f"{t:.6f}.png")
            f.write(f"{t:.6f} depth/{t:.6f}.png\n")
    with open(tmp_path / "groundtruth.txt", "w") as f:
        f.write("# ground truth trajectory\n# file: 'hand made'\n# timestamp tx ty tz qx qy qz qw\n")
        for t, m in zip(TUM_POSE_T, mats):
            f.write(" ".join(repr(float(v)) for v in [t, *m[:3, 3], *Rotation.from_matrix(m[:3, :3]).as_quat()]) + "\n")
    cfg = R.make_cfg(H, W, dataset="tumrgbd", input_folder=str(tmp_path), png_depth_scale=5000.0, scale=2.0, crop_size=(10, 14), crop_edge=1,
                     distortion=R.TUM_DISTORTION)
    ds = get_dataset(cfg, device="cpu", engine=E)
    assert type(ds).__name__ == "TUM_RGBD" and len(ds) == len(TUM_KEPT)
    assert [os.path.basename(p) for p in ds.color_paths] == [f"{TUM_IMAGE_T[i]:.6f}.png" for i, _, _ in TUM_KEPT]
    assert [os.path.basename(p) for p in ds.depth_paths] == [f"{TUM_DEPTH_T[j]:.6f}.png" for _, j, _ in TUM_KEPT]
    flip = np.diag([1.0, -1.0, -1.0, 1.0])
    assert torch.equal(ds[0][3], torch.from_numpy(flip).float())       # the first pose: identity, axes flipped
    for n, (i, j, k) in enumerate(TUM_KEPT):
        want = (np.linalg.inv(mats[TUM_KEPT[0][2]]) @ mats[k]) @ flip  # relative to the first kept frame; columns y, z negated
        want[:3, 3] *= 2.0
        idx, color, depth, c2w = ds[n]
        assert np.abs(c2w.numpy() - want).max() <= 1e-5
        raw_c, raw_d = ds.read_raw(n)
        assert np.array_equal(raw_c, colors[i]) and np.array_equal(raw_d, depths[j])
        ref = R.prepare(raw_c, raw_d, cfg, bgr=False)
        assert not ref["ties"].any()
        assert depth.numpy().tobytes() == ref["depth"].tobytes() and tuple(depth.shape) == (8, 12) == ds.camera[:2]
        assert np.abs(color.numpy().astype(np.float64) - ref["color"]).max() <= R.COLOR_TOL


# --------------------------------------------------------------------------------------------------
# the tuples feed the evaluation as they are
# --------------------------------------------------------------------------------------------------
class EchoRenderer:
    """render_img gives back the input depth and a constant colour"""

    def render_img(self, c, decoders, c2w, device, stage, gt_depth=None):
        assert tuple(c2w.shape) == (4, 4) and c2w.dtype == torch.float32
        return gt_depth.clone(), None, torch.full(tuple(gt_depth.shape) + (3,), 0.5)


def test_frames_feed_evaluate_rendering(E, gold, tmp_path):
    cfg, _ = written("replica", gold, tmp_path)
    ds = get_dataset(cfg, device="cpu", engine=E)
    out = imgeval.evaluate_rendering(EchoRenderer(), None, None, (ds[i] for i in range(len(ds))), device="cpu", engine=E)
    assert out["n_frames"] == 3 and [r["idx"] for r in out["frames"]] == [0, 1, 2]
    assert all(r["depth_l1_cm"] == 0.0 and np.isfinite(r["psnr"]) for r in out["frames"])


def test_frames_come_through_the_trackers_loader(E, gold, tmp_path):
    from torch.utils.data import DataLoader
    cfg, _ = written("replica", gold, tmp_path)
    ds = get_dataset(cfg, device="cpu", engine=E)
    seen = []
    for idx, gt_color, gt_depth, gt_c2w in DataLoader(ds, batch_size=1, shuffle=False, num_workers=0):       # Tracker.py:64-65, :153-158
        one = ds[int(idx[0])]
        assert torch.equal(gt_color[0], one[1]) and torch.equal(gt_depth[0], one[2]) and torch.equal(gt_c2w[0], one[3])
        seen.append(int(idx[0]))
    assert seen == [0, 1, 2]


def test_the_two_kernels_use_no_scratch():
    from nice_slam_amd import build
    res = json.load(open(build.RESOURCES))
    mine = {k: v for k, v in res.items() if "frame_prepare_kernel" in k or "frame_undistort_kernel" in k}
    assert len(mine) == 2 and all(v["scratch_bytes_per_lane"] == 0 for v in mine.values()), mine


def test_ctypes_descriptor_follows_the_header(tmp_path):
    import re
    import subprocess
    from conftest import ROOT
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsr.h")).read(), flags=re.S)
    body = re.search(r"typedef struct nsr_frame_desc \{(.*?)\} nsr_frame_desc;", txt, re.S).group(1)
    names = [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", decl.strip()).group(1) for stmt in body.split(";") for decl in stmt.split(",") if decl.strip()]
    assert names == [f[0] for f in _capi.NsrFrameDesc._fields_]
    (tmp_path / "t.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nsr.h"\nint main(){printf("%zu %zu %zu\\n", '
                                  'sizeof(nsr_frame_desc), offsetof(nsr_frame_desc, fx), offsetof(nsr_frame_desc, scale));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    out = subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()
    D = _capi.NsrFrameDesc
    assert [int(v) for v in out] == [C.sizeof(D), D.fx.offset, D.scale.offset]
