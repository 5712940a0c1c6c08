"""TEST INFRASTRUCTURE: the host restatement of the frame preparation (nice_slam_amd/csrc/nsr_frame.h), stage by stage after
the reference's BaseDataset.__getitem__ (src/utils/datasets.py:77-113), with the cases the emulator and the GPU tests share.

  stage 1  undistortion (:85-88)     numpy fp64, the continuous bilinear remap of the contract (cv2 is not used)
  stage 2  / 255 and resize (:90-94) numpy fp64; the resize is F.interpolate(mode='bilinear', align_corners=False) on fp64,
                                     which is cv2.resize(INTER_LINEAR)'s definition
  stage 3  depth (:92, :96)          numpy fp32 division, torch fp32 product, as the reference
  stage 4  crop_size (:97-104)       the reference's own two F.interpolate calls
  stage 5  crop_edge (:106-110)      slices
The colour is cast to fp32 at the end.

Gates (derived, none measured on the kernel):
  depth    bit-exact: the same two fp32 operations on the same pixel.
  colour   bit-exact on the identity path (no stage 1, no resize, no crop_size): (float)(u8 / 255.0) on both sides.
           Elsewhere |delta| <= 2^-23: both sides evaluate the same bilinear forms in fp64, possibly in another operation order,
           so they differ by a few 1e-16 before each is rounded ONCE to fp32; the values are <= 1, where one fp32 step is at
           most 2^-24 below 1 and 2^-23 is a full step at 1.  Anything looser is an indexing error.
  stage 1  the undistorted u8 image is equal outside the pixels the restatement flags as within 1e-9 of a rounding tie, and
           within one level on those; a case may flag at most 0.1 % of its pixels.
"""
import numpy as np
import torch
import torch.nn.functional as F

COLOR_TOL = 2.0 ** -23
TIE_EPS = 1e-9
MAX_TIE_FRACTION = 1e-3
TUM_DISTORTION = [0.2624, -0.9531, -0.0054, 0.0026, 1.1633]          # configs/TUM_RGBD/freiburg1_desk.yaml


def make_cfg(H, W, fx=40.0, fy=41.0, cx=None, cy=None, crop_size=None, crop_edge=0, distortion=None, png_depth_scale=6553.5, scale=1.0,
             dataset="replica", input_folder=""):
    cam = {"H": H, "W": W, "fx": fx, "fy": fy, "cx": (W - 1) / 2.0 + 0.3 if cx is None else cx, "cy": (H - 1) / 2.0 - 0.2 if cy is None else cy,
           "png_depth_scale": png_depth_scale, "crop_edge": crop_edge}
    if crop_size is not None:
        cam["crop_size"] = list(crop_size)
    if distortion is not None:
        cam["distortion"] = list(distortion)
    return {"dataset": dataset, "scale": scale, "cam": cam, "data": {"input_folder": input_folder}}


def make_frames(B, color_hw, depth_hw, seed=0, depth_f32=False):
    """smooth-plus-noise colour (u8 [B, Hc, Wc, 3]) and a depth image with holes (u16, or fp32 metres-like values)"""
    rng = np.random.default_rng(seed)
    Hc, Wc = color_hw
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    color = np.empty((B, Hc, Wc, 3), np.uint8)
    for k in range(B):
        for c in range(3):
            base = 128 + 90 * np.sin(0.21 * xx + 0.7 * c + k) * np.cos(0.17 * yy - 0.4 * c)
            color[k, ..., c] = np.clip(base + rng.normal(0, 12, (Hc, Wc)), 0, 255).astype(np.uint8)
    color[:, 0, 0] = (255, 0, 1)
    Hd, Wd = depth_hw
    if depth_f32:
        depth = rng.uniform(0.3, 9.0, (B, Hd, Wd)).astype(np.float32)
    else:
        depth = rng.integers(1, 65536, (B, Hd, Wd)).astype(np.uint16)
        depth[:, -1, -1] = 65535
    depth[rng.random((B, Hd, Wd)) < 0.1] = 0
    return color, depth


def guarded(a, device="cpu"):
    """the array as a tensor on ``device``: one contiguous block inside a larger allocation whose surroundings hold the largest
    value (255 / 65535): a read outside the block changes the output.  u16 travels as int16, the same bytes."""
    pad = 4096
    big = np.full(a.size + 2 * pad, 65535 if a.dtype != np.uint8 else 255, dtype=a.dtype)
    big[pad:pad + a.size] = a.reshape(-1)
    if big.dtype == np.uint16:
        big = big.view(np.int16)
    return torch.from_numpy(big).to(device)[pad:pad + a.size].view(a.shape)


# --------------------------------------------------------------------------------------------------
# the stages
# --------------------------------------------------------------------------------------------------
def undistort(img, fx, fy, cx, cy, dist):
    """(u8 [H, W, 3], ties bool [H, W]: some channel within TIE_EPS of a rounding tie, the number of taps outside the image)"""
    H, W = img.shape[:2]
    k1, k2, p1, p2, k3 = (float(v) for v in dist)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    rad = ((1.0 + k1 * r2) + k2 * (r2 * r2)) + k3 * ((r2 * r2) * r2)
    xd = (x * rad + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x)
    yd = (y * rad + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y
    sx, sy = fx * xd + cx, fy * yd + cy
    with np.errstate(invalid="ignore"):
        near = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)          # else all four taps are outside
    sx, sy = np.where(near, sx, -1.0), np.where(near, sy, -1.0)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = (sx - x0)[..., None], (sy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    padded = np.zeros((H + 2, W + 2, 3), np.float64)
    padded[1:-1, 1:-1] = img
    p00, p01 = padded[y0 + 1, x0 + 1], padded[y0 + 1, x0 + 2]
    p10, p11 = padded[y0 + 2, x0 + 1], padded[y0 + 2, x0 + 2]
    val = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11)
    val = np.where(near[..., None], val, 0.0)
    t = val + 0.5
    ties = (np.abs(t - np.round(t)) < TIE_EPS).any(-1)
    outside = 0
    for dy in (0, 1):
        for dx in (0, 1):
            outside += int(((y0 + dy < 0) | (y0 + dy >= H) | (x0 + dx < 0) | (x0 + dx >= W)).sum())
    return np.minimum(np.floor(t), 255).astype(np.uint8), ties, outside


def prepare(color_u8, depth_raw, cfg, bgr=False):
    """one frame through the five stages -> {"color" fp32 [H, W, 3], "depth" fp32 [H, W], and with distortion "undistorted" u8,
    "ties", "outside_taps"}"""
    cam = cfg["cam"]
    out = {}
    img = np.asarray(color_u8)
    if "distortion" in cam:                                                        # :85-88
        img, out["ties"], out["outside_taps"] = undistort(img, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["distortion"])
        out["undistorted"] = img
    if bgr:                                                                        # :90
        img = img[..., ::-1]
    color = img / 255.                                                             # :91
    depth = np.asarray(depth_raw).astype(np.float32) / np.float32(cam["png_depth_scale"])      # :92 (numpy keeps fp32 here)
    H, W = depth.shape
    color = torch.from_numpy(np.ascontiguousarray(color))
    if color.shape[:2] != (H, W):                                                  # :94, cv2.resize(color, (W, H)) INTER_LINEAR
        color = F.interpolate(color.permute(2, 0, 1)[None], (H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    depth = torch.from_numpy(depth) * cfg["scale"]                                 # :96
    if "crop_size" in cam:                                                         # :97-104
        color = color.permute(2, 0, 1)
        color = F.interpolate(color[None], list(cam["crop_size"]), mode="bilinear", align_corners=True)[0]
        depth = F.interpolate(depth[None, None], list(cam["crop_size"]), mode="nearest")[0, 0]
        color = color.permute(1, 2, 0).contiguous()
    edge = cam["crop_edge"]
    if edge > 0:                                                                   # :106-110
        color = color[edge:-edge, edge:-edge]
        depth = depth[edge:-edge, edge:-edge]
    assert color.dtype == torch.float64 and depth.dtype == torch.float32
    out["color64"] = color.contiguous().numpy()
    out["color"] = out["color64"].astype(np.float32)
    out["depth"] = depth.contiguous().numpy()
    return out


def update_cam(cfg):
    """NICE_SLAM.update_cam (NICE_SLAM.py:113-135) on the config's camera -> (H, W, fx, fy, cx, cy)"""
    cam = cfg["cam"]
    H, W, fx, fy, cx, cy = cam["H"], cam["W"], cam["fx"], cam["fy"], cam["cx"], cam["cy"]
    if "crop_size" in cam:
        crop_size = cam["crop_size"]
        sx = crop_size[1] / W
        sy = crop_size[0] / H
        fx = sx * fx
        fy = sy * fy
        cx = sx * cx
        cy = sy * cy
        W = crop_size[1]
        H = crop_size[0]
    if cam["crop_edge"] > 0:
        H -= cam["crop_edge"] * 2
        W -= cam["crop_edge"] * 2
        cx -= cam["crop_edge"]
        cy -= cam["crop_edge"]
    return H, W, fx, fy, cx, cy


# --------------------------------------------------------------------------------------------------
# the shared cases: name -> (B, colour size, depth size, make_cfg keywords, depth_f32, bgr)
# --------------------------------------------------------------------------------------------------
def _case(B, chw, dhw, depth_f32=False, bgr=True, **kw):
    return B, chw, dhw, kw, depth_f32, bgr


CASES = {
    "identity_24x40": _case(2, (24, 40), (24, 40), scale=0.7),
    "identity_w1": _case(1, (5, 1), (5, 1)),
    "identity_w5": _case(1, (3, 5), (3, 5), bgr=False),
    "identity_w41": _case(2, (4, 41), (4, 41)),
    "identity_edge_w41": _case(1, (9, 41), (9, 41), crop_edge=2, scale=0.7),
    "identity_f32_depth": _case(1, (6, 11), (6, 11), depth_f32=True, png_depth_scale=1.0, scale=0.7),
    "one_pixel": _case(1, (1, 1), (1, 1)),
    "color_larger_edge3": _case(1, (37, 53), (23, 31), crop_edge=3),
    "color_smaller": _case(1, (15, 20), (23, 31), bgr=False),
    "crop_down_edge2": _case(1, (30, 40), (30, 40), crop_size=(24, 32), crop_edge=2, scale=0.7),
    "crop_up": _case(1, (24, 32), (24, 32), crop_size=(30, 41)),
    "crop_to_one_row": _case(1, (12, 16), (12, 16), crop_size=(1, 7)),
    "f32_depth_crop": _case(1, (12, 16), (12, 16), depth_f32=True, crop_size=(9, 13), png_depth_scale=1.0, scale=0.7),
    "undistort_tum": _case(1, (37, 53), (37, 53), distortion=TUM_DISTORTION),
    "undistort_zero_border": _case(1, (24, 40), (24, 40), distortion=[0.4, 0.0, 0.0, 0.0, 0.0], fx=30.0, fy=30.0),
    "all_stages": _case(2, (37, 53), (30, 40), crop_size=(24, 32), crop_edge=2, distortion=TUM_DISTORTION, scale=0.5),
}
IDENTITY = tuple(k for k in CASES if k.startswith("identity") or k == "one_pixel")
# the real grid sizes (GPU only): a Replica frame, and a TUM frame through every stage
BIG_CASES = {
    "replica_680x1200": _case(1, (680, 1200), (680, 1200), png_depth_scale=6553.5),
    "tum_480x640": _case(1, (480, 640), (480, 640), crop_size=(384, 512), crop_edge=8, distortion=TUM_DISTORTION, fx=517.3, fy=516.5,
                         cx=318.6, cy=255.3, png_depth_scale=5000.0),
}


def build_case(name, seed=None):
    """(cfg, colour u8 [B, ...], depth [B, ...], bgr) of a case; the seed defaults to one derived from the name"""
    B, chw, dhw, kw, depth_f32, bgr = (CASES.get(name) or BIG_CASES[name])
    cfg = make_cfg(dhw[0], dhw[1], **kw)
    if "distortion" in cfg["cam"] and "cx" not in kw:                # the raw intrinsics belong to the colour image
        cfg["cam"]["cx"], cfg["cam"]["cy"] = (chw[1] - 1) / 2.0 + 0.3, (chw[0] - 1) / 2.0 - 0.2
    color, depth = make_frames(B, chw, dhw, seed=sum(map(ord, name)) if seed is None else seed, depth_f32=depth_f32)
    return cfg, color, depth, bgr


def check_case(name, cfg, color, depth, bgr, got_color, got_depth, got_undistorted=None):
    """hold a kernel's result for the case's frames to the restatement under the gates above"""
    got_color, got_depth = np.asarray(got_color), np.asarray(got_depth)
    assert got_color.dtype == np.float32 and got_depth.dtype == np.float32
    for k in range(color.shape[0]):
        ref = prepare(color[k], depth[k], cfg, bgr)
        assert got_depth[k].shape == ref["depth"].shape and got_color[k].shape == ref["color"].shape, (name, got_color[k].shape, ref["color"].shape)
        assert got_depth[k].tobytes() == ref["depth"].tobytes(), (name, k, "depth")
        if "undistorted" in ref:
            n_ties = int(ref["ties"].sum())
            assert n_ties <= MAX_TIE_FRACTION * ref["ties"].size, (name, k, n_ties)
            if got_undistorted is not None:
                diff = np.abs(got_undistorted[k].astype(np.int32) - ref["undistorted"].astype(np.int32)).max(-1)
                assert not diff[~ref["ties"]].any() and diff.max() <= 1, (name, k, int(diff.max()), int((diff > 0).sum()))
            if n_ties:                                   # a tie may have gone the other way: that pixel's level moves its footprint
                continue
        err = float(np.abs(got_color[k].astype(np.float64) - ref["color"].astype(np.float64)).max()) if ref["color"].size else 0.0
        print(f"{name}[{k}]: colour max |delta| = {err:.3e}")
        if name in IDENTITY or name.startswith("replica"):
            assert got_color[k].tobytes() == ref["color"].tobytes(), (name, k, "colour", err)
        else:
            assert err <= COLOR_TOL, (name, k, err)


# --------------------------------------------------------------------------------------------------
# tiny sequences on disk, in the layouts the reference's loaders read (datasets.py:116-231)
# --------------------------------------------------------------------------------------------------
def make_poses(n, seed=0):
    """n camera-to-world matrices (fp64) with a proper rotation and a translation"""
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(seed)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, :3] = Rotation.from_rotvec(rng.normal(0, 0.4, (n, 3))).as_matrix()
    poses[:, :3, 3] = rng.normal(0, 1.5, (n, 3))
    return poses


def write_sequence(layout, folder, colors, depths, poses, numbers=None):
    """write frames (colour u8 RGB [N, H, W, 3], depth u16 [N, H, W]) and poses [N, 4, 4] under ``folder`` as a 'replica',
    'scannet' or 'azure' sequence; ``numbers``: ScanNet's frame numbers (file names), default 0..N-1.  Colour files are JPEG
    or PNG as the layout's glob wants, so what a reader decodes is NOT ``colors``: compare against a second decode."""
    import os
    from PIL import Image
    n = len(colors)
    numbers = list(range(n)) if numbers is None else list(numbers)

    def rows(m):
        return "\n".join(" ".join(repr(float(v)) for v in r) for r in m)

    if layout == "replica":
        os.makedirs(os.path.join(folder, "results"))
        for i in range(n):
            Image.fromarray(colors[i]).save(os.path.join(folder, "results", f"frame{i:06d}.jpg"), quality=95)
            Image.fromarray(depths[i]).save(os.path.join(folder, "results", f"depth{i:06d}.png"))
        with open(os.path.join(folder, "traj.txt"), "w") as f:
            f.write("\n".join(" ".join(repr(float(v)) for v in m.reshape(-1)) for m in poses) + "\n")
    elif layout == "scannet":
        for sub in ("color", "depth", "pose"):
            os.makedirs(os.path.join(folder, "frames", sub))
        for i, num in enumerate(numbers):
            Image.fromarray(colors[i]).save(os.path.join(folder, "frames", "color", f"{num}.jpg"), quality=95)
            Image.fromarray(depths[i]).save(os.path.join(folder, "frames", "depth", f"{num}.png"))
            with open(os.path.join(folder, "frames", "pose", f"{num}.txt"), "w") as f:
                f.write(rows(poses[i]))
    elif layout == "azure":
        for sub in ("color", "depth"):
            os.makedirs(os.path.join(folder, sub))
        for i in range(n):
            Image.fromarray(colors[i]).save(os.path.join(folder, "color", f"{i:05d}.jpg"), quality=95)
            Image.fromarray(depths[i]).save(os.path.join(folder, "depth", f"{i:05d}.png"))
        if poses is not None:
            os.makedirs(os.path.join(folder, "scene"))
            with open(os.path.join(folder, "scene", "trajectory.log"), "w") as f:
                for i in range(n):
                    f.write(f"{i} {i} {i + 1}\n" + rows(poses[i]) + "\n")
    else:
        raise ValueError(layout)


# --------------------------------------------------------------------------------------------------
# driving the library (the emulator engine in the CPU tests, the product's on the GPU)
# --------------------------------------------------------------------------------------------------
def run_abi(E, cfg, color, depth, bgr):
    """nsr_frame_prepare on guarded copies of a batch, called directly with a workspace of the test's own -> (colour, depth,
    the workspace as u8 [B, Hc, Wc, 3] or None), host arrays"""
    import ctypes as C
    from nice_slam_amd.datasets import FramePreparer
    lib = E.lib
    prep = FramePreparer(cfg, engine=E)
    c, d = guarded(color, E.device), guarded(depth, E.device)
    B = c.shape[0]
    desc = prep.desc(c.shape[1:3], d.shape[1:3], d.dtype == torch.float32, bgr)
    H, W = C.c_int32(), C.c_int32()
    lib.check(lib.nsr_frame_out_size(C.byref(desc), C.byref(H), C.byref(W)), "nsr_frame_out_size")
    out_c = torch.full((B, H.value, W.value, 3), float("nan"), dtype=torch.float32, device=E.device)
    out_d = torch.full((B, H.value, W.value), float("nan"), dtype=torch.float32, device=E.device)
    nbytes = int(lib.nsr_frame_workspace_bytes(C.byref(desc), B))
    assert nbytes == (c.numel() if "distortion" in cfg["cam"] else 0)
    ws = torch.full((max(nbytes, 1),), 77, dtype=torch.uint8, device=E.device)
    with E.guard():
        lib.check(lib.nsr_frame_prepare(c.data_ptr(), d.data_ptr(), C.byref(desc), B, out_c.data_ptr(), out_d.data_ptr(),
                                        ws.data_ptr() if nbytes else None, nbytes, E.stream()), "nsr_frame_prepare")
    return out_c.cpu().numpy(), out_d.cpu().numpy(), ws.cpu().numpy().reshape(c.shape) if nbytes else None


def run_and_check(E, name):
    """a case through FramePreparer.prepare (guarded device inputs) and through the bare ABI: the same bits, and both within
    the gates"""
    from nice_slam_amd.datasets import FramePreparer
    cfg, color, depth, bgr = build_case(name)
    got_c, got_d = FramePreparer(cfg, engine=E).prepare(guarded(color, E.device), guarded(depth, E.device), bgr=bgr)
    abi_c, abi_d, und = run_abi(E, cfg, color, depth, bgr)
    got_c, got_d = got_c.cpu().numpy(), got_d.cpu().numpy()
    assert got_c.tobytes() == abi_c.tobytes() and got_d.tobytes() == abi_d.tobytes(), name
    assert ("distortion" in cfg["cam"]) == (und is not None)
    check_case(name, cfg, color, depth, bgr, got_c, got_d, und)
    return cfg, color, depth, bgr, got_c, got_d
