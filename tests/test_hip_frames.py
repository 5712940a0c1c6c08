"""GPU tests of the frame preparation (nice_slam_amd/csrc/nsr_frame.h) and the sequence readers (nice_slam_amd/datasets.py): the
emulator test's cases on the product library under the same gates (tests/frames_reference.py), the unmodified reference's
frames (tests/golden/frames.npz), one Replica-sized and one TUM-sized frame so that real grid sizes run, device tensors in
stream order without a host synchronisation, and a folder read end to end."""
import json
import os

import numpy as np
import pytest
import torch

import frames_reference as R
from conftest import GOLDEN
from nice_slam_amd import get_dataset
from nice_slam_amd.datasets import FramePreparer
from nice_slam_amd.engine import gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "frames.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(R.CASES) + list(R.BIG_CASES))
def test_case_matches_restatement(name):
    R.run_and_check(gpu(), name)


@pytest.mark.parametrize("layout", ["replica", "scannet", "azure"])
def test_golden_frames(gold, layout):
    cfg = json.loads(str(gold[f"{layout}/cfg"]))
    raw_c, raw_d = gold[f"{layout}/raw_color"], gold[f"{layout}/raw_depth"]
    want_c, want_d = gold[f"{layout}/color"].astype(np.float32), gold[f"{layout}/depth"]
    got_c, got_d = FramePreparer(cfg).prepare(R.guarded(raw_c, "cuda"), R.guarded(raw_d, "cuda"), bgr=False)
    assert got_c.is_cuda and got_d.is_cuda and got_c.dtype == torch.float32 and got_d.dtype == torch.float32
    got_c, got_d = got_c.cpu().numpy(), got_d.cpu().numpy()
    assert got_d.tobytes() == want_d.tobytes()
    if "crop_size" in cfg["cam"]:
        assert np.abs(got_c.astype(np.float64) - want_c).max() <= R.COLOR_TOL
    else:
        assert got_c.tobytes() == want_c.tobytes()


def test_batch_frames_equal_single_frames_and_empty_batch():
    cfg, color, depth, bgr = R.build_case("all_stages")
    color, depth = np.concatenate([color, color[:1]]), np.concatenate([depth, depth[:1]])
    prep = FramePreparer(cfg)
    bc, bd = prep.prepare(color, depth, bgr=bgr)
    for k in range(3):
        c1, d1 = prep.prepare(color[k], depth[k], bgr=bgr)
        assert torch.equal(c1, bc[k]) and torch.equal(d1, bd[k])
    ec, ed = prep.prepare(color[:0], depth[:0], bgr=bgr)
    assert tuple(ec.shape) == (0,) + tuple(bc.shape[1:]) and tuple(ed.shape) == (0,) + tuple(bd.shape[1:])


def test_device_tensors_in_stream_order_without_a_host_sync():
    cfg, color, depth, bgr = R.build_case("all_stages")
    prep = FramePreparer(cfg)
    want_c, want_d = prep.prepare(color, depth, bgr=bgr)
    again_c, again_d = prep.prepare(color, depth, bgr=bgr)
    assert torch.equal(want_c, again_c) and torch.equal(want_d, again_d)            # a second call: the same bits
    c0, d0 = torch.from_numpy(color).cuda(), torch.from_numpy(depth.view(np.int16)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.cuda.stream(side):
            c, d = c0 ^ 0x5A, d0 ^ 0x0F0F                                          # the inputs exist only after work on this stream
            for _ in range(40):
                c, d = c ^ 0x33, d ^ 0x1111
            c, d = c ^ 0x5A, d ^ 0x0F0F
            got_c, got_d = prep.prepare(c, d, bgr=bgr)
            got_c, got_d = got_c + 0.0, got_d + 0.0                                # ... and the outputs are read on it at once
    finally:
        torch.cuda.set_sync_debug_mode("default")
    side.synchronize()
    assert torch.equal(got_c, want_c) and torch.equal(got_d, want_d)


def test_folder_end_to_end(gold, tmp_path):
    layout = "scannet"
    n = len(gold[f"{layout}/raw_color"])
    H, W = gold[f"{layout}/raw_color"].shape[1:3]
    colors, depths = R.make_frames(n, (H, W), (H, W), seed=len(layout))
    R.write_sequence(layout, str(tmp_path / layout), colors, depths, R.make_poses(n, seed=len(layout)), [0, 1, 2, 9, 10])
    cfg = json.loads(str(gold[f"{layout}/cfg"]))
    cfg["data"]["input_folder"] = str(tmp_path / layout)
    ds = get_dataset(cfg, device="cuda:0")
    assert len(ds) == n and ds.camera == R.update_cam(cfg)
    for i in range(n):
        idx, color, depth, c2w = ds[i]
        assert idx == i and color.is_cuda and depth.is_cuda and c2w.is_cuda and tuple(color.shape[:2]) == ds.camera[:2]
        raw_c, raw_d = ds.read_raw(i)
        ref = R.prepare(raw_c, raw_d, cfg, bgr=False)
        assert color.cpu().numpy().tobytes() == ref["color"].tobytes()              # crop_edge only: the identity path
        assert depth.cpu().numpy().tobytes() == ref["depth"].tobytes() == gold[f"{layout}/depth"][i].tobytes()
        assert c2w.cpu().numpy().tobytes() == gold[f"{layout}/pose"][i].tobytes()
    idx, color, depth, c2w = ds.load_batch([4, 1])
    assert torch.equal(color[0], ds[4][1]) and torch.equal(depth[1], ds[1][2]) and torch.equal(c2w[0], ds[4][3])
