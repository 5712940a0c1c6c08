"""GPU tests of the JPEG encoder (nice_slam_amd/csrc/nsr_jpeg.h, nice_slam_amd/jpeg.py): the bytes of tests/jpeg_reference.py on the
device for every test image, both subsamplings and six qualities; a batch against single calls; the sizes at which the kernels go
round their loops again; the capacity of the size query with sentinels behind it; and the replay command with --encoder gpu
--video in a child process."""
import ctypes as C
import glob
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_reference as R
from nice_slam_amd import jpeg
from nice_slam_amd.engine import gpu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SUBS = ("4:2:0", "4:4:4")
IMAGES = R.image_set()


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_bytes_equal_the_restatement(name, sub):
    img = torch.from_numpy(IMAGES[name]).cuda()
    for q in R.QUALITIES:
        want = R.reference_file(name, q, sub)
        got = jpeg.encode_jpeg(img, q, sub)
        assert len(got) == 1 and got[0] == want, (name, sub, q)
        assert jpeg.encode_jpeg(img, q, sub)[0] == want                              # a second call
    with Image.open(io.BytesIO(got[0])) as im:
        im.load()
        assert im.size == (img.shape[1], img.shape[0])


@pytest.mark.parametrize("sub", SUBS)
def test_batch_of_three_equals_three_calls(sub):
    batch = R.batch_of_three()
    got = jpeg.encode_jpeg(batch, 75, sub)
    assert len(got) == 3
    for k in range(3):
        assert got[k] == jpeg.encode_jpeg(batch[k], 75, sub)[0] == R.encode(batch[k], 75, sub)
    assert jpeg.encode_jpeg(batch[::-1].copy(), 75, sub) == got[::-1]


@pytest.mark.parametrize("name", sorted(R.round_cases()))
def test_more_than_one_round_of_every_loop(name):
    batch, q, sub = R.round_cases()[name]
    got = jpeg.encode_jpeg(batch, q, sub)
    assert got == [R.encode(img, q, sub) for img in batch]
    assert jpeg.encode_jpeg(batch, q, sub) == got


def test_capacity_and_sentinels():
    E = gpu()
    img = torch.from_numpy(np.stack([R.noise_image(33, 47, seed=5), R.noise_image(33, 47, seed=6)])).cuda()
    nws, cap = jpeg.jpeg_size(2, 33, 47, "4:4:4")
    tail = 4096
    ws = torch.full((nws + tail,), 0xa5, dtype=torch.uint8, device="cuda")
    out = torch.full((cap + tail,), 0xa5, dtype=torch.uint8, device="cuda")
    offsets = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    E.call("nsr_jpeg_encode", img.data_ptr(), 2, 33, 47, 100, jpeg.SUBSAMPLING["4:4:4"], ws.data_ptr(), nws, out.data_ptr(), cap, offsets.data_ptr())
    off = offsets.cpu().tolist()
    used = off[-1]
    assert off[0] == 0 and off[1] > 0 and off[2] > off[1] and used <= cap
    host = out.cpu().numpy()
    assert (host[used:] == 0xa5).all()                                               # behind the used range and behind the capacity
    assert (ws[nws:].cpu().numpy() == 0xa5).all()
    for k in range(2):
        data = jpeg.jfif_header(33, 47, 100, "4:4:4") + host[off[k]:off[k + 1]].tobytes() + b"\xff\xd9"
        assert data == R.encode(img[k].cpu().numpy(), 100, "4:4:4")
    assert b"\xff\x00" in host[:used].tobytes()                                      # stuffing happened on the device


def test_replay_command_with_gpu_encoder_and_video(tmp_path):
    """the run directory of tests/test_hip_view.py::test_replay_command, replayed with --encoder gpu --video"""
    import raster_reference as RR
    from test_hip_view import room
    from nice_slam_amd.ply import write_ply
    out = tmp_path / "run"
    os.makedirs(out / "mesh")
    os.makedirs(out / "ckpts")
    rng = np.random.default_rng(9)
    for i, n in ((0, (10, 8, 6)), (6, (20, 16, 12))):
        v, f = room(n, (4, 3, 2))
        if i == 6:
            v = v * 1.1
        write_ply(str(out / "mesh" / f"{i:05d}_mesh.ply"), v, f, rng.integers(0, 256, (len(v), 3), dtype=np.uint8))
    n, scale = 12, 2.0
    est, gt = torch.zeros((n + 3, 4, 4)), torch.zeros((n + 3, 4, 4))
    for i in range(n):
        for lst, wob in ((est, 0.03 * np.sin(i)), (gt, 0.0)):
            m = RR.look_from([0.8 + 0.25 * i, 2.0 + wob, 1.4], [5.0, 2.0 + wob, 1.4])
            m[:3, 1] *= -1
            m[:3, 2] *= -1
            m[:3, 3] *= scale
            lst[i] = torch.from_numpy(m).float()
    torch.save({"estimate_c2w_list": est, "gt_c2w_list": gt, "idx": n - 1}, str(out / "ckpts" / "00011.tar"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "nice_slam_amd.viewer", "--output", str(out), "--scale", str(scale),
                          "--encoder", "gpu", "--video"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "vis.avi" in res.stdout and "ffmpeg" not in res.stdout
    files = sorted(glob.glob(str(out / "tmp_rendering" / "*.jpg")))
    assert [os.path.basename(p) for p in files] == [f"{k:06d}.jpg" for k in range(1, n + 1)]
    streams = [open(p, "rb").read() for p in files]
    riff = R.walk_avi((out / "vis.avi").read_bytes())
    movi = R.find(riff, b"LIST", b"movi")
    assert [c["id"] for c in movi["children"]] == [b"00dc"] * n
    assert [c["data"] for c in movi["children"]] == streams
    imgs = []
    for s in streams:
        with Image.open(io.BytesIO(s)) as im:
            assert im.size == (960, 540) and im.mode == "RGB"
            imgs.append(np.asarray(im).astype(np.int32))
    assert (imgs[0] < 250).mean() > 0.05                                             # a mesh is on the picture
    step = [float(np.abs(a - b).mean()) for a, b in zip(imgs[:-1], imgs[1:])]
    assert step[5] > 5 * max(step[:5] + step[6:]) and step[5] > 1.0                  # the second mesh arrives with frame 6
