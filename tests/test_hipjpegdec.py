"""GPU tests of the JPEG decoder (nice_slam_amd/csrc/nsr_jpegdec.h, nice_slam_amd/jpeg.py): the pixels of tests/jpegdec_reference.py
on the device for the small sizes, the four samplings, both subsequence sizes and the named synchronisation cases; the golden
file's pixels; batches and a second call; sentinels; one file of more than three tiles at the default subsequence size; the round
trip through ``encode_jpeg``; the dataset readers; ``MjpegReader`` on a vis.avi written by the replay command in a child process;
a truncated stream inside a guard-filled allocation."""
import numpy as np
import pytest
import torch

import jpeg_reference as R
import jpegdec_reference as D
import test_jpegdec_emu as T
from nice_slam_amd import jpeg
from nice_slam_amd.engine import gpu

pytestmark = pytest.mark.gpu


def decode(files, sb=128):
    out, status = jpeg.decode_jpeg_status(files, subsequence_bytes=sb)
    assert out.is_cuda
    return out.cpu().numpy(), status


@pytest.mark.parametrize("sb", (16, 128))
@pytest.mark.parametrize("sampling", D.SAMPLINGS)
def test_device_equals_restatement(sampling, sb):
    """every small size at this sampling; content, quality, tables and restart setting rotate through the sizes (small_cases)"""
    for size in D.SIZES:
        cases = [c for c in D.small_cases() if c[1] == size and c[2] == sampling]
        assert len(cases) == 4 and {c[5] for c in cases} == {0, 1, 2, 3}
        files = [D.case_file(*c) for c in cases]
        got, status = decode(files, sb)                              # one call per size: own tables and stream length per file
        assert status == [0] * len(files)
        for k, case in enumerate(cases):
            assert np.array_equal(got[k], D.reference(files[k])[0]), case


@pytest.mark.parametrize("name", sorted(T.sync_cases()))
def test_sync_cases(name):
    data, sb = T.sync_cases()[name]
    want = D.reference(data)[0]
    for s in (sb, 128 if sb == 16 else 16):
        got, status = decode(data, s)
        assert status == [0] and np.array_equal(got[0], want), s


def test_golden_pixels():
    for name in T.GOLDEN_NAMES:
        data = T.GOLDEN[name + ".jpg"].tobytes()
        if name.startswith("refused"):
            with pytest.raises(ValueError, match="not supported"):
                jpeg.decode_jpeg(data)
            continue
        for sb in (16, 128, 1024):
            got, status = decode(data, sb)
            assert status == [0] and np.array_equal(got[0], T.GOLDEN[name + ".rgb"]), (name, sb)


def test_batch_equals_single_calls_and_a_second_call():
    files = T.batch_of_three()
    got, status = decode(files)
    assert status == [0, 0, 0]
    for k, f in enumerate(files):
        assert np.array_equal(got[k], decode(f)[0][0]) and np.array_equal(got[k], D.reference(f)[0])
    assert np.array_equal(decode(files[::-1])[0], got[::-1])
    assert np.array_equal(decode(files)[0], got)
    many = [D.pil_file(D.noise_image(8, 8, seed=200 + k), quality=75) for k in range(257)]
    out, status = decode(many)
    assert status == [0] * 257 and all(np.array_equal(out[k], D.decode(many[k])[0]) for k in (0, 1, 255, 256))


def device_raw_decode(files, sb=128, tail=4096, guard=512):
    """test_jpegdec_emu.raw_decode on the device: the files between guard bytes of 0xFF in one allocation, sentinels behind the
    workspace and the output"""
    E = gpu()
    parsed = [jpeg._parse(f) for f in files]
    H, W, sampling = parsed[0]["height"], parsed[0]["width"], parsed[0]["sampling"]
    blob = b"".join(b"\xff" * guard + f for f in files) + b"\xff" * guard
    offsets = np.cumsum([0] + [guard + len(f) for f in files])[:-1] + guard
    desc = torch.from_numpy(jpeg._descriptors(parsed, offsets).view(np.uint8).reshape(-1)).cuda()
    buf = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
    n = len(files)
    nws = jpeg.jpegdec_size(n, H, W, sampling, max(map(len, files)), sb)
    ws = torch.full((nws + tail,), 0xa5, dtype=torch.uint8, device="cuda")
    out = torch.full((n * H * W * 3 + tail,), 0xa5, dtype=torch.uint8, device="cuda")
    status = torch.full((n + 4,), -7, dtype=torch.int32, device="cuda")
    E.call("nsr_jpegdec_decode", buf.data_ptr(), desc.data_ptr(), n, H, W, jpeg.SAMPLING[sampling], sb, ws.data_ptr(), nws, out.data_ptr(),
           status.data_ptr())
    assert (ws[nws:] == 0xa5).all() and (out[n * H * W * 3:] == 0xa5).all() and (status[n:] == -7).all()
    return out[:n * H * W * 3].reshape(n, H, W, 3).cpu().numpy(), status[:n].cpu().tolist()


def test_sentinels_and_guard_bytes():
    for files, sb in ((T.batch_of_three(), 128), ([T.sync_cases()["noise_split_pair"][0]], 16), ([D.case_file("recipe", (1, 1), "grey", 90)], 1024)):
        got, status = device_raw_decode(files, sb)
        assert status == [0] * len(files)
        for k, f in enumerate(files):
            assert np.array_equal(got[k], D.reference(f)[0])


def test_more_than_three_tiles_at_the_default_size():
    data = D.pil_file(D.noise_image(320, 320, seed=7), quality=100, subsampling="4:4:4")
    assert D.chain_lengths(data)[0] > 3 * 1024 * 128                      # (a tile is 1024 subsequences of 128 bytes)
    got, status = decode(data)
    assert status == [0] and np.array_equal(got[0], D.pil_pixels(data))
    small = D.pil_file(D.noise_image(160, 160, seed=7), quality=100, subsampling="4:4:4")      # the issue's file: a tile's worth
    got, status = decode(small)
    assert status == [0] and np.array_equal(got[0], D.pil_pixels(small))


def test_round_trip_through_the_encoder():
    images = R.image_set()
    for sub in ("4:2:0", "4:4:4"):
        for name in ("recipe100x150", "noise33x47", "small1x1", "small17x23"):
            data, = jpeg.encode_jpeg(torch.from_numpy(images[name]).cuda(), 90, sub)
            assert data == R.reference_file(name, 90, sub)
            got, status = decode(data)
            assert status == [0] and np.array_equal(got[0], D.pil_pixels(data)), (name, sub)


def test_datasets_with_the_gpu_decoder(tmp_path):
    T.check_datasets(tmp_path, None, "cuda:0")


def test_mjpeg_reader_on_the_replay_commands_video(tmp_path):
    """vis.avi of ``python -m nice_slam_amd.viewer --encoder gpu --video`` (a child process) read back: the files of
    tmp_rendering/, and Pillow's pixels of them"""
    import glob

    from test_hip_jpeg import test_replay_command_with_gpu_encoder_and_video as replay
    replay(tmp_path)
    files = [open(p, "rb").read() for p in sorted(glob.glob(str(tmp_path / "run" / "tmp_rendering" / "*.jpg")))]
    with jpeg.MjpegReader(str(tmp_path / "run" / "vis.avi")) as video:
        assert len(video) == len(files) == 12 and (video.width, video.height) == (960, 540)
        assert [video.frame_bytes(i) for i in range(12)] == files
        frames = video.read()
    assert frames.is_cuda and frames.shape == (12, 540, 960, 3)
    for k in (0, 5, 6, 11):
        assert np.array_equal(frames[k].cpu().numpy(), D.pil_pixels(files[k])), k


def test_truncated_stream_sets_its_status_only():
    """(the emulator's damaged-stream cases come first: tests/test_jpegdec_emu.py::test_damaged_streams_set_their_status_only)"""
    good, cut, _ = T.damaged()
    other = D.case_file("noise", (33, 49), "4:2:0", 100)
    got, status = device_raw_decode([good, cut, other], 128)
    assert status[0] == 0 and status[1] != 0 and status[2] == 0
    assert np.array_equal(got[0], D.reference(good)[0]) and np.array_equal(got[2], D.reference(other)[0])
    with pytest.raises(ValueError, match="frame 1"):
        jpeg.decode_jpeg([good, cut])
