"""GPU tests of the PNG decoder (nice_slam_amd/csrc/nsr_png.h, nice_slam_amd/png.py): Pillow's pixels on the device for the filter
matrix, the output forms and the named paths through inflate (tests/test_png_emu.py asserts what each of them holds); batches and a
second call; sentinels and guard bytes; the damaged streams, which set their status and leave their neighbours alone; one
Replica-sized depth frame as Pillow saves it; the dataset readers."""
import numpy as np
import pytest
import torch

import png_reference as R
import test_png_emu as T
from nice_slam_amd import png
from nice_slam_amd.engine import gpu

pytestmark = pytest.mark.gpu


def decode(files, mode=None):
    out, status = png.decode_png_status(files, mode=mode)
    assert out.is_cuda
    return T.to_numpy(out), status


@pytest.mark.parametrize("kind", R.KINDS)
def test_device_equals_pillow_on_the_filter_matrix(kind):
    for size in T.SIZES:
        px = R.image(kind, *size, seed=2)
        files = [R.write_png(px, how, seed=5) for how in T.FILTERS]
        got, status = decode(files)
        assert status == [0] * len(files) and got.dtype == px.dtype
        for how, f, g in zip(T.FILTERS, files, got):
            assert np.array_equal(g, R.pil_pixels(f)), (size, how)


def test_output_forms():
    for kind in ("rgba8", "grey8", "rgb8"):
        f = R.write_png(R.image(kind, 13, 17, seed=4), "mix")
        assert np.array_equal(decode(f)[0][0], R.pil_pixels(f)) and np.array_equal(decode(f, "RGB")[0][0], R.pil_pixels(f, "RGB"))
    assert png.decode_png(R.write_png(R.image("grey16", 5, 5))).dtype == torch.uint16


@pytest.mark.parametrize("name", sorted(R.deflate_cases()))
def test_deflate_cases(name):
    data = R.deflate_cases()[name]
    got, status = decode(data)
    assert status == [0] and np.array_equal(got[0], R.pil_pixels(data))


def test_batch_equals_single_calls_and_a_second_call():
    files = T.batch_of_three()
    got, status = decode(files)
    assert status == [0, 0, 0]
    for k, f in enumerate(files):
        assert np.array_equal(got[k], decode(f)[0][0]) and np.array_equal(got[k], R.pil_pixels(f))
    assert np.array_equal(decode(files[::-1])[0], got[::-1])
    a, b = device_raw_decode(files, twice=True)
    assert np.array_equal(a, got) and np.array_equal(b, got)
    many = [R.write_png(R.image("grey16", 5, 7, seed=k), k % 5, level=k % 10) for k in range(65)]
    out, status = decode(many)
    assert status == [0] * 65 and all(np.array_equal(out[k], R.pil_pixels(many[k])) for k in range(65))


def device_raw_decode(files, out_channels=None, twice=False):
    """test_png_emu.raw_decode on the device"""
    return T.raw_decode(gpu(), files, out_channels, twice=twice)


def test_sentinels_and_guard_bytes():
    cases = R.deflate_cases()
    for files, oc in ((T.batch_of_three(), None), ([cases["stored"]] * 2, None), ([cases["full_flush"]], None),
                      ([R.write_png(R.image("rgba8", 70, 9, seed=1), "mix")], 3), ([R.write_png(R.image("grey8", 1, 1), 4)], 3),
                      ([cases["rle"]], None), ([R.write_png(R.image("rgb8", 130, 3, seed=2), "random")], None)):
        got, status = device_raw_decode(files, oc)
        assert status == [0] * len(files)
        for k, f in enumerate(files):
            assert np.array_equal(got[k], R.pil_pixels(f, "RGB" if oc == 3 else None))


def test_damaged_streams_set_their_status_only():
    """(the emulator's run of the same set comes first: tests/test_png_emu.py::test_damaged_streams_set_their_status_only; every
    fetch and store of the kernels is bounded by the stream's range and the frame's slice, and the guard bytes here show it)"""
    good, cases = R.damaged_cases()
    for name, (bad, bit) in sorted(cases.items()):
        first = R.write_png(R.image("grey16", 64, 64, seed=6), "mix", level=9) if name == "hlit_287" else good
        other = R.write_png(R.image("grey16", *R.pil_pixels(first).shape, seed=9), 4, level=1)
        got, status = device_raw_decode([first, bad, other])
        assert status[0] == 0 and status[1] & bit and status[2] == 0, (name, status)
        assert np.array_equal(got[0], R.pil_pixels(first)) and np.array_equal(got[2], R.pil_pixels(other)), name
    with pytest.raises(ValueError, match="frame 1 holds a damaged stream"):
        png.decode_png([good, cases["truncated"][0]])


def test_a_replica_sized_depth_frame():
    """680 x 1200, 16 bit, as Pillow saves it: eleven passes of 64 rows, a stream of more than one 64 KiB IDAT chunk"""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:680, 0:1200]
    depth = (1500 + 2 * y + x + 40 * np.sin(x / 37.0) * np.cos(y / 23.0) + rng.integers(0, 12, (680, 1200))).astype(np.uint16)
    data = R.pil_save(depth)
    assert data.count(b"IDAT") >= 2
    got, status = decode([data, data])
    assert status == [0, 0] and np.array_equal(got[0], depth) and np.array_equal(got[1], depth)


def test_datasets_with_the_gpu_png_decoder(tmp_path):
    T.check_datasets(tmp_path, None, "cuda:0")
