"""CPU tests of the PNG decoder (nice_slam_amd/csrc/nsr_png.h, nice_slam_amd/png.py): the kernel sources on the emulator against
live Pillow, with zero differing pixels, on files written by hand (tests/png_reference.py) -- the filter matrix, the output forms,
the paths through inflate, each with the property it is there for asserted from the restatement's record; batches; sentinels and
guards; damaged streams and refusals; the C ABI's errors; the dataset readers with ``png_decoder="gpu"``."""
import ctypes as C
import os
import re
import shutil
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import emu_harness
import png_reference as R
from nice_slam_amd import _capi, datasets, png
from nice_slam_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((13, 17), (1, 1), (1, 300), (70, 9), (130, 3))       # 70: one hand-over between passes of 64 rows; 130: two
FILTERS = (0, 1, 2, 3, 4, "mix", "random")


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


@pytest.fixture(scope="module")
def deflate_cases():
    return R.deflate_cases()


def to_numpy(t: torch.Tensor) -> np.ndarray:
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.uint16 else t.numpy()


def decode(E, files, mode=None):
    out, status = png.decode_png_status(files, mode=mode, engine=E)
    return to_numpy(out), status


def lut_bits() -> int:
    with open(os.path.join(HERE, "..", "nice_slam_amd", "csrc", "nsr_png.h")) as fh:
        return int(re.search(r"constexpr int kPngLutBits = (\d+);", fh.read()).group(1))


# ---- 1. the restatement and the writer -----------------------------------------------------------------------------------------------
def test_restatement_equals_zlib_and_writer_equals_pillow(deflate_cases):
    for name, data in deflate_cases.items():
        stream = R.zlib_stream(data)
        assert R.inflate(stream)[0] == zlib.decompress(stream), name
        assert png.probe_png(data)["supported"], name
    for kind in R.KINDS:
        for size in SIZES:
            px = R.image(kind, *size, seed=1)
            for how in FILTERS:
                assert np.array_equal(R.pil_pixels(R.write_png(px, how, seed=3)), px), (kind, size, how)


# ---- 2. filters and output forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_filters(E, size, kind):
    px = R.image(kind, *size, seed=2)
    files = [R.write_png(px, how, seed=5) for how in FILTERS]
    for how, f in zip(FILTERS, files):                             # the case holds the filter it is named for
        rows = zlib.decompress(R.zlib_stream(f))
        types = set(rows[::1 + size[1] * R.BPP[kind]])
        assert types == ({how} if isinstance(how, int) else types) and (isinstance(how, int) or len(types) > 1 or size[0] == 1), how
    got, status = decode(E, files)                                 # one call for the seven files
    assert status == [0] * len(files) and got.dtype == px.dtype and got.shape[1:] == px.shape
    for how, f, g in zip(FILTERS, files, got):
        assert np.array_equal(g, R.pil_pixels(f)) and np.array_equal(g, px), how


def test_output_forms(E):
    for kind in ("rgba8", "grey8", "rgb8"):
        px = R.image(kind, 13, 17, seed=4)
        f = R.write_png(px, "mix")
        assert np.array_equal(decode(E, f)[0][0], R.pil_pixels(f))                      # alpha kept, grey once
        rgb = decode(E, f, "RGB")[0][0]
        assert rgb.shape == (13, 17, 3) and np.array_equal(rgb, R.pil_pixels(f, "RGB"))   # alpha dropped, grey three times
    with pytest.raises(ValueError, match="16-bit"):
        png.decode_png(R.write_png(R.image("grey16", 5, 5)), mode="RGB", engine=E)
    with pytest.raises(ValueError, match="mode"):
        png.decode_png(R.write_png(R.image("grey8", 5, 5)), mode="L", engine=E)
    assert png.decode_png(R.write_png(R.image("grey16", 5, 5)), engine=E).dtype == torch.uint16


# ---- 3. the paths through inflate ----------------------------------------------------------------------------------------------------
def test_deflate_cases_have_their_property(deflate_cases):
    rec = {name: R.inflate(R.zlib_stream(data))[1] for name, data in deflate_cases.items()}
    assert rec["stored"]["blocks"] == [0]
    assert rec["stored_two_blocks"]["blocks"] == [0, 0]
    assert struct.unpack("<H", R.zlib_stream(deflate_cases["stored_two_blocks"])[3:5])[0] > 65000     # the first block is a full one
    assert rec["fixed"]["blocks"] == [1] and rec["fixed"]["largest_length"] >= 3
    assert rec["dynamic"]["blocks"] == [2] and rec["dynamic"]["largest_length"] >= 3
    assert rec["huffman_only"]["blocks"] == [2] and rec["huffman_only"]["largest_length"] == 0
    assert rec["single_distance_code"]["single_dist_code"] and rec["single_distance_code"]["largest_distance"] == 1
    assert rec["rle"]["largest_distance"] == 1 and rec["rle"]["overlapped"] and rec["rle"]["largest_length"] == 258
    assert rec["full_flush"]["empty_stored"] >= 5 and len(rec["full_flush"]["blocks"]) >= 10
    assert rec["fixed_flushed"]["blocks"].count(1) >= 5 and 2 not in rec["fixed_flushed"]["blocks"]      # the fixed tables are built once
    assert deflate_cases["idat_7"].count(b"IDAT") >= 30
    assert 32000 < rec["window_end"]["largest_distance"] <= 32768
    assert rec["long_codes"]["longest_litlen_code"] > lut_bits() and lut_bits() >= 9      # (a fixed block's codes fit the table)
    assert rec["pil_saved"]["blocks"] == [2]
    assert rec["fixed"]["overlapped"] or rec["dynamic"]["overlapped"]


@pytest.mark.parametrize("name", sorted(R.deflate_cases()))
def test_deflate_cases(E, deflate_cases, name):
    data = deflate_cases[name]
    got, status = decode(E, data)
    assert status == [0] and np.array_equal(got[0], R.pil_pixels(data))


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------
def batch_of_three():
    return [R.write_png(R.image("grey16", 34, 50, seed=k), how, level=lvl) for k, (how, lvl) in enumerate((("mix", 9), (4, 0), ("random", 1)))]


def test_batch_equals_single_calls(E):
    files = batch_of_three()
    got, status = decode(E, files)
    assert status == [0, 0, 0]
    for k, f in enumerate(files):
        one, st = decode(E, f)
        assert st == [0] and np.array_equal(one[0], got[k]) and np.array_equal(one[0], R.pil_pixels(f))
    a, b = raw_decode(E, files, twice=True)
    assert np.array_equal(a, got)


def test_batch_of_65(E):
    files = [R.write_png(R.image("grey16", 5, 7, seed=k), k % 5, level=k % 10) for k in range(65)]
    got, status = decode(E, files)
    assert status == [0] * 65
    for k, f in enumerate(files):
        assert np.array_equal(got[k], R.pil_pixels(f)), k


def test_mixed_sizes_raise(E):
    a, b, c = R.write_png(R.image("grey16", 5, 7)), R.write_png(R.image("grey16", 7, 5)), R.write_png(R.image("grey8", 5, 7))
    with pytest.raises(ValueError, match="frame 1 is 7 x 5"):
        png.decode_png([a, b], engine=E)
    with pytest.raises(ValueError, match="frame 1 is 5 x 7 grey8"):
        png.decode_png([a, c], engine=E)
    out, status = png.decode_png_status([], engine=E)
    assert out.shape[0] == 0 and status == []


# ---- 5. sentinels and guards -------------------------------------------------------------------------------------------------------
def raw_decode(E, files, out_channels=None, tail=4096, guard=512, twice=False):
    """The C ABI on buffers of the engine's device (host memory under the emulator, device memory in tests/test_hip_png.py): every
    stream sits between `guard` bytes of 0xFF, sentinels stand before and behind the workspace, the output and the status.  Returns
    (pixels, status); with `twice`, the pixels of a second call on the same workspace instead of the status."""
    parsed = [png.parse_png(f) for f in files]
    H, W, kind = parsed[0]["height"], parsed[0]["width"], parsed[0]["kind"]
    oc = png.CHANNELS[kind] if out_channels is None else out_channels
    blob, desc = png.pack_streams(parsed, gap=guard)
    blob = np.frombuffer(blob, np.uint8).copy()
    assert all(blob[d["stream_begin"] - 1] == 0xff and blob[d["stream_end"]] == 0xff for d in desc)
    buf, dev_desc = torch.from_numpy(blob).to(E.device), torch.from_numpy(desc.view(np.uint8).reshape(-1).copy()).to(E.device)
    n, nws = len(files), png.png_size(len(files), H, W, kind, E)
    assert nws >= n * H * (1 + W * R.BPP[kind])
    nout = n * H * W * oc * (2 if kind == "grey16" else 1)
    ws = torch.full((nws + 2 * tail,), 0xa5, dtype=torch.uint8, device=E.device)
    out = torch.full((nout + 2 * tail,), 0xa5, dtype=torch.uint8, device=E.device)
    status = torch.full((n + 8,), -7, dtype=torch.int32, device=E.device)
    assert ws.data_ptr() % 16 == 0 and tail % 16 == 0

    def call():
        with E.guard():
            E.call("nsr_png_decode", buf.data_ptr(), dev_desc.data_ptr(), n, H, W, png.KIND[kind], oc, ws[tail:].data_ptr(), nws,
                   out[tail:].data_ptr(), status[4:].data_ptr())
        assert (ws[:tail] == 0xa5).all() and (ws[tail + nws:] == 0xa5).all()
        assert (out[:tail] == 0xa5).all() and (out[tail + nout:] == 0xa5).all()
        assert (status[:4] == -7).all() and (status[4 + n:] == -7).all() and np.array_equal(buf.cpu().numpy(), blob)
        px = out[tail:tail + nout].cpu().numpy().copy()
        px = px.view(np.uint16) if kind == "grey16" else px
        return px.reshape((n, H, W) + ((oc,) if oc > 1 else ()))

    first = call()
    if twice:
        second = call()
        assert np.array_equal(first, second)
        return first, second
    return first, status[4:4 + n].cpu().tolist()


def test_sentinels_and_guard_bytes(E, deflate_cases):
    for files, oc in ((batch_of_three(), None), ([deflate_cases["stored"]] * 2, None), ([deflate_cases["full_flush"]], None),
                      ([R.write_png(R.image("rgba8", 70, 9, seed=1), "mix")], 3), ([R.write_png(R.image("grey8", 1, 1), 4)], 3),
                      ([deflate_cases["rle"]], None), ([R.write_png(R.image("rgb8", 130, 3, seed=2), "random")], None)):
        got, status = raw_decode(E, files, oc)
        assert status == [0] * len(files)
        for k, f in enumerate(files):                              # a read outside a stream would have met 0xFF, not the file
            assert np.array_equal(got[k], R.pil_pixels(f, "RGB" if oc == 3 else None))


# ---- 6. damaged streams, refusals --------------------------------------------------------------------------------------------------
def test_damaged_cases_are_what_they_claim():
    good, cases = R.damaged_cases()
    assert R.inflate(R.zlib_stream(R.write_png(R.image("grey16", 64, 64, seed=6), "mix", level=9)))[1]["blocks"][0] == 2
    for name, (data, bit) in cases.items():
        H, W = png.probe_png(data)["height"], png.probe_png(data)["width"]
        assert png.probe_png(data)["supported"], name              # the host parser takes the file: the device has to find it
        try:
            rows = zlib.decompress(R.zlib_stream(data))
        except zlib.error:
            continue
        wrong_length = len(rows) != H * (1 + 2 * W)
        bad_filter = not wrong_length and max(rows[::1 + 2 * W]) > 4
        assert wrong_length or bad_filter, name


@pytest.mark.parametrize("name", sorted(R.damaged_cases()[1]))
def test_damaged_streams_set_their_status_only(E, name):
    good, cases = R.damaged_cases()
    bad, bit = cases[name]
    if name == "hlit_287":                                         # (a 64 x 64 file: its neighbours have its size)
        good = R.write_png(R.image("grey16", 64, 64, seed=6), "mix", level=9)
    other = R.write_png(R.image("grey16", *R.pil_pixels(good).shape, seed=9), 4, level=1)
    got, status = raw_decode(E, [good, bad, other])            # (asserts the guard bytes)
    assert status[0] == 0 and status[1] & bit and status[2] == 0, status
    assert np.array_equal(got[0], R.pil_pixels(good)) and np.array_equal(got[2], R.pil_pixels(other))
    with pytest.raises(ValueError, match="frame 1 holds a damaged stream"):
        png.decode_png([good, bad], engine=E)


def refused_cases():
    """{name: (file, a word of the reason)}"""
    def saved(im, **kw):
        import io
        buf = io.BytesIO()
        im.save(buf, "PNG", **kw)
        return buf.getvalue()

    rgb = Image.fromarray(R.image("rgb8", 9, 11, seed=1))
    good = R.write_png(R.image("rgb8", 9, 11, seed=1), "mix")
    adam7 = bytearray(good)
    adam7[28] = 1                                                  # IHDR's interlace byte, and the chunk's CRC
    adam7[29:33] = struct.pack(">I", zlib.crc32(bytes(adam7[12:29])))
    bad_crc = bytearray(good)
    bad_crc[-20] ^= 1                                              # a byte of the IDAT payload
    stream = R.zlib_stream(good)
    return {"palette": (saved(rgb.quantize(16)), "palette"),
            "grey_alpha": (saved(rgb.convert("LA")), "grey + alpha"),
            "bit_depth_4": (R.png_file(9, 11, "grey8", zlib.compress(bytes(9 * 7)), depth=4), "bit depth 4"),
            "rgb16": (R.png_file(9, 11, "rgb8", zlib.compress(bytes(9 * 67)), depth=16), "16-bit colour"),
            "adam7": (bytes(adam7), "Adam7"),
            "trns": (R.png_file(9, 11, "rgb8", stream, extra=[(b"tRNS", bytes(6))]), "tRNS"),
            "apng": (R.png_file(9, 11, "rgb8", stream, extra=[(b"acTL", struct.pack(">II", 1, 0))]), "acTL"),
            "bad_crc": (bytes(bad_crc), "CRC"),
            "no_idat": (good[:33] + R.chunk(b"IEND", b""), "no IDAT"),
            "split_idat": (R.png_file(9, 11, "rgb8", stream[:20]) [:-12] + R.chunk(b"tEXt", b"k\0v") + R.chunk(b"IDAT", stream[20:]) + R.chunk(b"IEND", b""),
                           "not consecutive"),
            "no_iend": (good[:-12], "no IEND"),
            "not_png": (b"\xff\xd8\xff\xe0" + bytes(40), "not a PNG")}, good


def test_refusals(E):
    cases, good = refused_cases()
    for name, (bad, word) in cases.items():
        info = png.probe_png(bad)
        assert not info["supported"] and word in info["reason"], (name, info)
        with pytest.raises(ValueError, match="frame 0 is not supported"):
            png.decode_png(bad, engine=E)
        with pytest.raises(ValueError, match="frame 1 is not supported"):
            png.decode_png([good, bad], engine=E)
    for name in ("palette", "grey_alpha", "trns"):                 # files Pillow itself reads: refused here, not damaged
        Image.open(__import__("io").BytesIO(cases[name][0])).load()
    assert png.probe_png(good) == {"height": 9, "width": 11, "kind": "rgb8", "supported": True, "reason": None}
    assert png.probe_png(cases["palette"][0])["height"] == 9


def test_command_line(tmp_path, capsys):
    cases, good = refused_cases()
    for name, data in (("good.png", good), ("palette.png", cases["palette"][0])):
        with open(tmp_path / name, "wb") as fh:
            fh.write(data)
    assert png._main([str(tmp_path / "good.png"), str(tmp_path / "palette.png")]) == 0
    text = capsys.readouterr().out.splitlines()
    assert "9 x 11 rgb8: supported" in text[0] and "refused: a palette image" in text[1]


# ---- 7. the C ABI's errors ---------------------------------------------------------------------------------------------------------
def check_abi_errors(lib):
    data = R.write_png(R.image("rgba8", 16, 16, seed=1), "mix")
    stream = R.zlib_stream(data)
    nws = C.c_int64(-7)
    assert lib.nsr_png_size(1, 16, 16, 3, C.byref(nws)) == 0 and nws.value >= 16 * 65
    for args in ((1, 0, 16, 3), (1, 16, 32769, 3), (1, 16, 16, 4), (1, 16, 16, -1), (-1, 16, 16, 3), (65536, 16, 16, 3), (65535, 32768, 32768, 3)):
        a = C.c_int64(-7)
        assert lib.nsr_png_size(*args, C.byref(a)) != 0 and lib.nsr_last_error() and a.value == -7, args
    assert lib.nsr_png_size(1, 16, 16, 3, None) != 0 and b"null" in lib.nsr_last_error()
    big, zero = C.c_int64(0), C.c_int64(-7)
    assert lib.nsr_png_size(1, 32768, 32768, 3, C.byref(big)) == 0 and big.value >= 32768 * (1 + 4 * 32768)
    assert lib.nsr_png_size(0, 16, 16, 3, C.byref(zero)) == 0 and zero.value == 0
    ws = np.full(nws.value + 32, 0xa5, np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:][:nws.value + 16]
    out, status = np.full(16 * 16 * 4, 0xa5, np.uint8), np.full(1, -7, np.int32)
    buf, desc = np.frombuffer(stream, np.uint8).copy(), np.zeros(1, png.FRAME_DTYPE)
    desc["stream_end"] = len(stream)
    ptr = emu_harness.ptr

    def call(s=ptr(buf), d=ptr(desc), n=1, H=16, W=16, kind=3, oc=4, w=ptr(ws), nw=nws.value, o=ptr(out), st=ptr(status)):
        return lib.nsr_png_decode(s, d, n, H, W, kind, oc, w, nw, o, st, None)

    for kw, word in ((dict(H=0), b"sizes"), (dict(W=32769), b"sizes"), (dict(kind=4), b"kind"), (dict(oc=1), b"out_channels"), (dict(oc=5), b"out_channels"),
                     (dict(kind=1, oc=3), b"out_channels"), (dict(kind=2, oc=4), b"out_channels"), (dict(kind=0, oc=4), b"out_channels"),
                     (dict(s=None), b"null"), (dict(d=None), b"null"), (dict(w=None), b"null"), (dict(o=None), b"null"), (dict(st=None), b"null"),
                     (dict(nw=nws.value - 1), b"smaller"), (dict(w=C.c_void_p(ws.ctypes.data + 8)), b"aligned"),
                     (dict(d=C.c_void_p(desc.ctypes.data + 4)), b"aligned"), (dict(n=-1), b"batch"), (dict(n=65536), b"batch")):
        assert call(**kw) != 0 and word in lib.nsr_last_error(), kw
        assert (ws == 0xa5).all() and (out == 0xa5).all() and (status == -7).all(), kw      # nothing was launched
    assert call(n=0) == 0 and (out == 0xa5).all() and (status == -7).all()                  # an empty batch: nothing to do
    return call, out, status, R.pil_pixels(data)


def test_abi_errors_emulator(E):
    call, out, status, want = check_abi_errors(E.lib)
    assert call() == 0 and status[0] == 0                          # and the same arguments, all valid, do decode
    assert np.array_equal(out.reshape(16, 16, 4), want)


def test_abi_errors_product_library():
    """argument validation happens before any device work, so the product library answers it without a GPU; both libraries
    export the entries, and the compiler's report on the two kernels is in the resources file: no scratch"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    import json

    from nice_slam_amd import build
    build.build_lib()
    lib = _capi.Lib(_capi.LIB_PATH)
    for name in ("nsr_png_size", "nsr_png_decode"):
        assert hasattr(lib.cdll, name) and hasattr(emu_harness.emu_lib().cdll, name)
    check_abi_errors(lib)
    with open(build.RESOURCES) as fh:
        res = {k: v for k, v in json.load(fh).items() if "png_inflate_kernel" in k or "png_unfilter_kernel" in k}
    assert len(res) == 5 and all(v["scratch_bytes_per_lane"] == 0 for v in res.values())


# ---- 8. the dataset readers --------------------------------------------------------------------------------------------------------
def same(a, b):
    return a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def check_datasets(tmp_path, engine, device):
    for name, cfg in (("replica", R.replica_folder(str(tmp_path / "replica"))), ("tum", R.tum_folder(str(tmp_path / "tum")))):
        ref = datasets.get_dataset(cfg, device=device, engine=engine)
        assert ref.png_decoder == "pil" and ref.decoder == "pil" and len(ref) == 3
        for decoder in ("pil", "gpu"):
            ds = datasets.get_dataset(cfg, device=device, engine=engine, decoder=decoder, png_decoder="gpu")
            assert ds.png_decoder == "gpu" and ds.decoder == decoder
            for i in range(3):
                assert same(ref[i], ds[i]), (name, decoder, i)
            assert same(ref.load_batch([2, 0, 1]), ds.load_batch([2, 0, 1])), (name, decoder)
            assert ds.png_fallbacks == 0 and ds.decode_fallbacks == 0 and ref.png_fallbacks == 0
    # the config's own switch; one palette image among the colour files
    cfg = R.tum_folder(str(tmp_path / "tum2"), palette_at=1)
    ref = datasets.get_dataset(cfg, device=device, engine=engine)
    cfg["data"]["png_decoder"] = "gpu"
    ds = datasets.get_dataset(cfg, device=device, engine=engine)
    assert ds.png_decoder == "gpu" and datasets.get_dataset(cfg, device=device, engine=engine, png_decoder="pil").png_decoder == "pil"
    assert same(ref.load_batch([0, 1, 2]), ds.load_batch([0, 1, 2])) and ds.png_fallbacks == 1 and ds.decode_fallbacks == 0
    # an 8-bit grey depth file is widened as read_depth widens it
    cfg8 = R.tum_folder(str(tmp_path / "tum8"))
    ref8 = datasets.get_dataset(cfg8, device=device, engine=engine)
    Image.fromarray(R.image("grey8", 30, 42, seed=3)).save(ref8.depth_paths[1])
    ds8 = datasets.get_dataset(cfg8, device=device, engine=engine, png_decoder="gpu")
    assert same(ref8[1], ds8[1]) and ds8.png_fallbacks == 0 and float(ds8[1][2].max()) > 0
    # decoder="gpu" alone: the PNG colour files are counted fallbacks of the JPEG decoder, as before
    cfg = R.tum_folder(str(tmp_path / "tum3"))
    ref, old = datasets.get_dataset(cfg, device=device, engine=engine), datasets.get_dataset(cfg, device=device, engine=engine, decoder="gpu")
    assert same(ref.load_batch([0, 1, 2]), old.load_batch([0, 1, 2])) and old.decode_fallbacks == 3 and old.png_fallbacks == 0
    with pytest.raises(ValueError, match="png_decoder"):
        datasets.get_dataset(cfg, device=device, engine=engine, png_decoder="cpu")


def test_datasets_with_the_gpu_png_decoder(E, tmp_path):
    check_datasets(tmp_path, E, "cpu")
