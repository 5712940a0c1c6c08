"""CPU tests of the JPEG decoder (nice_slam_amd/csrc/nsr_jpegdec.h, nice_slam_amd/jpeg.py): the numpy restatement
(tests/jpegdec_reference.py) against Pillow's pixels, live and from tests/golden/jpeg_decode.npz, with zero differing pixels; the
kernel sources on the emulator against the restatement; the cases where the self-synchronisation can go wrong, each with the
property it is there for asserted; batches; the round trip through the encoder and the Motion-JPEG reader; sentinels and guards;
damaged streams and refusals; the dataset readers with ``decoder="gpu"``."""
import ctypes as C
import io
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image, features

import emu_harness
import jpeg_reference as R
import jpegdec_reference as D
from nice_slam_amd import _capi, datasets, jpeg
from nice_slam_amd.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "jpeg_decode.npz"))
GOLDEN_NAMES = sorted(k[:-4] for k in GOLDEN.files if k.endswith(".jpg"))
KINDS = ("recipe", "noise", "constant", "white")
QUALITIES = (1, 30, 90, 100)


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


def matrix(size, sampling):
    """the issue's cross product at one size and sampling: content x quality x tables x restart setting, 128 files"""
    return [(kind, size, sampling, q, opt, r) for kind in KINDS for q in QUALITIES for opt in (False, True) for r in range(4)]


def decode(E, files, sb=128):
    out, status = jpeg.decode_jpeg_status(files, engine=E, subsequence_bytes=sb)
    return out.numpy(), status


# ---- 1. the restatement against Pillow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", D.SAMPLINGS)
@pytest.mark.parametrize("size", D.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_live_pillow(size, sampling):
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo; the golden file holds its pixels")
    for case in matrix(size, sampling):
        data = D.case_file(*case)
        got, status = D.reference(data)
        assert status == 0 and np.array_equal(got, D.pil_pixels(data)), case


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_restatement_equals_golden_pillow(name):
    data = GOLDEN[name + ".jpg"].tobytes()
    if name.startswith("refused"):
        assert D.verdict(data) is not None
        return
    got, status = D.decode(data)
    assert status == 0 and np.array_equal(got, GOLDEN[name + ".rgb"])
    if features.check_feature("libjpeg_turbo"):
        assert np.array_equal(D.pil_pixels(data), GOLDEN[name + ".rgb"])


def test_golden_holds_what_it_is_there_for():
    info = {n: jpeg.probe_jpeg(GOLDEN[n + ".jpg"].tobytes()) for n in GOLDEN_NAMES}
    assert {p["sampling"] for p in info.values() if p["supported"]} == {"4:4:4", "4:2:2", "4:2:0", "grey"}
    assert info["default_33x49_420"]["restart_interval"] == 0 and info["rows_50x70_444"]["restart_interval"] == 9
    assert info["blocks3_50x70_420"]["restart_interval"] == 3 and info["blocks1_17x23_422"]["restart_interval"] == 1
    tables = {n: jpeg._parse(GOLDEN[n + ".jpg"].tobytes())["huff"] for n in ("default_33x49_420", "optimize_50x70_420")}
    assert tables["default_33x49_420"][(1, 0)] == (bytes(R.AC_BITS[0]), bytes(R.AC_VALS[0]))      # the typical tables of annex K
    assert tables["optimize_50x70_420"][(1, 0)][0] != bytes(R.AC_BITS[0])                         # tables of the file's own
    assert not info["refused_progressive_33x49"]["supported"] and "progressive" in info["refused_progressive_33x49"]["reason"]
    assert sum(os.path.getsize(os.path.join(HERE, "golden", f)) for f in ("jpeg_decode.npz",)) < 200 * 1024


# ---- 2. the emulator against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sb", (16, 128))
@pytest.mark.parametrize("sampling", D.SAMPLINGS)
@pytest.mark.parametrize("size", D.SIZES, ids=lambda s: "%dx%d" % s)
def test_emulator_equals_restatement(E, size, sampling, sb):
    cases = matrix(size, sampling)
    files = [D.case_file(*c) for c in cases]
    got, status = decode(E, files, sb)                               # one call: every file has its own tables and stream length
    assert status == [0] * len(files)
    for k, case in enumerate(cases):
        assert np.array_equal(got[k], D.reference(files[k])[0]), case


@pytest.mark.parametrize("name", [n for n in GOLDEN_NAMES if not n.startswith("refused")])
def test_emulator_equals_golden(E, name):
    for sb in (16, 128, 1024):
        got, status = decode(E, GOLDEN[name + ".jpg"].tobytes(), sb)
        assert status == [0] and np.array_equal(got[0], GOLDEN[name + ".rgb"]), sb


# ---- 3. where the self-synchronisation can go wrong --------------------------------------------------------------------------------
def sync_cases():
    """{name: (file, subsequence_bytes)}; test_sync_cases_have_their_property says what each is there for"""
    return {"noise_long_blocks": (D.case_file("noise", (104, 120), "4:4:4", 100, seed=1), 16),       # (a tile is 1024 subsequences here)
            "noise_split_pair": (D.case_file("noise", (50, 70), "4:4:4", 100, seed=2), 16),
            "constant_many_blocks": (D.pil_file(np.full((200, 200, 3), (200, 90, 30), np.uint8), quality=90), 128),
            "interval_shorter_than_subsequence": (D.case_file("recipe", (33, 49), "4:2:0", 30, restart=2), 128),
            "interval_across_rows": (D.case_file("recipe", (50, 70), "4:2:0", 90, restart=3), 16),
            "rst_wraps": (D.pil_file(D.recipe_image(112, 24, seed=5), quality=90, subsampling="4:4:4", restart_marker_rows=1), 16)}


def test_sync_cases_have_their_property():
    cases = sync_cases()
    data, sb = cases["noise_long_blocks"]
    lengths = D.chain_lengths(data)
    assert len(lengths) == 1 and lengths[0] > 3 * 1024 * sb               # more than three tiles of 1024 subsequences
    for name in ("noise_long_blocks", "noise_split_pair"):
        data, sb = cases[name]
        ends = np.array([0] + D.block_ends(data)[0])
        assert (np.diff(ends) // sb).min() >= 3 and (np.diff(ends) // sb).max() >= 5      # every block spans several subsequences
    assert D.split_pairs(cases["noise_split_pair"][0], 16) >= 1           # an FF 00 pair split across a subsequence boundary
    data, sb = cases["constant_many_blocks"]
    ends = np.array(D.block_ends(data)[0])
    assert len(D.chain_lengths(data)) == 1 and np.bincount(ends // sb).max() >= 150      # well over a hundred blocks in one subsequence
    data, sb = cases["interval_shorter_than_subsequence"]
    assert jpeg.probe_jpeg(data)["restart_interval"] == 1 and max(D.chain_lengths(data)) < sb and len(D.chain_lengths(data)) == 3 * 4
    data, sb = cases["interval_across_rows"]
    assert jpeg.probe_jpeg(data)["restart_interval"] == 3 and -(-70 // 16) == 5 and 5 % 3 != 0 and len(D.chain_lengths(data)) == 7
    data, sb = cases["rst_wraps"]
    marks = D.chains(D.parse(data), data)[1]
    assert len(marks) == 13 and marks == [m % 8 for m in range(13)]       # 14 MCU rows: RSTm wraps past RST7


@pytest.mark.parametrize("name", sorted(sync_cases()))
def test_sync_cases(E, name):
    data, sb = sync_cases()[name]
    want, ref_status = D.reference(data)
    assert ref_status == 0
    if features.check_feature("libjpeg_turbo"):
        assert np.array_equal(want, D.pil_pixels(data))
    for s in (sb, 128 if sb == 16 else 16):
        got, status = decode(E, data, s)
        assert status == [0] and np.array_equal(got[0], want), s


# ---- 4. batches and the workspace --------------------------------------------------------------------------------------------------
def batch_of_three():
    return [D.case_file("recipe", (33, 49), "4:2:0", 90), D.case_file("noise", (33, 49), "4:2:0", 100, True), D.case_file("white", (33, 49), "4:2:0", 30, False, 3)]


def test_batch_equals_single_calls(E):
    files = batch_of_three()
    assert len({len(f) for f in files}) == 3
    got, status = decode(E, files)
    assert status == [0, 0, 0]
    for k, f in enumerate(files):
        assert np.array_equal(got[k], decode(E, f)[0][0]) and np.array_equal(got[k], D.reference(f)[0])
    back, _ = decode(E, files[::-1])
    assert np.array_equal(back, got[::-1])                                # the place in the batch does not leak
    again, _ = decode(E, files)
    assert np.array_equal(again, got)                                     # a second call
    assert jpeg.decode_jpeg([], engine=E).shape == (0, 0, 0, 3)


def test_batch_of_257(E):
    files = [D.pil_file(D.noise_image(8, 8, seed=200 + k), quality=75) for k in range(257)]
    got, status = decode(E, files)
    assert status == [0] * 257
    for k in (0, 1, 127, 255, 256):
        assert np.array_equal(got[k], D.reference(files[k])[0])
    assert all(np.array_equal(got[k], D.decode(files[k])[0]) for k in range(0, 257, 16))


def test_mixed_sizes_raise(E):
    a, b, c = D.case_file("recipe", (16, 16), "4:2:0", 90), D.case_file("recipe", (17, 23), "4:2:0", 90), D.case_file("recipe", (16, 16), "4:4:4", 90)
    with pytest.raises(ValueError, match="frame 1"):
        jpeg.decode_jpeg([a, b], engine=E)
    with pytest.raises(ValueError, match="frame 1"):
        jpeg.decode_jpeg([a, c], engine=E)


# ---- 5. round trip and video -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", ("4:2:0", "4:4:4"))
def test_encoder_streams_decode_to_pillows_pixels(E, sub):
    for name in sorted(R.image_set()):
        for q in (1, 90, 100):
            data = R.reference_file(name, q, sub)
            got, status = decode(E, data)
            assert status == [0] and np.array_equal(got[0], D.pil_pixels(data)), (name, q)
    img = R.image_set()["recipe40x56"]
    assert np.array_equal(decode(E, jpeg.encode_jpeg(img, 90, sub, engine=E))[0][0], D.pil_pixels(R.reference_file("recipe40x56", 90, sub)))


def test_mjpeg_writer_then_reader(E, tmp_path):
    frames = [R.reference_file("small16x16", q, "4:2:0") for q in (1, 50, 75, 90, 100)]
    path = str(tmp_path / "v.avi")
    with jpeg.MjpegWriter(path, 16, 16, fps=25) as w:
        for f in frames:
            w.write(f)
    assert [c["data"] for c in R.find(R.walk_avi(open(path, "rb").read()), b"LIST", b"movi")["children"]] == frames
    with jpeg.MjpegReader(path, engine=E, batch=2) as video:
        assert len(video) == 5 and (video.width, video.height, video.fps) == (16, 16, 25.0)
        assert [video.frame_bytes(i) for i in range(5)] == frames
        got = video.read().numpy()
        part = video.read([3, 0]).numpy()
    assert got.shape == (5, 16, 16, 3) and all(np.array_equal(got[i], D.pil_pixels(f)) for i, f in enumerate(frames))
    assert np.array_equal(part, got[[3, 0]])
    assert np.array_equal(jpeg.read_video(path, engine=E).numpy(), got)
    with pytest.raises(ValueError, match="closed"):
        video.frame_bytes(0)
    (tmp_path / "one.jpg").write_bytes(frames[3])
    assert np.array_equal(jpeg.read_jpeg(str(tmp_path / "one.jpg"), engine=E).numpy(), got[3])
    (tmp_path / "not.avi").write_bytes(b"RIFF" + bytes(20))
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        jpeg.MjpegReader(str(tmp_path / "not.avi"), engine=E)


# ---- 6. sentinels and guards -------------------------------------------------------------------------------------------------------
def raw_decode(lib, files, sb=128, tail=4096, guard=512, edit=None):
    """The C ABI on numpy buffers: every file sits between `guard` bytes of 0xFF, sentinels stand behind the workspace and the
    output.  `edit(k, parsed)`: changes a frame's parsed header before the descriptors are built.  Returns (pixels, status)."""
    parsed = [jpeg._parse(f) for f in files]
    for k, p in enumerate(parsed):
        if edit is not None:
            edit(k, p)
    H, W, sampling = parsed[0]["height"], parsed[0]["width"], parsed[0]["sampling"]
    blob = b"".join(b"\xff" * guard + f for f in files) + b"\xff" * guard
    offsets = np.cumsum([0] + [guard + len(f) for f in files])[:-1] + guard
    desc = jpeg._descriptors(parsed, offsets)
    n = len(files)
    nws = C.c_int64(0)
    lib.call("nsr_jpegdec_size", n, H, W, jpeg.SAMPLING[sampling], max(len(f) for f in files), sb, C.byref(nws))
    ws = np.full(nws.value + tail + 16, 0xa5, np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:][:nws.value + tail]
    out = np.full(n * H * W * 3 + tail, 0xa5, np.uint8)
    status = np.full(n + 4, -7, np.int32)
    buf = np.frombuffer(blob, np.uint8)
    lib.call("nsr_jpegdec_decode", emu_harness.ptr(buf), emu_harness.ptr(desc), n, H, W, jpeg.SAMPLING[sampling], sb, emu_harness.ptr(ws), nws.value,
             emu_harness.ptr(out), emu_harness.ptr(status), None)
    assert (ws[nws.value:] == 0xa5).all() and (out[n * H * W * 3:] == 0xa5).all() and (status[n:] == -7).all()
    return out[:n * H * W * 3].reshape(n, H, W, 3), status[:n].tolist()


def test_sentinels_and_guard_bytes(E):
    for files, sb in ((batch_of_three(), 128), ([sync_cases()["noise_split_pair"][0]], 16), ([sync_cases()["interval_shorter_than_subsequence"][0]] * 2, 16),
                      ([D.case_file("recipe", (1, 1), "grey", 90)], 1024)):
        got, status = raw_decode(E.lib, files, sb)
        assert status == [0] * len(files)
        for k, f in enumerate(files):
            assert np.array_equal(got[k], D.reference(f)[0])              # a read outside a scan would have met 0xFF, not the file


# ---- 7. damaged streams, refusals --------------------------------------------------------------------------------------------------
def damaged():
    """(a file cut off in the middle of its scan, one with a flipped byte in its scan), each still a file the parser takes"""
    good = D.case_file("recipe", (33, 49), "4:2:0", 90)
    p = jpeg._parse(good)
    mid = (p["scan_begin"] + p["scan_end"]) // 2
    flipped = bytearray(good)
    flipped[mid] ^= 0x5a
    return good, good[:mid], bytes(flipped)


def test_damaged_streams_set_their_status_only(E):
    good, cut, flipped = damaged()
    other = D.case_file("noise", (33, 49), "4:2:0", 100)
    for bad in (cut, flipped):
        assert jpeg.probe_jpeg(bad)["supported"] and D.reference(bad)[1] != 0
        for sb in (16, 128):
            got, status = raw_decode(E.lib, [good, bad, other], sb)
            assert status[0] == 0 and status[1] != 0 and status[2] == 0
            assert np.array_equal(got[0], D.reference(good)[0]) and np.array_equal(got[2], D.reference(other)[0])
        with pytest.raises(ValueError, match="frame 1"):
            jpeg.decode_jpeg([good, bad], engine=E)
    # markers out of sequence, and fewer than the interval asks for
    rows = D.case_file("recipe", (50, 70), "4:4:4", 90, restart=1)
    swapped = rows.replace(b"\xff\xd1", b"\xff\xd3")
    missing = bytearray(rows)
    at = rows.index(b"\xff\xd2")
    del missing[at:at + 2]
    for bad in (swapped, bytes(missing)):
        assert bad != rows and raw_decode(E.lib, [bad, rows])[1][0] & 8 and raw_decode(E.lib, [bad, rows])[1][1] == 0


def test_refusals(E):
    progressive = GOLDEN["refused_progressive_33x49.jpg"].tobytes()
    rgb = GOLDEN["refused_rgb_adobe0_17x23.jpg"].tobytes()
    f444 = D.case_file("recipe", (17, 23), "4:4:4", 90)
    at = f444.index(b"\xff\xc0")
    f440 = f444[:at + 11] + b"\x12" + f444[at + 12:]                      # the luma sampling factors 1x1 -> 1x2: 4:4:0
    assert f444[at + 11] == 0x11
    oversubscribed = bytearray(f444)
    dht = f444.index(b"\xff\xc4")
    oversubscribed[dht + 5] = 3                                           # three codes of length 1
    cmyk = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "CMYK").save(cmyk, "JPEG")
    for bad, word in ((progressive, "progressive"), (rgb, "transform 0"), (f440, "sampling"), (bytes(oversubscribed), "oversubscribed"),
                      (cmyk.getvalue(), "4 components"), (b"\x89PNG\r\n\x1a\n" + bytes(40), "not a JPEG")):
        info = jpeg.probe_jpeg(bad)
        assert not info["supported"] and word in info["reason"], (word, info)
        assert (D.verdict(bad) is not None) or word == "not a JPEG"
        with pytest.raises(ValueError, match="frame 0 is not supported"):
            jpeg.decode_jpeg(bad, engine=E)
        with pytest.raises(ValueError, match="frame 1 is not supported"):
            jpeg.decode_jpeg([f444, bad], engine=E)
    good = jpeg.probe_jpeg(f444)
    assert good == {"height": 17, "width": 23, "components": 3, "sampling": "4:4:4", "restart_interval": 0, "supported": True, "reason": None}


def check_abi_errors(lib):
    data = D.case_file("recipe", (16, 16), "4:2:0", 90)
    p = jpeg._parse(data)
    nws = C.c_int64(-7)
    assert lib.nsr_jpegdec_size(1, 16, 16, 2, len(data), 128, C.byref(nws)) == 0 and nws.value > 0
    for args in ((1, 0, 16, 2, 0, 128), (1, 16, 65536, 2, 0, 128), (1, 16, 16, 4, 0, 128), (1, 16, 16, -1, 0, 128), (-1, 16, 16, 2, 0, 128),
                 (65536, 16, 16, 2, 0, 128), (1, 16, 16, 2, 0, 12), (1, 16, 16, 2, 0, 130), (1, 16, 16, 2, 0, 1028), (1, 16, 16, 2, -1, 128),
                 (1, 16, 16, 2, (1 << 28) + 1, 128)):
        a = C.c_int64(-7)
        assert lib.nsr_jpegdec_size(*args, C.byref(a)) != 0 and lib.nsr_last_error() and a.value == -7, args
    assert lib.nsr_jpegdec_size(1, 16, 16, 2, 0, 128, None) != 0 and b"null" in lib.nsr_last_error()
    big = C.c_int64(0)
    assert lib.nsr_jpegdec_size(1, 65535, 65535, 0, 0, 128, C.byref(big)) == 0 and big.value > 3 * 65535 * 65535
    ws = np.full(nws.value + 32, 0xa5, np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:][:nws.value + 16]
    out, status = np.full(16 * 16 * 3, 0xa5, np.uint8), np.full(1, -7, np.int32)
    buf, desc = np.frombuffer(data, np.uint8), jpeg._descriptors([p], [0])
    ptr = emu_harness.ptr

    def call(files=ptr(buf), d=ptr(desc), n=1, H=16, W=16, sampling=2, sb=128, w=ptr(ws), nw=nws.value, o=ptr(out), st=ptr(status)):
        return lib.nsr_jpegdec_decode(files, d, n, H, W, sampling, sb, w, nw, o, st, None)

    for kw, word in ((dict(H=0), b"sizes"), (dict(W=65536), b"sizes"), (dict(sampling=4), b"sampling"), (dict(sb=20 + 2), b"subsequence"), (dict(sb=8), b"subsequence"),
                     (dict(files=None), b"null"), (dict(d=None), b"null"), (dict(w=None), b"null"), (dict(o=None), b"null"), (dict(st=None), b"null"),
                     (dict(nw=nws.value - 1), b"smaller"), (dict(w=C.c_void_p(ws.ctypes.data + 8)), b"aligned"), (dict(n=-1), b"batch")):
        assert call(**kw) != 0 and word in lib.nsr_last_error(), kw
        assert (ws == 0xa5).all() and (out == 0xa5).all() and (status == -7).all(), kw      # nothing was launched
    assert call(n=0) == 0 and (out == 0xa5).all() and (status == -7).all()                  # an empty batch: nothing to do
    return call, out, status


def test_abi_errors_emulator(E):
    call, out, status = check_abi_errors(E.lib)
    assert call() == 0 and status[0] == 0                          # and the same arguments, all valid, do decode
    assert np.array_equal(out.reshape(16, 16, 3), D.reference(D.case_file("recipe", (16, 16), "4:2:0", 90))[0])


def test_abi_errors_product_library():
    """argument validation happens before any device work, so the product library answers it without a GPU; both libraries
    export the entries"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from nice_slam_amd import build
    build.build_lib()
    lib = _capi.Lib(_capi.LIB_PATH)
    for name in ("nsr_jpegdec_size", "nsr_jpegdec_decode"):
        assert hasattr(lib.cdll, name) and hasattr(emu_harness.emu_lib().cdll, name)
    check_abi_errors(lib)


# ---- 8. the dataset readers --------------------------------------------------------------------------------------------------------
def replica_folder(root, files):
    """a Replica-layout folder with these colour files and PNG depth; returns its config"""
    os.makedirs(os.path.join(root, "results"))
    rng = np.random.default_rng(4)
    for k, data in enumerate(files):
        with open(os.path.join(root, "results", f"frame{k:06d}.jpg"), "wb") as fh:
            fh.write(data)
        Image.fromarray(rng.integers(0, 6000, (34, 50)).astype(np.uint16)).save(os.path.join(root, "results", f"depth{k:06d}.png"))
    with open(os.path.join(root, "traj.txt"), "w") as fh:
        for k in range(len(files)):
            m = np.eye(4)
            m[:3, 3] = (0.1 * k, 0.2, 0.3)
            fh.write(" ".join(repr(float(v)) for v in m.reshape(-1)) + "\n")
    return {"dataset": "replica", "scale": 1.0, "data": {"input_folder": root},
            "cam": {"H": 34, "W": 50, "fx": 40.0, "fy": 40.0, "cx": 24.5, "cy": 16.5, "png_depth_scale": 1000.0, "crop_edge": 2}}


def dataset_files():
    return [D.pil_file(D.recipe_image(34, 50, seed=k), quality=90, **opts) for k, opts in enumerate(({}, {"optimize": True}, {"subsampling": "4:4:4"}))]


def check_datasets(tmp_path, engine, device):
    files = dataset_files()
    assert all(D.reference(f)[1] == 0 and jpeg.probe_jpeg(f)["supported"] for f in files)        # none of them needs the fallback
    cfg = replica_folder(str(tmp_path / "seq"), files)
    ref = datasets.get_dataset(cfg, device=device, engine=engine)
    ds = datasets.get_dataset(cfg, device=device, engine=engine, decoder="gpu")
    assert ref.decoder == "pil" and ds.decoder == "gpu"
    for i in range(3):
        a, b = ref[i], ds[i]
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    a, b = ref.load_batch([2, 0, 1]), ds.load_batch([2, 0, 1])
    assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    assert ds.decode_fallbacks == 0 and ref.decode_fallbacks == 0
    cfg2 = replica_folder(str(tmp_path / "seq2"), [files[0], D.pil_file(D.recipe_image(34, 50, seed=1), quality=90, progressive=True), files[2]])
    cfg2["data"]["decoder"] = "gpu"
    ref2, ds2 = datasets.get_dataset(cfg2, device=device, engine=engine, decoder="pil"), datasets.get_dataset(cfg2, device=device, engine=engine)
    assert ds2.decoder == "gpu" and ref2.decoder == "pil"
    a, b = ref2.load_batch([0, 1, 2]), ds2.load_batch([0, 1, 2])
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and ds2.decode_fallbacks == 1
    assert all(torch.equal(x, y) for x, y in zip(ref2[1][1:], ds2[1][1:])) and ds2.decode_fallbacks == 2
    with pytest.raises(ValueError, match="decoder"):
        datasets.get_dataset(cfg, device=device, engine=engine, decoder="cpu")


def test_datasets_with_the_gpu_decoder(E, tmp_path):
    check_datasets(tmp_path, E, "cpu")
