"""CPU tests of the JPEG encoder (nice_slam_amd/csrc/nsr_jpeg.h, nice_slam_amd/jpeg.py): the kernel sources run on the emulator
against the numpy restatement (tests/jpeg_reference.py) byte for byte; the streams through PIL's decoder; the restatement held to
PIL's own encoder within one quality step; the capacity the size query reports; the AVI writer; the callers; the ABI's error paths."""
import ctypes as C
import io
import os
import shutil
import struct

import numpy as np
import pytest
import torch
from PIL import Image, JpegImagePlugin

import emu_harness
import jpeg_reference as R
from nice_slam_amd import _capi, imgeval, jpeg, viewer
from nice_slam_amd.engine import Engine

SUBS = ("4:2:0", "4:4:4")
IMAGES = R.image_set()


@pytest.fixture(scope="module")
def E():
    return Engine(emu_harness.emu_lib(), "cpu")


# ---- 1. byte equality with the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_bytes_equal_the_restatement(E, name, sub):
    for q in R.QUALITIES:
        want = R.reference_file(name, q, sub)
        got = jpeg.encode_jpeg(IMAGES[name], q, sub, engine=E)
        assert len(got) == 1 and got[0] == want, (name, sub, q)
        if q == 90:
            assert jpeg.encode_jpeg(torch.from_numpy(IMAGES[name]), q, sub, engine=E)[0] == want       # a second call, a tensor


@pytest.mark.parametrize("sub", SUBS)
def test_batch_of_three_equals_three_calls(E, sub):
    batch = R.batch_of_three()
    got = jpeg.encode_jpeg(batch, 75, sub, engine=E)
    assert len(got) == 3 and len({len(g) for g in got}) == 3
    for k in range(3):
        assert got[k] == jpeg.encode_jpeg(batch[k], 75, sub, engine=E)[0] == R.encode(batch[k], 75, sub)
    assert jpeg.encode_jpeg(batch[::-1].copy(), 75, sub, engine=E) == got[::-1]                       # the place in the batch does not leak
    assert jpeg.encode_jpeg(batch[:0], 75, sub, engine=E) == []


@pytest.mark.parametrize("name", sorted(R.round_cases()))
def test_more_than_one_round_of_every_loop(E, name):
    batch, q, sub = R.round_cases()[name]
    got = jpeg.encode_jpeg(batch, q, sub, engine=E)
    assert got == [R.encode(img, q, sub) for img in batch]
    if name.startswith("wide"):
        rows = [r for r in R.entropy_segment(got[0]).split(b"\xff\xd0")]
        assert len(rows[0]) * 8 > 131072 and batch.shape[2] // (8 if sub == "4:4:4" else 16) * (3 if sub == "4:4:4" else 6) > 256


def test_every_quality_on_one_block(E):
    """the library's tables at every quality, through the bytes of one 8 x 8 block"""
    img = R.recipe_image(8, 8, seed=3)
    for q in range(1, 101):
        assert jpeg.encode_jpeg(img, q, "4:4:4", engine=E)[0] == R.encode(img, q, "4:4:4"), q


def test_rst_cycle_wraps():
    seg = R.entropy_segment(R.reference_file("recipe100x150", 90, "4:4:4"))
    assert R.restart_markers(seg) == [m % 8 for m in range(12)]                  # 13 MCU rows: past RST7 back to RST0


# ---- 2. valid streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_pil_opens_every_stream(E, sub):
    for name, img in IMAGES.items():
        for q in R.QUALITIES:
            data = R.reference_file(name, q, sub)
            with Image.open(io.BytesIO(data)) as im:
                assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and im.format == "JPEG"
                assert JpegImagePlugin.get_sampling(im) == (2 if sub == "4:2:0" else 0)
                with Image.open(io.BytesIO(R.pil_file(img, q, sub))) as theirs:
                    assert im.quantization == theirs.quantization
                im.load()                                                         # decoded to the end
                side = 16 if sub == "4:2:0" else 8
                rows = -(-img.shape[0] // side)
                assert R.restart_markers(R.entropy_segment(data)) == [m % 8 for m in range(rows - 1)]
        # the decode of the library's stream is that of the restatement's
        got = jpeg.encode_jpeg(img, 90, sub, engine=E)[0]
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(got))), np.asarray(Image.open(io.BytesIO(R.reference_file(name, 90, sub)))))


def test_quantisation_tables_are_pils_at_every_quality():
    img = np.zeros((8, 8, 3), np.uint8)
    for q in range(1, 101):
        with Image.open(io.BytesIO(R.pil_file(img, q, "4:4:4"))) as theirs, Image.open(io.BytesIO(jpeg.jfif_header(8, 8, q, "4:4:4") + b"\xff\xd9")) as ours, \
                Image.open(io.BytesIO(R.header(8, 8, q, "4:4:4") + b"\xff\xd9")) as ref:
            assert ours.quantization == theirs.quantization == ref.quantization, q
        assert [list(t) for t in jpeg.quant_tables(q)] == [[int(v) for v in t] for t in R.quant_tables(q)]


def test_headers_agree():
    for sub in SUBS:
        for h, w in ((1, 1), (17, 23), (540, 960), (65535, 65535)):
            assert jpeg.jfif_header(h, w, 90, sub) == R.header(h, w, 90, sub)


def test_huffman_tables_are_pils():
    """the DHT segments of a PIL file written with optimize=False hold the tables typed in here"""
    data = R.pil_file(IMAGES["recipe40x56"], 90, "4:2:0")
    theirs, at = {}, 2
    while data[at + 1] != 0xda:
        length = struct.unpack(">H", data[at + 2:at + 4])[0]
        if data[at + 1] == 0xc4:
            p, end = at + 4, at + 2 + length
            while p < end:
                n = sum(data[p + 1:p + 17])
                theirs[data[p]] = (list(data[p + 1:p + 17]), list(data[p + 17:p + 17 + n]))
                p += 17 + n
        at += 2 + length
    assert theirs == {0x00: (list(R.DC_BITS[0]), R.DC_VALS), 0x01: (list(R.DC_BITS[1]), R.DC_VALS),
                      0x10: (list(R.AC_BITS[0]), R.AC_VALS[0]), 0x11: (list(R.AC_BITS[1]), R.AC_VALS[1])}


# ---- 3. byte stuffing ------------------------------------------------------------------------------------------------------------
def test_byte_stuffing_is_exercised(E):
    for sub in SUBS:
        data = R.reference_file("noise33x47", 100, sub)
        seg = R.entropy_segment(data)
        assert b"\xff\x00" in seg
        assert all(seg[i + 1] == 0 or 0xd0 <= seg[i + 1] <= 0xd7 for i in range(len(seg) - 1) if seg[i] == 0xff)
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert np.abs(np.asarray(im).astype(int) - IMAGES["noise33x47"].astype(int)).mean() < (2 if sub == "4:4:4" else 60)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------
def raw_encode(lib, img, quality, sub, tail=4096):
    """the C ABI on numpy buffers with sentinels behind the workspace and the capacity: (offsets, out, capacity, workspace, its size)"""
    n, H, W = img.shape[:3]
    nws, cap = C.c_int64(0), C.c_int64(0)
    lib.call("nsr_jpeg_size", n, H, W, jpeg.SUBSAMPLING[sub], C.byref(nws), C.byref(cap))
    ws = np.full(nws.value + tail + 16, 0xa5, np.uint8)
    shift = (-ws.ctypes.data) % 16
    ws = ws[shift:shift + nws.value + tail]
    out = np.full(cap.value + tail, 0xa5, np.uint8)
    offsets = np.full(n + 1, -1, np.int64)
    lib.call("nsr_jpeg_encode", emu_harness.ptr(img), n, H, W, quality, jpeg.SUBSAMPLING[sub], emu_harness.ptr(ws), nws.value,
             emu_harness.ptr(out), cap.value, emu_harness.ptr(offsets), None)
    return offsets, out, cap.value, ws, nws.value


def test_capacity_and_sentinels(E):
    img = np.stack([R.noise_image(33, 47, seed=5), R.noise_image(33, 47, seed=6)])
    offsets, out, cap, ws, nws = raw_encode(E.lib, img, 100, "4:4:4")
    used = int(offsets[-1])
    assert offsets[0] == 0 and (np.diff(offsets) > 0).all() and used <= cap
    assert (out[used:] == 0xa5).all()                                             # behind the used range and behind the capacity
    assert (ws[nws:] == 0xa5).all()
    for k in range(2):
        assert jpeg.jfif_header(33, 47, 100, "4:4:4") + out[offsets[k]:offsets[k + 1]].tobytes() + b"\xff\xd9" == R.encode(img[k], 100, "4:4:4")
    # noise at quality 100 is far from the bound: a block of 63 AC codes of 26 bits and a DC code of 20, every byte stuffed
    blocks = 2 * 5 * 6 * 3
    assert cap >= 2 * blocks * (63 * 26 + 20) // 8 and used < cap // 2


# ---- 5. held to PIL --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("size", R.RECIPE_SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_is_within_one_quality_step_of_pil(size, sub):
    name = "recipe%dx%d" % size
    img = IMAGES[name]
    for q in (75, 90, 95):
        planes, mine, theirs = R.pil_gate(R.reference_file(name, q, sub), img, q, sub)
        for c, (ours, a, b, d, rising, bound) in enumerate(planes):
            print(f"{name} {sub} q{q} plane {c}: ours {ours:.3f} dB, PIL {a:.3f} {b:.3f} {d:.3f} ({'rising' if rising else 'flat'}), "
                  f"ours - PIL(q) {ours - b:+.3f}, bound {bound:.3f}")
            assert rising or (sub == "4:2:0" and c > 0)           # about PIL alone: luma everywhere, every plane of 4:4:4 rises
            assert ours >= bound, (name, sub, q, c)
        print(f"{name} {sub} q{q}: {mine} bytes, PIL {theirs}")
        if size == (100, 150):
            assert theirs[0] < theirs[1] < theirs[2]              # about PIL alone
            assert mine <= theirs[2]


# ---- 6. video --------------------------------------------------------------------------------------------------------------------
def test_mjpeg_writer(tmp_path):
    frames = [R.reference_file("small16x16", q, "4:2:0") for q in (1, 50, 75, 90, 100)]
    frames[1] += b"\xff" * (1 - len(frames[1]) % 2)               # lengths differ, odd and even both occur
    frames[2] += b"\xff" * (len(frames[2]) % 2)
    assert len({len(f) for f in frames}) == 5 and {len(f) % 2 for f in frames} == {0, 1}
    path = tmp_path / "v.avi"
    with jpeg.MjpegWriter(str(path), 16, 16, fps=30) as w:
        for f in frames:
            w.write(f)
    data = path.read_bytes()
    riff = R.walk_avi(data)                                        # every chunk size against the file's length
    avih = struct.unpack("<14I", R.find(riff, b"avih")["data"])
    assert avih[0] == 33333 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (16, 16) and avih[3] & 0x10 and avih[7] == max(map(len, frames))
    strh = R.find(riff, b"strh")["data"]
    assert strh[:8] == b"vidsMJPG" and len(strh) == 56
    scale, rate, start, length = struct.unpack("<4I", strh[20:36])
    assert (scale, rate, start, length) == (1, 30, 0, 5) and struct.unpack("<4H", strh[48:56]) == (0, 0, 16, 16)
    strf = R.find(riff, b"strf")["data"]
    size, w_, h_, planes, bits, comp = struct.unpack("<IiiHH4s", strf[:20])
    assert (size, w_, h_, planes, bits, comp) == (40, 16, 16, 1, 24, b"MJPG") and len(strf) == 40
    movi = R.find(riff, b"LIST", b"movi")
    assert [c["id"] for c in movi["children"]] == [b"00dc"] * 5
    assert [c["data"] for c in movi["children"]] == frames
    for c in movi["children"]:
        assert c["offset"] % 2 == 0                                # padded to even length
    idx = R.find(riff, b"idx1")["data"]
    assert len(idx) == 16 * 5
    for k, c in enumerate(movi["children"]):
        ckid, flags, off, size = struct.unpack("<4sIII", idx[16 * k:16 * k + 16])
        assert ckid == b"00dc" and flags == 0x10 and size == len(frames[k])
        at = movi["offset"] + 8 + off                              # offsets count from the 'movi' fourcc
        assert at == c["offset"] and data[at:at + 4] == b"00dc"
    assert riff["children"][-1]["id"] == b"idx1"
    with pytest.raises(ValueError):
        w.write(frames[0])                                         # closed
    with jpeg.MjpegWriter(str(tmp_path / "ntsc.avi"), 16, 16, fps=29.97) as w2:
        w2.write(frames[0])
    strh = R.find(R.walk_avi((tmp_path / "ntsc.avi").read_bytes()), b"strh")["data"]
    assert struct.unpack("<2I", strh[20:28]) == (1000, 29970)


def test_mjpeg_writer_size_guard(tmp_path, monkeypatch):
    frame = R.reference_file("small16x16", 90, "4:2:0")
    path = tmp_path / "small.avi"
    monkeypatch.setattr(jpeg.MjpegWriter, "MAX_BYTES", jpeg.MjpegWriter._HEADER_BYTES + 2 * (8 + len(frame) + len(frame) % 2 + 16) + 8 + 5)
    w = jpeg.MjpegWriter(str(path), 16, 16)
    w.write(frame)
    w.write(frame)
    before = w.fh.tell()
    with pytest.raises(ValueError, match="would pass"):
        w.write(frame)
    assert w.fh.tell() == before                                   # nothing of the refused frame was written
    w.close()
    data = path.read_bytes()
    assert len(data) <= jpeg.MjpegWriter.MAX_BYTES
    assert len(R.find(R.walk_avi(data), b"LIST", b"movi")["children"]) == 2
    monkeypatch.undo()
    assert jpeg.MjpegWriter.MAX_BYTES == (1 << 31) - 1


# ---- 7. callers ------------------------------------------------------------------------------------------------------------------
def small_replay(E):
    from test_view_emu import H, W, oriented_room, toy_run
    est, gt = toy_run(3)
    rp = viewer.Replay(est[0], cam_scale=0.3, estimate_c2w_list=est, gt_c2w_list=gt, width=W, height=H, engine=E)
    v, f = oriented_room((5, 4, 3))
    rp.update_mesh((v, f, np.random.default_rng(2).integers(0, 256, (len(v), 3), dtype=np.uint8)))
    rp.update_pose(1, est[1])
    rp.update_pose(1, gt[1], gt=True)
    return rp, H, W


def test_replay_save_with_the_gpu_encoder(E, tmp_path):
    rp, H, W = small_replay(E)
    frame = rp.frame().numpy()
    rp.save(str(tmp_path / "gpu.jpg"), encoder="gpu")
    rp.save(str(tmp_path / "pil.jpg"))
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90)
    assert (tmp_path / "pil.jpg").read_bytes() == buf.getvalue()                  # the default: what Image.save(quality=90) writes
    data = (tmp_path / "gpu.jpg").read_bytes()
    assert data == R.encode(frame, 90, "4:2:0")
    with Image.open(io.BytesIO(data)) as im:
        assert im.size == (W, H) and im.mode == "RGB"
    planes, _, _ = R.pil_gate(data, frame, 90, "4:2:0")
    for c, (ours, a, b, d, rising, bound) in enumerate(planes):
        print(f"replay frame plane {c}: ours {ours:.3f} dB, PIL {a:.3f} {b:.3f} {d:.3f}, bound {bound:.3f}")
        assert ours >= bound
    with pytest.raises(ValueError, match="encoder"):
        rp.save(str(tmp_path / "x.jpg"), encoder="cpu")
    sheet = torch.from_numpy(frame)
    imgeval.save_sheet(sheet, str(tmp_path / "sheet.jpg"), encoder="gpu", engine=E)
    assert (tmp_path / "sheet.jpg").read_bytes() == data
    jpeg.save_jpeg(frame, str(tmp_path / "q.jpg"), quality=50, subsampling="4:4:4", engine=E)
    assert (tmp_path / "q.jpg").read_bytes() == R.encode(frame, 50, "4:4:4")


def test_visualizer_with_the_gpu_encoder(E, tmp_path):
    import figure_reference as F
    from test_figure_emu import StubRenderer
    color, gt_color, depth, gt_depth = F.main_case()
    gd, gc = torch.from_numpy(gt_depth[0]), torch.from_numpy(gt_color[0])
    names, sheets = {}, {}
    for enc in ("pil", "gpu"):
        vis = imgeval.Visualizer(2, 5, str(tmp_path / enc), StubRenderer(color, depth), False, "cpu", stride=1, margin=3, gap=2, engine=E, encoder=enc)
        calls = []
        real = E.lib.nsr_jpeg_encode
        E.lib.nsr_jpeg_encode = lambda *a: calls.append(a[1]) or real(*a)
        try:
            poses = []
            for k in (1, 0, 2):
                t = torch.eye(4)
                t[0, 3] = k
                poses.append(t)
            sheets[enc] = vis.vis_many(6, [0, 3, 5], poses, gd, gc, None, None).numpy()
            vis.vis(8, 0, gd, gc, poses[0], None, None)
        finally:
            E.lib.nsr_jpeg_encode = real
        assert calls == ([2, 1] if enc == "gpu" else [])                           # the sheets of one vis_many: one call
        names[enc] = sorted(os.listdir(tmp_path / enc))
    assert names["gpu"] == names["pil"] == ["00006_0000.jpg", "00006_0005.jpg", "00008_0000.jpg"]
    assert np.array_equal(sheets["gpu"], sheets["pil"])
    for k, name in enumerate(names["gpu"][:2]):
        assert (tmp_path / "gpu" / name).read_bytes() == R.encode(sheets["gpu"][k], 90, "4:2:0")
        with Image.open(tmp_path / "gpu" / name) as a, Image.open(tmp_path / "pil" / name) as b:
            assert a.size == b.size and np.abs(np.asarray(a).astype(int) - np.asarray(b).astype(int)).mean() < 2.0
    with pytest.raises(ValueError, match="encoder"):
        imgeval.Visualizer(2, 5, str(tmp_path / "x"), None, False, "cpu", engine=E, encoder="cpu")


def test_command_line_flags(capsys):
    with pytest.raises(SystemExit):
        viewer.main(["--help"])
    text = capsys.readouterr().out
    assert "--encoder" in text and "--video" in text and "vis.avi" in text


# ---- 8. the ABI ------------------------------------------------------------------------------------------------------------------
def check_abi_errors(lib):
    nws, cap = C.c_int64(-7), C.c_int64(-7)
    assert lib.nsr_jpeg_size(1, 16, 16, 2, C.byref(nws), C.byref(cap)) == 0 and nws.value > 0 and cap.value > 0
    for args in ((1, 0, 16, 2), (1, 16, 0, 2), (1, 65536, 16, 2), (1, 16, 65536, 0), (1, 16, 16, 1), (1, 16, 16, 3), (-1, 16, 16, 2), (65536, 16, 16, 2)):
        a, b = C.c_int64(-7), C.c_int64(-7)
        assert lib.nsr_jpeg_size(*args, C.byref(a), C.byref(b)) != 0 and lib.nsr_last_error() and (a.value, b.value) == (-7, -7), args
    assert lib.nsr_jpeg_size(1, 16, 16, 2, None, C.byref(cap)) != 0 and b"null" in lib.nsr_last_error()
    assert lib.nsr_jpeg_size(1, 65535, 65535, 0, C.byref(nws), C.byref(cap)) == 0 and cap.value > 2 * 65535 * 65535      # the largest image
    img = R.recipe_image(16, 16)
    lib.nsr_jpeg_size(1, 16, 16, 2, C.byref(nws), C.byref(cap))
    ws = np.full(nws.value + 16, 0xa5, np.uint8)
    ws = ws[(-ws.ctypes.data) % 16:][:nws.value]
    out, off = np.full(cap.value, 0xa5, np.uint8), np.full(2, -1, np.int64)
    p = emu_harness.ptr

    def call(images=p(img), n=1, H=16, W=16, q=90, sub=2, w=p(ws), nw=nws.value, o=p(out), no=cap.value, offs=p(off)):
        return lib.nsr_jpeg_encode(images, n, H, W, q, sub, w, nw, o, no, offs, None)

    for kw, word in ((dict(q=0), b"quality"), (dict(q=101), b"quality"), (dict(H=0), b"sizes"), (dict(W=65536), b"sizes"), (dict(sub=1), b"subsampling"),
                     (dict(images=None), b"null"), (dict(w=None), b"null"), (dict(o=None), b"null"), (dict(offs=None), b"null"),
                     (dict(nw=nws.value - 1), b"smaller"), (dict(no=cap.value - 1), b"smaller"), (dict(n=-1), b"batch")):
        assert call(**kw) != 0 and word in lib.nsr_last_error(), kw
        assert (ws == 0xa5).all() and (out == 0xa5).all() and (off == -1).all(), kw      # nothing was launched
    assert call(n=0) == 0 and (out == 0xa5).all() and (off == -1).all()                  # an empty batch: nothing to do
    return call


def test_abi_errors_emulator(E):
    call = check_abi_errors(E.lib)
    assert call() == 0                                             # and the same arguments, all valid, do encode


def test_abi_errors_product_library():
    """argument validation happens before any device work, so the product library answers it without a GPU; both libraries
    export the entries"""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    from nice_slam_amd import build
    build.build_lib()
    lib = _capi.Lib(_capi.LIB_PATH)
    for name in ("nsr_jpeg_size", "nsr_jpeg_encode"):
        assert hasattr(lib.cdll, name) and hasattr(emu_harness.emu_lib().cdll, name)
    check_abi_errors(lib)
