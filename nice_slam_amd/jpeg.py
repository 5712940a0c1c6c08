"""JPEG encoding on the GPU, and a Motion-JPEG video written around the streams.

    from nice_slam_amd import jpeg
    files = jpeg.encode_jpeg(frames, quality=90)                 # u8 [n, H, W, 3] on the device -> n complete JFIF files (bytes)
    jpeg.save_jpeg(sheet, "00010_0000.jpg")
    with jpeg.MjpegWriter("vis.avi", 960, 540, fps=30) as video:
        for f in files:
            video.write(f)

The encoder is baseline sequential DCT, 8 bit, three components (JFIF YCbCr), 4:2:0 or 4:4:4, with the quantisation tables of the
IJG quality rule and the "typical" Huffman tables of T.81 annex K -- what PIL writes for ``quality=q`` with ``optimize=False`` --
and a restart interval of one MCU row (PIL's ``restart_marker_rows=1``), which is what lets every MCU row be coded on its own.
The colour conversion, the chroma average, the DCT, the quantisation, the Huffman coding, the byte stuffing and the compaction of a
whole batch run in libnsr.so (include/nsr.h, "JPEG encoding"; the arithmetic is written out in csrc/nsr_jpeg.h: integers end to
end, the same bytes on every run).  The host writes the markers around each frame's entropy-coded segment and reads the device
twice per batch: the frames' offsets, then exactly the bytes that were used.

``MjpegWriter`` writes a RIFF AVI 1.0 file (one ``vids`` / ``MJPG`` stream, ``00dc`` chunks, an ``idx1`` index), which ffmpeg, VLC
and OpenCV read; it stops with an error before the file would pass 2^31 - 1 bytes (OpenDML is not written).

And the way back: baseline JPEG files decoded on the GPU, and the reader of such a video.

    info = jpeg.probe_jpeg(data)                                 # size, sampling, restart interval, supported (and why not)
    frames = jpeg.decode_jpeg([data0, data1])                    # files (bytes) of one size -> u8 [n, H, W, 3] on the device
    img = jpeg.read_jpeg("frame000000.jpg")                      # u8 [H, W, 3]
    with jpeg.MjpegReader("vis.avi") as video:
        frames = video.read()                                    # u8 [len(video), H, W, 3]

The decoder takes what Pillow writes by default and what the dataset sequences hold: SOF0, 8 bit, Huffman coded, one interleaved
scan, greyscale or YCbCr at 4:4:4, 4:2:2 or 4:2:0, any tables (optimised ones too), any restart interval or none.  The host walks
the markers, checks the tables and uploads the files' bytes as they are with one descriptor per file; the entropy decoding (by
self-synchronising subsequences), the DC sums, the inverse DCT, the upsampling and the colour conversion run in libnsr.so
(include/nsr.h, "JPEG decoding"; csrc/nsr_jpegdec.h writes the arithmetic out).  The pixels are those of libjpeg-turbo's default
decoder -- ``np.array(Image.open(f).convert("RGB"))`` -- bit for bit (checked against Pillow 12.2.0 with libjpeg-turbo 3.1,
``features.version("jpg")`` 6.2).  ``decode_jpeg`` never falls back: a file outside this set, or a damaged stream, raises.
"""
from __future__ import annotations

import ctypes as C
import re
import struct
from typing import List, Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, gpu

__all__ = ["encode_jpeg", "save_jpeg", "MjpegWriter", "quant_tables", "jfif_header", "SUBSAMPLING",
           "probe_jpeg", "decode_jpeg", "decode_jpeg_status", "read_jpeg", "MjpegReader", "read_video", "SAMPLING"]

SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2}          # the library's codes: PIL's JpegImagePlugin.get_sampling
MAX_BYTES_PER_LAUNCH = 1 << 31                  # workspace + worst-case output of one library call (a batch is split to stay below)

# T.81 annex K, typed in from the standard: tables K.1 / K.2 (natural order), the zig-zag order, tables K.3 - K.6
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_QUANT = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
          (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
_DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
_DC_VALS = tuple(range(12))
_AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77))
_AC_VALS = (
    (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa),
    (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa))


def quant_tables(quality: int):
    """(luminance, chrominance), 64 entries each in natural order: annex K scaled by the IJG quality rule -- ``s = 5000 / q`` below
    50, else ``200 - 2 q``; an entry is ``(t s + 50) / 100`` clamped to 1..255 -- which is what PIL reports for the same quality"""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality must be in [1, 100] (got {quality})")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((t * s + 50) // 100, 1), 255) for t in table] for table in _QUANT)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xff, marker, len(payload) + 2) + payload


def jfif_header(H: int, W: int, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
    """everything of the file before the entropy-coded segment: SOI, APP0 (JFIF 1.01, aspect 1 : 1), DQT, SOF0, DHT, DRI (one MCU
    row), SOS"""
    side = 1 if SUBSAMPLING[subsampling] == 0 else 2
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xe0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    out += _segment(0xdb, b"\x00" + bytes(ql[k] for k in _ZIGZAG) + b"\x01" + bytes(qc[k] for k in _ZIGZAG))
    out += _segment(0xc0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11 * side, 0, 2, 0x11, 1, 3, 0x11, 1]))
    out += _segment(0xc4, b"".join(bytes([cls_id]) + bytes(bits) + bytes(vals) for cls_id, bits, vals in (
        (0x00, _DC_BITS[0], _DC_VALS), (0x10, _AC_BITS[0], _AC_VALS[0]), (0x01, _DC_BITS[1], _DC_VALS), (0x11, _AC_BITS[1], _AC_VALS[1]))))
    out += _segment(0xdd, struct.pack(">H", (W + 8 * side - 1) // (8 * side)))
    out += _segment(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def _batch(E: Engine, images) -> torch.Tensor:
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
    t = t.detach()
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4 or t.shape[-1] != 3 or t.dtype != torch.uint8:
        raise ValueError(f"encode_jpeg: images must be uint8 [H, W, 3] or [n, H, W, 3] (got {t.dtype} {tuple(t.shape)})")
    return t.to(E.device).contiguous()


def jpeg_size(n: int, H: int, W: int, subsampling: str = "4:2:0", engine: Optional[Engine] = None):
    """(workspace bytes, worst-case output bytes) of one library call for n images of H x W"""
    lib = (engine or gpu()).lib
    ws, cap = C.c_int64(0), C.c_int64(0)
    lib.call("nsr_jpeg_size", int(n), int(H), int(W), SUBSAMPLING[subsampling], C.byref(ws), C.byref(cap))
    return ws.value, cap.value


def encode_jpeg(images, quality: int = 90, subsampling: str = "4:2:0", engine: Optional[Engine] = None) -> List[bytes]:
    """Complete JFIF files of a batch of images: uint8 [n, H, W, 3] (or one [H, W, 3]), tensor or array of any device, 1 <= H, W <=
    65535.  ``quality`` 1..100 as PIL counts it, ``subsampling`` "4:2:0" (PIL's default at this quality) or "4:4:4".  One library
    call for the batch (more only when its workspace would pass 2 GiB); the device is read twice per call: the offsets, then the
    used bytes."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"encode_jpeg: subsampling must be '4:2:0' or '4:4:4' (got {subsampling!r})")
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"encode_jpeg: quality must be in [1, 100] (got {quality})")
    E = engine or gpu()
    img = _batch(E, images)
    n, H, W = int(img.shape[0]), int(img.shape[1]), int(img.shape[2])
    if n == 0:
        return []
    head = jfif_header(H, W, quality, subsampling)
    ws1, cap1 = jpeg_size(1, H, W, subsampling, E)
    step = max(1, min(n, 65535, MAX_BYTES_PER_LAUNCH // max(ws1 + cap1, 1)))
    files = []
    with torch.no_grad(), E.guard():
        for k0 in range(0, n, step):
            kb = min(step, n - k0)
            nws, cap = jpeg_size(kb, H, W, subsampling, E)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=E.device)
            out = torch.empty(max(cap, 16), dtype=torch.uint8, device=E.device)
            offsets = torch.empty(kb + 1, dtype=torch.int64, device=E.device)
            E.call("nsr_jpeg_encode", img[k0:k0 + kb].data_ptr(), kb, H, W, quality, SUBSAMPLING[subsampling], ws.data_ptr(), nws,
                   out.data_ptr(), cap, offsets.data_ptr())
            off = offsets.cpu().tolist()                           # read 1: where each frame's segment lies
            if off[-1] > cap:
                raise _capi.NsrError(f"encode_jpeg: {off[-1]} bytes used of {cap}")
            data = out[:off[-1]].cpu().numpy().tobytes()           # read 2: the used bytes, not the capacity
            files += [head + data[a:b] + b"\xff\xd9" for a, b in zip(off[:-1], off[1:])]
    return files


def save_jpeg(img, path: str, quality: int = 90, subsampling: str = "4:2:0", engine: Optional[Engine] = None):
    """one uint8 [H, W, 3] image as a JPEG file"""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dim() != 3:
        raise ValueError(f"save_jpeg: one [H, W, 3] image (got {tuple(t.shape)})")
    data, = encode_jpeg(t, quality, subsampling, engine)
    with open(path, "wb") as fh:
        fh.write(data)


class MjpegWriter:
    """A Motion-JPEG video as a RIFF AVI 1.0 file: ``write`` appends one complete JPEG file of ``width`` x ``height`` as a frame,
    ``close`` writes the index and patches the sizes and the frame count (also at the end of a ``with`` block).

        RIFF 'AVI '  LIST 'hdrl' ( avih  LIST 'strl' ( strh vids/MJPG, strf BITMAPINFOHEADER ) )  LIST 'movi' ( 00dc ... )  idx1

    A frame that would take the finished file past ``MAX_BYTES`` (2^31 - 1) raises ``ValueError`` before any byte of it is written;
    the file can then still be closed and holds the frames written so far."""

    MAX_BYTES = (1 << 31) - 1
    _HEADER_BYTES = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12      # up to and including 'movi'

    def __init__(self, path: str, width: int, height: int, fps=30):
        self.width, self.height, self.fps = int(width), int(height), fps
        if self.width < 1 or self.height < 1 or not fps > 0:
            raise ValueError(f"MjpegWriter: bad size or rate ({width} x {height}, {fps} frames/s)")
        if float(fps) == int(fps):
            self.rate, self.scale = int(fps), 1
        else:
            self.rate, self.scale = int(round(float(fps) * 1000)), 1000
        self.path = path
        self.index = []                     # (offset from the 'movi' fourcc, size) per frame
        self.max_frame = 0
        self.fh = open(path, "wb")
        self.fh.write(self._header())
        self.pos = self._HEADER_BYTES

    def _header(self) -> bytes:
        n, movi = len(self.index), 4 + sum(8 + s + (s & 1) for _, s in self.index)
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        per_sec = (sum(s for _, s in self.index) * self.rate) // (self.scale * n) if n else 0
        avih = struct.pack("<14I", usec, per_sec, 0, 0x10, n, 0, 1, self.max_frame, self.width, self.height, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, self.scale, self.rate, 0, n, self.max_frame, 0xffffffff, 0,
                                               0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", 3 * self.width * self.height, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh \
            + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        total = 12 + len(hdrl) + 8 + movi + 8 + 16 * n
        out = b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi) + b"movi"
        assert len(out) == self._HEADER_BYTES
        return out

    def write(self, jpeg: bytes):
        if self.fh is None:
            raise ValueError("MjpegWriter: the file is closed")
        size = len(jpeg)
        chunk = 8 + size + (size & 1)
        if self.pos + chunk + 8 + 16 * (len(self.index) + 1) > self.MAX_BYTES:
            raise ValueError(f"MjpegWriter: {self.path} would pass {self.MAX_BYTES} bytes with this frame (AVI 1.0; OpenDML is not written)")
        self.fh.write(b"00dc" + struct.pack("<I", size) + jpeg + (b"\0" if size & 1 else b""))
        self.index.append((self.pos - (self._HEADER_BYTES - 4), size))
        self.max_frame = max(self.max_frame, size)
        self.pos += chunk

    def close(self):
        if self.fh is None:
            return
        self.fh.write(b"idx1" + struct.pack("<I", 16 * len(self.index)) + b"".join(b"00dc" + struct.pack("<III", 0x10, off, size)
                                                                                 for off, size in self.index))
        self.fh.seek(0)
        self.fh.write(self._header())
        self.fh.close()
        self.fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# --------------------------------------------------------------------------------------------------
# decoding
# --------------------------------------------------------------------------------------------------
SAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2, "grey": 3}     # the library's codes (the first three are PIL's get_sampling)
_LUMA_SAMPLING = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}
_NEXT_MARKER = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")      # the first marker in entropy-coded data that is no RSTm
_FRAME_DTYPE = np.dtype([("scan_begin", "<i8"), ("scan_end", "<i8"), ("restart_interval", "<i4"), ("reserved", "<i4"),
                         ("dc_table", "u1", 4), ("ac_table", "u1", 4), ("quant", "u1", (3, 64)), ("huff_bits", "u1", (8, 16)),
                         ("huff_vals", "u1", (8, 256))])
assert _FRAME_DTYPE.itemsize == C.sizeof(_capi.NsrJpegDecFrame)
_SOF_NAMES = {0xc1: "extended sequential (SOF1)", 0xc2: "progressive (SOF2)", 0xc3: "lossless (SOF3)", 0xc5: "hierarchical (SOF5)",
              0xc6: "hierarchical (SOF6)", 0xc7: "hierarchical (SOF7)", 0xc9: "arithmetic coding (SOF9)", 0xca: "arithmetic coding (SOF10)",
              0xcb: "arithmetic coding (SOF11)", 0xcd: "arithmetic coding (SOF13)", 0xce: "arithmetic coding (SOF14)",
              0xcf: "arithmetic coding (SOF15)", 0xcc: "arithmetic coding (DAC)"}


class _Unsupported(Exception):
    pass


def _check_huffman(cls: int, bits, vals):
    """T.81 annex C: no length holds more codes than are left (the all-ones code stays free, as libjpeg demands), and the
    symbols are as many as the counts say"""
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length) - (1 if bits[length - 1] else 0):
            raise _Unsupported(f"a Huffman table is oversubscribed at length {length}")
        code <<= 1
    if len(vals) != sum(bits) or len(vals) > 256:
        raise _Unsupported("a Huffman table's symbol count does not match its code counts")
    if cls == 0 and any(v > 15 for v in vals):
        raise _Unsupported("a DC Huffman table holds a symbol above 15")


def _parse(data: bytes) -> dict:
    """The header of a JPEG file up to its first scan: {height, width, components, sampling, restart_interval, quant [3][64],
    dc_table, ac_table, huff {(class, id): (bits, vals)}, scan_begin, scan_end}; ``_Unsupported`` for what the decoder does not take.
    The size and the sampling factors are in the exception's ``info`` when the frame header was read."""
    info = {"height": None, "width": None, "components": None, "sampling": None, "restart_interval": 0}

    def refuse(why):
        e = _Unsupported(why)
        e.info = info
        raise e

    if len(data) < 4 or data[:2] != b"\xff\xd8":
        refuse("not a JPEG file (no SOI)")
    qt, huff, sof, jfif, adobe, at = {}, {}, None, False, None, 2
    while True:
        if at + 4 > len(data):
            refuse("the file ends before a scan")
        if data[at] != 0xff:
            refuse(f"no marker at byte {at}")
        while data[at + 1] == 0xff and at + 4 < len(data):
            at += 1
        m = data[at + 1]
        if m == 0x01 or 0xd0 <= m <= 0xd8:
            at += 2
            continue
        if m == 0xd9:
            refuse("EOI before a scan")
        length = struct.unpack(">H", data[at + 2:at + 4])[0]
        seg = data[at + 4:at + 2 + length]
        if length < 2 or len(seg) != length - 2:
            refuse("a marker segment runs past the file")
        if m == 0xc0:
            if sof is not None:
                refuse("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                refuse("a malformed frame header")
            prec, h, w, nf = struct.unpack(">BHHB", seg[:6])
            sof = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)]
            info.update(height=h, width=w, components=nf)
            if prec != 8:
                refuse(f"{prec}-bit samples")
            if h == 0:
                refuse("the height comes in a DNL segment")
            if w == 0:
                refuse("a width of 0")
            if nf == 1:
                if sof[0][1:3] != (1, 1):
                    refuse(f"one component sampled {sof[0][1]}x{sof[0][2]}")
                info["sampling"] = "grey"
            elif nf == 3:
                if sof[1][1:3] != (1, 1) or sof[2][1:3] != (1, 1) or sof[0][1:3] not in _LUMA_SAMPLING:
                    refuse("sampling factors " + " ".join(f"{c[1]}x{c[2]}" for c in sof) + " (4:4:4, 4:2:2 and 4:2:0 are decoded)")
                info["sampling"] = _LUMA_SAMPLING[sof[0][1:3]]
            else:
                refuse(f"{nf} components")
        elif m in _SOF_NAMES:
            refuse(_SOF_NAMES[m])
        elif m == 0xc4:
            p = 0
            while p < len(seg):
                if p + 17 > len(seg):
                    refuse("a malformed DHT segment")
                cls, tid, bits = seg[p] >> 4, seg[p] & 15, seg[p + 1:p + 17]
                if cls > 1 or tid > 3:
                    refuse(f"Huffman table class {cls} id {tid}")
                vals = seg[p + 17:p + 17 + sum(bits)]
                try:
                    _check_huffman(cls, bits, vals)
                except _Unsupported as e:
                    refuse(str(e))
                huff[(cls, tid)] = (bits, vals)
                p += 17 + len(vals)
        elif m == 0xdb:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    refuse("a 16-bit quantisation table")
                if (seg[p] & 15) > 3 or p + 65 > len(seg):
                    refuse("a malformed DQT segment")
                qt[seg[p] & 15] = seg[p + 1:p + 65]
                p += 65
        elif m == 0xdd:
            if len(seg) != 2:
                refuse("a malformed DRI segment")
            info["restart_interval"] = struct.unpack(">H", seg)[0]
        elif m == 0xe0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xee and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xda:
            break
        at += 2 + length
    if sof is None:
        refuse("a scan before the frame header")
    nf = len(sof)
    if len(seg) < 1 or seg[0] != nf or len(seg) != 4 + 2 * nf:
        refuse("several scans (the first one does not hold every component)")
    if nf == 3 and not jfif:                       # libjpeg's rule: JFIF says YCbCr; else Adobe's transform; else the component ids
        if adobe is not None and adobe != 1:
            refuse(f"Adobe colour transform {adobe} (RGB or YCCK data)")
        if adobe is None and [c[0] for c in sof] != [1, 2, 3]:
            refuse("three components that are not marked as YCbCr")
    if tuple(seg[1 + 2 * nf:]) != (0, 63, 0):
        refuse("a scan of part of the spectrum")
    out = dict(info, quant=[], dc_table=[], ac_table=[], huff=huff)
    for i, (cid, _, _, tq) in enumerate(sof):
        if seg[1 + 2 * i] != cid:
            refuse("the scan's components are not in the frame's order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if tq not in qt or (0, td) not in huff or (1, ta) not in huff:
            refuse("a component refers to a table the file does not define")
        out["quant"].append(qt[tq])
        out["dc_table"].append(td)
        out["ac_table"].append(ta)
    begin = at + 2 + length
    hit = _NEXT_MARKER.search(data, begin)
    if hit is None:
        end = len(data)                            # no EOI: the stream is cut short, which the device reports
    else:
        end = hit.start()
        if data[end + 1] == 0xdc:
            refuse("a DNL segment")
        if data[end + 1] != 0xd9:
            refuse("several scans")
    while end > begin and data[end - 1] == 0xff:   # fill bytes before the marker
        end -= 1
    if end - begin > 1 << 28:
        refuse("a scan of more than 2^28 bytes")
    out.update(scan_begin=begin, scan_end=end)
    return out


def probe_jpeg(data: bytes) -> dict:
    """What the header of a JPEG file says: ``height``, ``width``, ``components``, ``sampling`` ("4:4:4", "4:2:2", "4:2:0", "grey";
    None for any other), ``restart_interval`` (MCUs, 0: none), and whether ``decode_jpeg`` takes the file: ``supported``, with the
    ``reason`` when it does not.  Nothing is launched."""
    try:
        p = _parse(bytes(data))
    except _Unsupported as e:
        return dict(getattr(e, "info", {}), supported=False, reason=str(e))
    return {k: p[k] for k in ("height", "width", "components", "sampling", "restart_interval")} | {"supported": True, "reason": None}


def jpegdec_size(n: int, H: int, W: int, sampling: str, max_scan_bytes: int = 0, subsequence_bytes: int = 128,
                 engine: Optional[Engine] = None) -> int:
    """workspace bytes of one library call that decodes n files of H x W"""
    ws = C.c_int64(0)
    (engine or gpu()).lib.call("nsr_jpegdec_size", int(n), int(H), int(W), SAMPLING[sampling], int(max_scan_bytes), int(subsequence_bytes),
                               C.byref(ws))
    return ws.value


def _descriptors(parsed, offsets) -> np.ndarray:
    rec = np.zeros(len(parsed), _FRAME_DTYPE)
    for k, (p, off) in enumerate(zip(parsed, offsets)):
        rec["scan_begin"][k], rec["scan_end"][k] = off + p["scan_begin"], off + p["scan_end"]
        rec["restart_interval"][k] = p["restart_interval"]
        for i in range(p["components"]):
            rec["dc_table"][k, i], rec["ac_table"][k, i] = p["dc_table"][i], p["ac_table"][i]
            rec["quant"][k, i] = np.frombuffer(p["quant"][i], np.uint8)
        for (cls, tid), (bits, vals) in p["huff"].items():
            rec["huff_bits"][k, 4 * cls + tid] = np.frombuffer(bits, np.uint8)
            rec["huff_vals"][k, 4 * cls + tid, :len(vals)] = np.frombuffer(vals, np.uint8)
    return rec


def decode_jpeg_status(files, engine: Optional[Engine] = None, subsequence_bytes: int = 128):
    """``decode_jpeg`` that hands a damaged stream back to the caller instead of raising: (u8 [n, H, W, 3] on the device, the
    frames' status words as a list).  A frame with a nonzero status has unspecified pixels (include/nsr.h names the bits)."""
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    files = [bytes(f) for f in files]
    E = engine or gpu()
    if not files:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=E.device), []
    parsed = []
    for k, f in enumerate(files):
        try:
            parsed.append(_parse(f))
        except _Unsupported as e:
            raise ValueError(f"decode_jpeg: frame {k} is not supported: {e}") from None
    H, W, sampling = parsed[0]["height"], parsed[0]["width"], parsed[0]["sampling"]
    for k, p in enumerate(parsed):
        if (p["height"], p["width"], p["sampling"]) != (H, W, sampling):
            raise ValueError(f"decode_jpeg: frame {k} is {p['height']} x {p['width']} {p['sampling']}, frame 0 is {H} x {W} {sampling}: "
                             f"the frames of one call share size and sampling")
    n = len(files)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=E.device)
    status = torch.empty(n, dtype=torch.int32, device=E.device)
    ws1 = jpegdec_size(1, H, W, sampling, 0, subsequence_bytes, E)
    step = max(1, min(n, 65535, MAX_BYTES_PER_LAUNCH // max(ws1 + 3 * H * W, 1)))
    with torch.no_grad(), E.guard():
        for k0 in range(0, n, step):
            k1 = min(k0 + step, n)
            offsets = np.cumsum([0] + [len(f) for f in files[k0:k1]])
            blob = torch.from_numpy(np.frombuffer(b"".join(files[k0:k1]), np.uint8).copy()).to(E.device)      # the files as they are
            desc = torch.from_numpy(_descriptors(parsed[k0:k1], offsets).view(np.uint8).reshape(-1)).to(E.device)
            nws = jpegdec_size(k1 - k0, H, W, sampling, max(p["scan_end"] - p["scan_begin"] for p in parsed[k0:k1]), subsequence_bytes, E)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=E.device)
            E.call("nsr_jpegdec_decode", blob.data_ptr(), desc.data_ptr(), k1 - k0, H, W, SAMPLING[sampling], int(subsequence_bytes),
                   ws.data_ptr(), nws, out[k0:k1].data_ptr(), status[k0:k1].data_ptr())
    return out, status.cpu().tolist()


def decode_jpeg(files, engine: Optional[Engine] = None, subsequence_bytes: int = 128) -> torch.Tensor:
    """u8 [n, H, W, 3] RGB on the device of n JPEG files (a list of ``bytes``, or one ``bytes`` value for n = 1): Pillow's pixels
    of ``im.convert("RGB")``, bit for bit.  One library call for the batch.  ``ValueError`` -- the message names the frame -- for a
    file the decoder does not take (``probe_jpeg`` tells why), for frames of different size or sampling in one call, and for a
    stream the device found damaged.  There is no other decoder behind this one.  ``subsequence_bytes``: the piece of the stream one
    lane decodes (a multiple of 4 in [16, 1024]); the pixels do not depend on it."""
    out, status = decode_jpeg_status(files, engine, subsequence_bytes)
    for k, st in enumerate(status):
        if st:
            raise ValueError(f"decode_jpeg: frame {k} holds a damaged stream (status {st}: "
                             + ", ".join(w for b, w in ((1, "an invalid Huffman code"), (2, "a coefficient past the block's end"),
                                                        (4, "a block count other than the header's"), (8, "restart markers out of sequence"))
                                         if st & b) + ")")
    return out


def read_jpeg(path: str, engine: Optional[Engine] = None) -> torch.Tensor:
    """u8 [H, W, 3] on the device of one JPEG file"""
    with open(path, "rb") as fh:
        return decode_jpeg(fh.read(), engine)[0]


class MjpegReader:
    """The frames of a Motion-JPEG video in a RIFF AVI file, as ``MjpegWriter`` (ffmpeg, OpenCV) writes it: the ``movi`` list is
    walked once, ``frame_bytes(i)`` is frame i's JPEG file, ``read(indices)`` decodes frames on the device, ``batch`` at a time.

        with MjpegReader("vis.avi") as video:
            print(len(video), video.width, video.height, video.fps)
            frames = video.read()                       # u8 [n, H, W, 3]
    """

    def __init__(self, path: str, engine: Optional[Engine] = None, batch: int = 16):
        self.path, self.engine, self.batch = path, engine, max(1, int(batch))
        self.fh = open(path, "rb")
        try:
            self._walk()
        except Exception:
            self.fh.close()
            self.fh = None
            raise

    def _walk(self):
        fh = self.fh
        head = fh.read(12)
        size = fh.seek(0, 2)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"MjpegReader: {self.path} is not a RIFF AVI file")
        self.index, self.width, self.height, self.fps = [], None, None, None      # index: (offset of the data, size) per frame

        def chunks(start, end):
            at = start
            while at + 8 <= end:
                fh.seek(at)
                fourcc, n = struct.unpack("<4sI", fh.read(8))
                if at + 8 + n > end:
                    raise ValueError(f"MjpegReader: {self.path}: chunk {fourcc!r} at byte {at} runs past its parent")
                yield fourcc, at + 8, n
                at += 8 + n + (n & 1)

        for fourcc, at, n in chunks(12, min(size, 8 + struct.unpack("<I", head[4:8])[0])):
            if fourcc != b"LIST":
                continue
            fh.seek(at)
            kind = fh.read(4)
            if kind == b"hdrl":
                for cc, a, m in chunks(at + 4, at + n):
                    if cc == b"avih" and m >= 40:
                        fh.seek(a)
                        v = struct.unpack("<10I", fh.read(40))
                        self.width, self.height = v[8], v[9]
                        self.fps = 1000000.0 / v[0] if v[0] else None
            elif kind == b"movi":
                for cc, a, m in chunks(at + 4, at + n):
                    if cc[2:] in (b"dc", b"db") and m > 0:
                        self.index.append((a, m))

    def __len__(self):
        return len(self.index)

    def frame_bytes(self, i: int) -> bytes:
        if self.fh is None:
            raise ValueError("MjpegReader: the file is closed")
        at, n = self.index[i]
        self.fh.seek(at)
        return self.fh.read(n)

    def read(self, indices=None) -> torch.Tensor:
        """u8 [n, H, W, 3] on the device: the frames ``indices`` (all of them by default), decoded ``batch`` files per call"""
        indices = list(range(len(self))) if indices is None else [int(i) for i in indices]
        parts = [decode_jpeg([self.frame_bytes(i) for i in indices[k:k + self.batch]], self.engine) for k in range(0, len(indices), self.batch)]
        if not parts:
            return decode_jpeg([], self.engine)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def close(self):
        if self.fh is not None:
            self.fh.close()
            self.fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def read_video(path: str, engine: Optional[Engine] = None) -> torch.Tensor:
    """u8 [n, H, W, 3] on the device: every frame of a Motion-JPEG AVI file"""
    with MjpegReader(path, engine) as video:
        return video.read()
