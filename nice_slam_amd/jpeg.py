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
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import List, Optional

import numpy as np
import torch

from . import _capi
from .engine import Engine, gpu

__all__ = ["encode_jpeg", "save_jpeg", "MjpegWriter", "quant_tables", "jfif_header", "SUBSAMPLING"]

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
