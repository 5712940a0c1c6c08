"""PNG files decoded on the GPU: the depth images of every sequence this package reads (16-bit grey) and the colour images of
the TUM RGB-D and CoFusion sequences (8-bit RGB).

    from nice_slam_amd import decode_png, read_png, probe_png
    depth = read_png("depth000000.png")                       # torch.uint16 [H, W] on the device: np.array(Image.open(f)), bit for bit
    frames = decode_png([bytes0, bytes1, ...], mode="RGB")    # u8 [n, H, W, 3]: the pixels of im.convert("RGB")
    probe_png(data)                                           # height, width, kind, and whether the decoder takes the file -- or why not

    python -m nice_slam_amd.png FILE...                       # what probe_png says about each file

The host walks the chunks, verifies every chunk's CRC (as Pillow does) and uploads the IDAT payloads -- the compressed bytes, not
the pixels; the device inflates, un-filters and orders the bytes (include/nsr.h, "PNG decoding"; csrc/nsr_png.h).  Taken: colour
type 0 at bit depth 8 or 16, colour types 2 and 6 at bit depth 8, non-interlaced.  Everything else is refused with a reason; there
is no other decoder behind ``decode_png``.

Deviations from Pillow, all deliberate: the zlib stream's trailing Adler-32 is neither verified nor required on the device (every
chunk's CRC-32 is verified, on the host, and it covers the same bytes); the window is 32 KiB whatever the zlib header declares; a
file with a ``tRNS`` chunk is refused, although Pillow reads its pixels.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import Optional

import numpy as np
import torch

from .engine import Engine, gpu

__all__ = ["probe_png", "parse_png", "pack_streams", "decode_png", "decode_png_status", "read_png", "png_size", "PngRefused", "KIND",
           "STATUS_BITS", "FRAME_DTYPE"]

SIGNATURE = b"\x89PNG\r\n\x1a\n"
KIND = {"grey8": 0, "grey16": 1, "rgb8": 2, "rgba8": 3}          # NSR_PNG_*
CHANNELS = {"grey8": 1, "grey16": 1, "rgb8": 3, "rgba8": 4}       # samples per pixel in the file
MAX_SIDE = 32768
MAX_BYTES_PER_LAUNCH = 1 << 31                                    # workspace + output of one library call (a batch is split to stay below)
STATUS_BITS = ((1, "a zlib header, block type or stored-length error"), (2, "an invalid code set or code"),
               (4, "a distance before the start of the output"), (8, "a stream that is too short or too long"), (16, "a filter type above 4"))
FRAME_DTYPE = np.dtype([("stream_begin", "<i8"), ("stream_end", "<i8")])      # nsr_png_frame


class PngRefused(ValueError):
    """a file ``decode_png`` does not take; ``info`` holds what the header said before the refusal"""


def parse_png(data: bytes) -> dict:
    """The one walk over a file's chunks, every CRC checked: ``height``, ``width``, ``kind`` and the IDAT payloads (``idat``: a list
    of byte strings) of a file the decoder takes; ``PngRefused`` with the reason for any other.  ``decode_png`` and
    ``decode_png_status`` take the result in place of the file's bytes, so a caller that has looked at a file need not have it
    walked again."""
    info = {}

    def refuse(why):
        e = PngRefused(why)
        e.info = info
        raise e

    if data[:8] != SIGNATURE:
        refuse("not a PNG file")
    at, idat, seen_idat, idat_closed, ended, first = 8, [], False, False, False, True
    while at + 12 <= len(data):
        length, ctype = struct.unpack(">I4s", data[at:at + 8])
        if at + 12 + length > len(data):
            refuse(f"chunk {ctype!r} at byte {at} runs past the end of the file")
        body = data[at + 8:at + 8 + length]
        if zlib.crc32(data[at + 4:at + 8 + length]) != struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0]:
            refuse(f"chunk {ctype!r} at byte {at} has a bad CRC")
        at += 12 + length
        if first:
            if ctype != b"IHDR" or length != 13:
                refuse("the first chunk is not IHDR")
            first = False
            W, H, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", body)
            info.update(height=H, width=W, kind=None, bit_depth=depth, colour_type=colour)
            if H < 1 or W < 1 or H > MAX_SIDE or W > MAX_SIDE:
                refuse(f"an image of {H} x {W} (sizes are in [1, {MAX_SIDE}])")
            if compression != 0 or filt != 0:
                refuse(f"compression method {compression}, filter method {filt}")
            if interlace != 0:
                refuse("an interlaced file (Adam7)")
            if colour == 3:
                refuse("a palette image")
            if colour == 4:
                refuse("grey + alpha")
            if colour not in (0, 2, 6):
                refuse(f"colour type {colour}")
            if depth in (1, 2, 4):
                refuse(f"bit depth {depth}")
            if depth == 16 and colour != 0:
                refuse("16-bit colour")
            if depth not in (8, 16):
                refuse(f"bit depth {depth}")
            info["kind"] = {(0, 8): "grey8", (0, 16): "grey16", (2, 8): "rgb8", (6, 8): "rgba8"}[(colour, depth)]
            continue
        if ctype == b"IDAT":
            if idat_closed:
                refuse("IDAT chunks that are not consecutive")
            seen_idat = True
            idat.append(body)
            continue
        if seen_idat:
            idat_closed = True
        if ctype == b"tRNS":
            refuse("a tRNS chunk (transparency)")
        if ctype == b"acTL":
            refuse("an animated PNG (acTL)")
        if ctype == b"IEND":
            ended = True
            break
    if first:
        refuse("no IHDR chunk")
    if not seen_idat:
        refuse("no IDAT chunk")
    if not ended:
        refuse("no IEND chunk")
    return dict(info, idat=idat)


def probe_png(data: bytes) -> dict:
    """What the chunks of a PNG file say: ``height``, ``width``, ``kind`` ("grey8", "grey16", "rgb8", "rgba8"; None for any other),
    and whether ``decode_png`` takes the file: ``supported``, with the ``reason`` when it does not.  Every chunk's CRC is checked;
    nothing is launched."""
    try:
        p = parse_png(bytes(data))
    except PngRefused as e:
        info = getattr(e, "info", {})
        return {"height": info.get("height"), "width": info.get("width"), "kind": info.get("kind"), "supported": False, "reason": str(e)}
    return {"height": p["height"], "width": p["width"], "kind": p["kind"], "supported": True, "reason": None}


def png_size(n: int, H: int, W: int, kind: str, engine: Optional[Engine] = None) -> int:
    """workspace bytes of one library call that decodes n files of H x W"""
    ws = C.c_int64(0)
    (engine or gpu()).lib.call("nsr_png_size", int(n), int(H), int(W), KIND[kind], C.byref(ws))
    return ws.value


def pack_streams(parsed, gap: int = 0):
    """(blob, descriptors) of parsed files as ``nsr_png_decode`` reads them: the files' zlib streams -- their IDAT payloads,
    concatenated -- one behind the other in ``blob`` (bytes), and a ``FRAME_DTYPE`` record per file with its stream's byte range.
    ``gap``: bytes of 0xFF before every stream and behind the last (a stream's neighbours, for a caller that checks that no fetch
    leaves a range)."""
    streams = [b"".join(p["idat"]) for p in parsed]
    desc = np.zeros(len(streams), FRAME_DTYPE)
    ends = np.cumsum([gap + len(s) for s in streams]) if streams else np.zeros(0, np.int64)
    desc["stream_end"], desc["stream_begin"] = ends, ends - np.array([len(s) for s in streams], np.int64)
    return b"".join(b"\xff" * gap + s for s in streams) + b"\xff" * gap, desc


def _out_form(kind: str, mode: Optional[str]):
    """(out_channels, shape behind [n, H, W], 16 bit?) of a kind in a mode"""
    if mode not in (None, "RGB"):
        raise ValueError(f"decode_png: mode must be None or 'RGB' (got {mode!r})")
    if mode == "RGB":
        if kind == "grey16":
            raise ValueError("decode_png: a 16-bit file has no RGB form")
        return 3, (3,), False
    return CHANNELS[kind], () if CHANNELS[kind] == 1 else (CHANNELS[kind],), kind == "grey16"


def decode_png_status(files, mode: Optional[str] = None, engine: Optional[Engine] = None):
    """``decode_png`` that hands a damaged stream back to the caller instead of raising: (the pixels on the device, the frames'
    status words as a list).  ``files``: the files' bytes, or what ``parse_png`` returned for them.  A frame with a nonzero status has unspecified pixels (``STATUS_BITS``, include/nsr.h)."""
    if isinstance(files, (bytes, bytearray, memoryview)):
        files = [files]
    if isinstance(files, dict):
        files = [files]
    E = engine or gpu()
    if not files:
        return torch.empty((0, 0, 0), dtype=torch.uint8, device=E.device), []
    parsed = []
    for k, f in enumerate(files):
        try:
            parsed.append(f if isinstance(f, dict) else parse_png(bytes(f)))      # (a dict: parse_png's, the walk already done)
        except PngRefused as e:
            raise ValueError(f"decode_png: frame {k} is not supported: {e}") from None
    H, W, kind = parsed[0]["height"], parsed[0]["width"], parsed[0]["kind"]
    for k, p in enumerate(parsed):
        if (p["height"], p["width"], p["kind"]) != (H, W, kind):
            raise ValueError(f"decode_png: frame {k} is {p['height']} x {p['width']} {p['kind']}, frame 0 is {H} x {W} {kind}: "
                             f"the frames of one call share size and kind")
    oc, tail, wide = _out_form(kind, mode)
    n = len(files)
    out = torch.empty((n, H, W) + tail, dtype=torch.int16 if wide else torch.uint8, device=E.device)
    status = torch.empty(n, dtype=torch.int32, device=E.device)
    ws1 = png_size(1, H, W, kind, E)
    step = max(1, min(n, 65535, MAX_BYTES_PER_LAUNCH // max(ws1 + H * W * oc * (2 if wide else 1), 1)))
    with torch.no_grad(), E.guard():
        for k0 in range(0, n, step):
            k1 = min(k0 + step, n)
            streams, desc = pack_streams(parsed[k0:k1])
            blob = torch.from_numpy(np.frombuffer(streams or b"\0", np.uint8).copy()).to(E.device)     # the compressed bytes
            dev_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1)).to(E.device)
            nws = png_size(k1 - k0, H, W, kind, E)
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=E.device)
            E.call("nsr_png_decode", blob.data_ptr(), dev_desc.data_ptr(), k1 - k0, H, W, KIND[kind], oc, ws.data_ptr(), nws,
                   out[k0:k1].data_ptr(), status[k0:k1].data_ptr())
    if wide:
        out = out.view(torch.uint16)
    return out, status.cpu().tolist()


def decode_png(files, mode: Optional[str] = None, engine: Optional[Engine] = None) -> torch.Tensor:
    """The pixels of n PNG files (a list of ``bytes``, or one ``bytes`` value for n = 1) on the device, bit for bit Pillow's.
    ``mode=None``: ``np.array(Image.open(f))`` -- u8 [n, H, W] (8-bit grey), ``torch.uint16`` [n, H, W] (16-bit grey), u8 [n, H, W, 3]
    (RGB), u8 [n, H, W, 4] (RGBA); ``mode="RGB"``: u8 [n, H, W, 3] of ``im.convert("RGB")`` (grey three times, alpha dropped; not for
    a 16-bit file).  One library call for the batch; only the status words come back to the host.  ``ValueError`` -- the message
    names the frame -- for a file the decoder does not take (``probe_png`` tells why), for frames of different size or kind in one
    call, and for a stream the device found damaged.  There is no other decoder behind this one."""
    out, status = decode_png_status(files, mode, engine)
    for k, st in enumerate(status):
        if st:
            raise ValueError(f"decode_png: frame {k} holds a damaged stream (status {st}: " + ", ".join(w for b, w in STATUS_BITS if st & b) + ")")
    return out


def read_png(path: str, mode: Optional[str] = None, engine: Optional[Engine] = None) -> torch.Tensor:
    """the pixels of one PNG file on the device ([H, W] or [H, W, C], see ``decode_png``)"""
    with open(path, "rb") as fh:
        return decode_png(fh.read(), mode, engine)[0]


def _main(argv) -> int:
    if not argv:
        print("usage: python -m nice_slam_amd.png FILE...")
        return 2
    for path in argv:
        with open(path, "rb") as fh:
            p = probe_png(fh.read())
        what = f"{p['height']} x {p['width']} {p['kind'] or ''}".strip() if p["height"] is not None else "?"
        print(f"{path}: {what}: " + ("supported" if p["supported"] else f"refused: {p['reason']}"))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(_main(sys.argv[1:]))
