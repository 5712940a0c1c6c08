"""TEST INFRASTRUCTURE for the PNG decoder (nice_slam_amd/csrc/nsr_png.h, nice_slam_amd/png.py): a PNG writer that builds files by
hand -- a chosen filter type per row, zlib's level and strategy, Z_FULL_FLUSH points, the stream cut into IDAT chunks of a given
size --, a plain-Python restatement of inflate that also records what the stream held (so that a test can assert that a case
exercises the path it is there for), a bit writer for the streams zlib itself would never emit, and the shared cases."""
import io
import struct
import zlib

import numpy as np
from PIL import Image

SIGNATURE = b"\x89PNG\r\n\x1a\n"
KINDS = ("grey16", "grey8", "rgb8", "rgba8")
COLOUR_TYPE = {"grey8": (0, 8), "grey16": (0, 16), "rgb8": (2, 8), "rgba8": (6, 8)}
BPP = {"grey8": 1, "grey16": 2, "rgb8": 3, "rgba8": 4}
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- pixels ------------------------------------------------------------------------------------------------------------------------
def kind_of(pixels: np.ndarray) -> str:
    if pixels.ndim == 2:
        return "grey16" if pixels.dtype == np.uint16 else "grey8"
    return {3: "rgb8", 4: "rgba8"}[pixels.shape[2]]


def image(kind: str, H: int, W: int, seed: int = 0, smooth: bool = True) -> np.ndarray:
    """a ramp plus small noise (so that every filter type leaves different bytes), or plain noise"""
    rng = np.random.default_rng(seed)
    tail = () if kind.startswith("grey") else (BPP[kind],)
    top = 65536 if kind == "grey16" else 256
    if smooth:
        y, x = np.mgrid[0:H, 0:W]
        base = (y * 37 + x * 101 + seed * 13)[(...,) + (None,) * len(tail)] * (top // 256) + rng.integers(0, 5, (H, W) + tail)
        return (base % top).astype(np.uint16 if kind == "grey16" else np.uint8)
    return rng.integers(0, top, (H, W) + tail).astype(np.uint16 if kind == "grey16" else np.uint8)


def scanlines(pixels: np.ndarray) -> np.ndarray:
    """u8 [H, stride]: the samples in PNG's order (16 bit: big-endian)"""
    H = pixels.shape[0]
    if pixels.dtype == np.uint16:
        return pixels.astype(">u2").view(np.uint8).reshape(H, -1)
    return np.ascontiguousarray(pixels).reshape(H, -1)


def filter_rows(raw: np.ndarray, bpp: int, types) -> bytes:
    """the filtered scanlines (PNG specification, section 9), a filter-type byte before each row"""
    H, stride = raw.shape
    out = bytearray()
    prev = np.zeros(stride, np.int32)
    for r in range(H):
        cur = raw[r].astype(np.int32)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if stride > bpp else np.zeros(stride, np.int32)
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if stride > bpp else np.zeros(stride, np.int32)
        b, t = prev, int(types[r])
        if t == 1:
            pred = a
        elif t == 2:
            pred = b
        elif t == 3:
            pred = (a + b) >> 1
        elif t == 4:
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:                                    # 0, and a type the specification does not know: the bytes as they are
            pred = np.zeros(stride, np.int32)
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def filter_types(H: int, how, seed: int = 0):
    """`how`: 0..4 (that type on every row), "mix" (rotating), "random" (seeded)"""
    if how == "mix":
        return [r % 5 for r in range(H)]
    if how == "random":
        return np.random.default_rng(seed).integers(0, 5, H).tolist()
    return [int(how)] * H


# ---- files -------------------------------------------------------------------------------------------------------------------------
def chunk(ctype: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + ctype + body + struct.pack(">I", zlib.crc32(ctype + body))


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = b""
    for k in range(0, len(data), flush_every):
        out += co.compress(data[k:k + flush_every]) + co.flush(zlib.Z_FULL_FLUSH)
    return out + co.flush()


def png_file(H: int, W: int, kind: str, stream: bytes, idat_bytes=None, extra=(), colour=None, depth=None, interlace=0) -> bytes:
    """a file around a zlib stream; `extra`: chunks between IHDR and the first IDAT"""
    ct, bd = COLOUR_TYPE[kind]
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bd if depth is None else depth, ct if colour is None else colour, 0, 0, interlace))
    for ctype, body in extra:
        out += chunk(ctype, body)
    step = idat_bytes or max(len(stream), 1)
    for k in range(0, max(len(stream), 1), step):
        out += chunk(b"IDAT", stream[k:k + step])
    return out + chunk(b"IEND", b"")


def write_png(pixels: np.ndarray, filters=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None, idat_bytes=None, seed=0,
              ihdr_height=None) -> bytes:
    """the file of `pixels` with the filter types `filters` (filter_types' `how`, or a list), compressed as asked"""
    kind = kind_of(pixels)
    H, W = pixels.shape[:2]
    types = filters if isinstance(filters, (list, tuple)) else filter_types(H, filters, seed)
    data = filter_rows(scanlines(pixels), BPP[kind], types)
    return png_file(H if ihdr_height is None else ihdr_height, W, kind, deflate(data, level, strategy, flush_every), idat_bytes)


def pil_save(pixels: np.ndarray, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "PNG", **kw)
    return buf.getvalue()


def pil_pixels(data: bytes, mode=None) -> np.ndarray:
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im if mode is None else im.convert(mode))


def zlib_stream(data: bytes) -> bytes:
    """the concatenated IDAT payloads of a file (no CRC check: the test files' own chunks)"""
    at, out = 8, b""
    while at < len(data):
        n, ctype = struct.unpack(">I4s", data[at:at + 8])
        if ctype == b"IDAT":
            out += data[at + 8:at + 8 + n]
        at += 12 + n
    return out


def replace_stream(data: bytes, stream: bytes) -> bytes:
    """the file with another zlib stream in one IDAT chunk"""
    W, H, bd, ct = struct.unpack(">IIBB", data[16:26])
    kind = {v: k for k, v in COLOUR_TYPE.items()}[(ct, bd)]
    return png_file(H, W, kind, stream)


# ---- inflate, restated -------------------------------------------------------------------------------------------------------------
class InflateError(ValueError):
    pass


class _Bits:
    def __init__(self, data: bytes, at: int = 0):
        self.data, self.pos = data, 8 * at

    def take(self, n: int) -> int:
        v = 0
        for k in range(n):
            byte = self.pos >> 3
            if byte >= len(self.data):
                raise InflateError("the stream ends early")
            v |= ((self.data[byte] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _table(lengths, complete_only=False):
    """{(length, code): symbol} of a canonical code; zlib's inflate_table rules for the sets it refuses"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    left, mx = 1, max(lengths) if lengths else 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise InflateError("over-subscribed code set")
    if mx and left > 0 and (complete_only or mx != 1):
        raise InflateError("incomplete code set")
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1] * (l > 1)) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def _symbol(bits: _Bits, table) -> tuple:
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)
        if (l, code) in table:
            return table[(l, code)], l
    raise InflateError("invalid code")


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def inflate(stream: bytes, limit: int = 1 << 26):
    """(the bytes, the record) of a zlib stream: RFC 1950 / 1951 as zlib's inflate reads them.  The record: `blocks` (the BTYPE of
    every block), `empty_stored`, `longest_litlen_code`, `longest_dist_code`, `largest_distance`, `largest_length`, `overlapped`
    (a copy with distance < length), `single_dist_code` (a block whose distance set is one code of length 1)."""
    rec = dict(blocks=[], empty_stored=0, longest_litlen_code=0, longest_dist_code=0, largest_distance=0, largest_length=0,
               overlapped=False, single_dist_code=False)
    if len(stream) < 2:
        raise InflateError("the stream ends early")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 32 or (cmf << 8 | flg) % 31:
        raise InflateError("zlib header")
    bits, out = _Bits(stream, 2), bytearray()
    while True:
        last, btype = bits.take(1), bits.take(2)
        rec["blocks"].append(btype)
        if btype == 3:
            raise InflateError("block type 3")
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            n, nn = bits.take(16), bits.take(16)
            if n ^ nn != 0xffff:
                raise InflateError("stored length")
            at = bits.pos >> 3
            if at + n > len(stream):
                raise InflateError("the stream ends early")
            out += stream[at:at + n]
            bits.pos += 8 * n
            rec["empty_stored"] += n == 0
        else:
            if btype == 1:
                lit, dist = _table(FIXED_LIT), _table(FIXED_DIST)
            else:
                nlen, ndist, ncode = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise InflateError("too many length or distance symbols")
                cl = [0] * 19
                for k in range(ncode):
                    cl[CL_ORDER[k]] = bits.take(3)
                clt = _table(cl, complete_only=True)
                lens = []
                while len(lens) < nlen + ndist:
                    s, _ = _symbol(bits, clt)
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise InflateError("repeat without a length before it")
                        val, rep = lens[-1], 3 + bits.take(2)
                    elif s == 17:
                        val, rep = 0, 3 + bits.take(3)
                    else:
                        val, rep = 0, 11 + bits.take(7)
                    if len(lens) + rep > nlen + ndist:
                        raise InflateError("repeat past the last length")
                    lens += [val] * rep
                if lens[256] == 0:
                    raise InflateError("missing end-of-block code")
                lit, dist = _table(lens[:nlen]), _table(lens[nlen:])
                rec["single_dist_code"] |= sorted(lens[nlen:])[-2:] in ([0, 1], [1])
            while True:
                s, l = _symbol(bits, lit)
                rec["longest_litlen_code"] = max(rec["longest_litlen_code"], l)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise InflateError("invalid literal/length code")
                    c = s - 257
                    length = 258 if c == 28 else (3 + c if c < 8 else 3 + ((4 + (c & 3)) << ((c >> 2) - 1)) + bits.take((c >> 2) - 1))
                    d, l = _symbol(bits, dist)
                    rec["longest_dist_code"] = max(rec["longest_dist_code"], l)
                    if d > 29:
                        raise InflateError("invalid distance code")
                    distance = 1 + d if d < 4 else 1 + ((2 + (d & 1)) << ((d >> 1) - 1)) + bits.take((d >> 1) - 1)
                    if distance > len(out):
                        raise InflateError("distance too far back")
                    rec["largest_distance"] = max(rec["largest_distance"], distance)
                    rec["largest_length"] = max(rec["largest_length"], length)
                    rec["overlapped"] |= distance < length
                    for _ in range(length):
                        out.append(out[-distance])
                if len(out) > limit:
                    raise InflateError("output limit")
        if last:
            return bytes(out), rec


# ---- streams zlib would not write ------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value: int, nbits: int):
        """`nbits` of `value`, least significant first (header fields, extra bits)"""
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int):
        """a Huffman code: most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _codes(lengths):
    return {s: (c, l) for (l, c), s in _table(lengths).items()}


def fixed_stream(symbols) -> bytes:
    """a zlib stream of one fixed block: `symbols` are literals (ints) or (length 3..10, distance 1..4) pairs, then end-of-block"""
    w, lit = BitWriter(), _codes(FIXED_LIT)
    w.put(0x78, 8)
    w.put(0x01, 8)
    w.put(1, 1)
    w.put(1, 2)
    for s in symbols:
        if isinstance(s, tuple):
            length, distance = s
            assert 3 <= length <= 10 and 1 <= distance <= 4
            w.code(*lit[257 + length - 3])
            w.code(distance - 1, 5)
        else:
            w.code(*lit[s])
    w.code(*lit[256])
    return w.done() + bytes(8)


def dynamic_stream(litlens, distlens, symbols=(), cl_lengths=None, end=True) -> bytes:
    """a zlib stream of one dynamic block whose header spells the lengths out one by one (no repeat codes); the code-length alphabet
    is 0..15 at 5 bits, 16 at 2, 17 and 18 at 3 (complete), or `cl_lengths`.  `symbols`: literals, or (3, distance symbol) pairs."""
    w = BitWriter()
    w.put(0x78, 8)
    w.put(0x01, 8)
    w.put(1, 1)
    w.put(2, 2)
    w.put(len(litlens) - 257, 5)
    w.put(len(distlens) - 1, 5)
    w.put(19 - 4, 4)
    cl = list(cl_lengths) if cl_lengths is not None else [5] * 16 + [2, 3, 3]
    for s in CL_ORDER:
        w.put(cl[s], 3)
    try:
        clc = _codes(cl)
    except InflateError:
        return w.done() + bytes(8)                 # (the set is the damage: nothing behind it is read)
    for l in list(litlens) + list(distlens):
        w.code(*clc[l])
    if litlens[256] if len(litlens) > 256 else 0:
        lit, dist = _codes(list(litlens)), _codes(list(distlens))
        for s in symbols:
            if isinstance(s, tuple):
                assert s[0] == 3
                w.code(*lit[257])
                w.code(*dist[s[1]])
            else:
                w.code(*lit[s])
        if end:
            w.code(*lit[256])
    return w.done() + bytes(8)


def seal(stream: bytes) -> bytes:
    """a hand-written stream (fixed_stream, dynamic_stream: eight zero bytes at the end) with its Adler-32 in their place"""
    return stream[:-8] + struct.pack(">I", zlib.adler32(inflate(stream)[0]))


# ---- the deflate cases -------------------------------------------------------------------------------------------------------------
def fibonacci_bytes(values: int = 22, seed: int = 3) -> np.ndarray:
    """bytes whose `values` values have Fibonacci-weighted frequencies, shuffled: a Huffman code as deep as a code can get"""
    fib = [1, 1]
    while len(fib) < values:
        fib.append(fib[-1] + fib[-2])
    data = np.repeat(np.arange(values, dtype=np.uint8) * 11 + 1, fib)
    np.random.default_rng(seed).shuffle(data)
    return data


def deflate_cases():
    """{name: file}; tests/test_png_emu.py::test_deflate_cases_have_their_property says what each is there for"""
    small = image("grey16", 13, 17, seed=1)
    rng = np.random.default_rng(7)
    ramp = ((np.add.outer(np.arange(64), np.arange(64)) * 40 + rng.integers(0, 7, (64, 64))) % 65536).astype(np.uint16)
    constant = image("grey16", 60, 40, seed=2, smooth=False)
    constant[10:50] = 0                                            # 40 x 40 pixels, and the rows' filter bytes: one run of zeros
    few = (image("grey16", 13, 17, seed=1, smooth=False) % 23).astype(np.uint16)      # few values: Huffman coding pays without matches
    far = image("grey16", 40, 1000, seed=3, smooth=False)
    far[16] = far[0]
    fib = fibonacci_bytes()
    deep = fib[:len(fib) // 41 * 41].reshape(-1, 41)              # 1130 rows of 41 grey8 pixels
    return {"stored": write_png(small, "mix", level=0),
            "stored_two_blocks": write_png(image("grey16", 200, 200, seed=4), 0, level=0),
            "fixed": write_png(small, "mix", strategy=zlib.Z_FIXED),
            "dynamic": write_png(ramp, "mix", level=9),
            "huffman_only": write_png(few, 0, strategy=zlib.Z_HUFFMAN_ONLY),
            # (zlib's deflate never leaves a distance set of one code: written by hand -- 3 x 7 grey8, rows of filter type 0)
            "single_distance_code": png_file(3, 7, "grey8", seal(dynamic_stream([8] * 254 + [0, 0, 8, 8], [1],
                                             [0, 5, (3, 0), 9, 9, 9, 0, 1, 2, 3, 4, 5, 6, 7, 0, 7, (3, 0), (3, 0)]))),
            "rle": write_png(constant, 0, strategy=zlib.Z_RLE),
            "full_flush": write_png(small, "mix", flush_every=50),
            "fixed_flushed": write_png(small, "mix", strategy=zlib.Z_FIXED, flush_every=50),
            "idat_7": write_png(small, "mix", idat_bytes=7),
            "window_end": write_png(far, 0, level=9),
            "long_codes": write_png(deep, 0, strategy=zlib.Z_HUFFMAN_ONLY),
            "pil_saved": pil_save(np.random.default_rng(4).integers(0, 6000, (34, 50)).astype(np.uint16))}


# ---- the damaged streams -----------------------------------------------------------------------------------------------------------
def damaged_cases():
    """{name: (file, status bits of which at least one must be set)}: 13 x 17 grey16 files the host parser takes, whose stream or
    scanlines are wrong"""
    px = image("grey16", 13, 17, seed=5)
    good = write_png(px, "mix", level=9)
    stream = zlib_stream(good)
    out = {"truncated": (replace_stream(good, stream[:len(stream) // 3]), 8)}
    stored = bytearray(zlib_stream(write_png(px, "mix", level=0)))
    stored[5] ^= 0x10                                              # NLEN's low byte (header 2, block header 1, LEN 2)
    out["stored_length"] = (replace_stream(good, bytes(stored)), 1)
    out["block_type_3"] = (replace_stream(good, b"\x78\x01\x07" + bytes(16)), 1)
    out["distance_before_start"] = (replace_stream(good, fixed_stream([65, 66, (4, 3)] + [0] * 40)), 4)
    out["oversubscribed"] = (replace_stream(good, dynamic_stream([8] * 256 + [1], [1], cl_lengths=[1] * 19)), 2)
    dyn = bytearray(zlib_stream(write_png(image("grey16", 64, 64, seed=6), "mix", level=9)))
    dyn[2] = (dyn[2] & 7) | (30 << 3)                              # HLIT = 30: 287 literal/length codes
    out["hlit_287"] = (png_file(64, 64, "grey16", bytes(dyn)), 2)
    out["no_end_of_block"] = (replace_stream(good, dynamic_stream([8] * 256 + [0], [1])), 2)
    out["row_too_long"] = (write_png(image("grey16", 14, 17, seed=5), "mix", level=9, ihdr_height=13), 8)
    out["row_too_short"] = (write_png(image("grey16", 12, 17, seed=5), "mix", level=9, ihdr_height=13), 8)
    out["filter_5"] = (write_png(px, [0, 1, 2, 5, 4] + [0] * 8, level=9), 16)
    return good, out


# ---- sequence folders --------------------------------------------------------------------------------------------------------------
def replica_folder(root: str, n: int = 3):
    """a Replica-layout folder: JPEG colour, 16-bit PNG depth as Pillow saves it; returns its config"""
    import os
    os.makedirs(os.path.join(root, "results"))
    rng = np.random.default_rng(4)
    for k in range(n):
        Image.fromarray(image("rgb8", 34, 50, seed=k)).save(os.path.join(root, "results", f"frame{k:06d}.jpg"), quality=90)
        Image.fromarray(rng.integers(0, 6000, (34, 50)).astype(np.uint16)).save(os.path.join(root, "results", f"depth{k:06d}.png"))
    with open(os.path.join(root, "traj.txt"), "w") as fh:
        for k in range(n):
            m = np.eye(4)
            m[:3, 3] = (0.1 * k, 0.2, 0.3)
            fh.write(" ".join(repr(float(v)) for v in m.reshape(-1)) + "\n")
    return {"dataset": "replica", "scale": 1.0, "data": {"input_folder": root},
            "cam": {"H": 34, "W": 50, "fx": 40.0, "fy": 40.0, "cx": 24.5, "cy": 16.5, "png_depth_scale": 1000.0, "crop_edge": 2}}


def tum_folder(root: str, n: int = 3, palette_at=None):
    """a folder in the TUM RGB-D layout: PNG colour (RGB; frame `palette_at` as a palette image) and 16-bit PNG depth, one pose
    per frame, timestamps a tenth of a second apart (every frame is kept); returns its config"""
    import os
    os.makedirs(os.path.join(root, "rgb"))
    os.makedirs(os.path.join(root, "depth"))
    rng = np.random.default_rng(8)
    with open(os.path.join(root, "rgb.txt"), "w") as fc, open(os.path.join(root, "depth.txt"), "w") as fd, \
            open(os.path.join(root, "groundtruth.txt"), "w") as fp:
        for f in (fc, fd, fp):
            f.write("# hand made\n# hand made\n# timestamp ...\n")
        for k in range(n):
            t = 100.0 + 0.1 * k
            im = Image.fromarray(image("rgb8", 30, 42, seed=10 + k))
            if k == palette_at:
                im = im.quantize(16)
            im.save(os.path.join(root, "rgb", f"{t:.6f}.png"))
            Image.fromarray(rng.integers(0, 30000, (30, 42)).astype(np.uint16)).save(os.path.join(root, "depth", f"{t:.6f}.png"))
            fc.write(f"{t:.6f} rgb/{t:.6f}.png\n")
            fd.write(f"{t:.6f} depth/{t:.6f}.png\n")
            fp.write(f"{t:.6f} {0.1 * k} 0.2 0.3 0 0 0 1\n")
    return {"dataset": "tumrgbd", "scale": 1.0, "data": {"input_folder": root},
            "cam": {"H": 30, "W": 42, "fx": 35.0, "fy": 35.0, "cx": 20.5, "cy": 14.5, "png_depth_scale": 5000.0, "crop_edge": 1}}
