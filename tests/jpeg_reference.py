"""TEST INFRASTRUCTURE: the JPEG encoder of nice_slam_amd/csrc/nsr_jpeg.h restated in numpy, operation for operation (the same
integers at the same rounding points, so the same bytes), the seeded test images, and a small RIFF walker for the AVI files of
``nice_slam_amd.jpeg.MjpegWriter``.  Nothing here imports the package.

    encode(img, quality, subsampling) -> bytes        a complete JFIF file of one u8 [H, W, 3] image
    entropy_segment(data) -> bytes                    what stands between a file's SOS header and its EOI
    walk_avi(data) -> dict                            the chunks of a RIFF AVI file, sizes checked against the file's length
"""
import struct

import numpy as np

# ---- T.81 annex K, typed in from the standard ----
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
QUANT_LUM = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                        + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = list(range(12))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa])

SUBSAMPLING = {"4:4:4": 1, "4:2:0": 2}            # the MCU's side in blocks


def quant_tables(quality: int):
    """(luminance, chrominance) int64 [64] in natural order: annex K scaled by the IJG rule"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (QUANT_LUM, QUANT_CHROMA))


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a table given as counts per length and symbols in code order (T.81 annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def dct_matrix():
    """M[u][x] = round(8192 a(u) cos((2 x + 1) u pi / 16)) as integers: 2896 in row 0, +-round(4096 cos(k pi / 16)) elsewhere"""
    cos = [4096, 4017, 3784, 3406, 2896, 2276, 1567, 799]        # k = 0..7, typed in as in the header
    M = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            k = ((2 * x + 1) * u) % 32                           # cos(k pi / 16) folded into k = 0..8
            sign = 1
            if k > 16:
                k = 32 - k
            if k > 8:
                k, sign = 16 - k, -1
            M[u, x] = 2896 if u == 0 else (0 if k == 8 else sign * cos[k])
    assert np.array_equal(M, np.rint(8192 * np.where(np.arange(8) == 0, np.sqrt(1 / 8), 0.5)[:, None]
                                     * np.cos((2 * np.arange(8)[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)).astype(np.int64))
    return M


def components(img):
    """int64 [3, H, W]: Y, Cb, Cr of u8 [H, W, 3] by the 16-bit constants"""
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16])


def coefficients(img, quality: int, subsampling: str):
    """(int64 [MCU rows, MCUs, blocks per MCU, 64], bool [MCU rows, MCUs, blocks per MCU]): the quantised coefficients in zig-zag
    order, interleaved scan order, and which blocks are dummies: the Y blocks of a 4:2:0 MCU that hold no pixel of the image"""
    S = SUBSAMPLING[subsampling]
    H, W = img.shape[:2]
    side = 8 * S
    my, mx = -(-H // side), -(-W // side)
    ycc = components(img)
    ycc = ycc[:, np.minimum(np.arange(my * side), H - 1)][:, :, np.minimum(np.arange(mx * side), W - 1)]       # edge replication
    planes = [ycc[0]]
    for c in (1, 2):
        p = ycc[c]
        planes.append(p if S == 1 else (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2)
    M = dct_matrix()
    ql, qc = (q[ZIGZAG] for q in quant_tables(quality))
    out = np.zeros((my, mx, 3 if S == 1 else 6, 64), np.int64)

    def blocks(plane, q):
        h, w = plane.shape
        s = (plane - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)          # [by, bx, y, x]
        t = (np.einsum("ux,byzx->byzu", M, s) + 512) >> 10                              # rows: t[y][u]
        F = np.einsum("vy,bzyu->bzvu", M, t).reshape(h // 8, w // 8, 64)[..., ZIGZAG]   # columns: F[v][u]
        d = q << 16
        c = (np.abs(F) + (d >> 1)) // d
        c[..., 1:] = np.minimum(c[..., 1:], 1023)
        return np.where(F < 0, -c, c)

    yb = blocks(planes[0], ql)
    if S == 1:
        out[:, :, 0] = yb
    else:
        for k in range(4):
            out[:, :, k] = yb[(k >> 1)::2, (k & 1)::2]
    out[:, :, -2] = blocks(planes[1], qc)
    out[:, :, -1] = blocks(planes[2], qc)
    dummy = np.zeros(out.shape[:3], bool)
    if S == 2:
        for k in range(4):
            dummy[:, :, k] = (16 * np.arange(mx)[None, :] + 8 * (k & 1) >= W) | (16 * np.arange(my)[:, None] + 8 * (k >> 1) >= H)
    return out, dummy


def _nbits(a: int) -> int:
    return int(a).bit_length()


def entropy_code(coef, dummy):
    """the entropy-coded segment of one frame's coefficients: one restart interval per MCU row, byte-stuffed, RSTm between; a dummy
    block is the DC value of the Y block before it and no AC (libjpeg's dummy blocks)"""
    dc = [huff_codes(DC_BITS[i], DC_VALS) for i in range(2)]
    ac = [huff_codes(AC_BITS[i], AC_VALS[i]) for i in range(2)]
    my, mx, bpm, _ = coef.shape
    out = bytearray()
    for r in range(my):
        acc, n = 0, 0
        pred = [0, 0, 0]
        for m in range(mx):
            for k in range(bpm):
                comp = 0 if k < bpm - 2 else k - (bpm - 3)
                t = 1 if comp else 0
                c = [pred[0]] + [0] * 63 if dummy[r, m, k] else [int(v) for v in coef[r, m, k]]
                diff = c[0] - pred[comp]
                pred[comp] = c[0]
                nb = _nbits(abs(diff))
                code, ln = dc[t][nb]
                acc, n = (acc << (ln + nb)) | (code << nb) | ((diff - 1 if diff < 0 else diff) & ((1 << nb) - 1)), n + ln + nb
                run = 0
                for v in c[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        code, ln = ac[t][0xf0]
                        acc, n = (acc << ln) | code, n + ln
                        run -= 16
                    nb = _nbits(abs(v))
                    code, ln = ac[t][run << 4 | nb]
                    acc, n = (acc << (ln + nb)) | (code << nb) | ((v - 1 if v < 0 else v) & ((1 << nb) - 1)), n + ln + nb
                    run = 0
                if run > 0:
                    code, ln = ac[t][0]
                    acc, n = (acc << ln) | code, n + ln
        pad = -n % 8
        acc, n = (acc << pad) | ((1 << pad) - 1), n + pad
        out += acc.to_bytes(n // 8, "big").replace(b"\xff", b"\xff\x00")
        if r < my - 1:
            out += bytes([0xff, 0xd0 + (r & 7)])
    return bytes(out)


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xff, marker, len(payload) + 2) + payload


def header(H: int, W: int, quality: int, subsampling: str) -> bytes:
    """SOI, APP0 (JFIF 1.01, no density unit, 1 : 1), DQT (both tables), SOF0, DHT (all four tables), DRI (one MCU row), SOS"""
    S = SUBSAMPLING[subsampling]
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xe0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    out += _segment(0xdb, b"\x00" + bytes(ql[ZIGZAG].astype(np.uint8)) + b"\x01" + bytes(qc[ZIGZAG].astype(np.uint8)))
    out += _segment(0xc0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x11 * S, 0, 2, 0x11, 1, 3, 0x11, 1]))
    dht = b""
    for cls_id, bits, vals in ((0x00, DC_BITS[0], DC_VALS), (0x10, AC_BITS[0], AC_VALS[0]), (0x01, DC_BITS[1], DC_VALS), (0x11, AC_BITS[1], AC_VALS[1])):
        dht += bytes([cls_id]) + bytes(bits) + bytes(vals)
    out += _segment(0xc4, dht)
    out += _segment(0xdd, struct.pack(">H", -(-W // (8 * S))))
    out += _segment(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(img, quality: int = 90, subsampling: str = "4:2:0") -> bytes:
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return header(img.shape[0], img.shape[1], quality, subsampling) + entropy_code(*coefficients(img, quality, subsampling)) + b"\xff\xd9"


def entropy_segment(data: bytes) -> bytes:
    """the bytes between the SOS segment and EOI of a file with one scan"""
    at = 2
    while True:
        assert data[at] == 0xff, at
        marker, (length,) = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])
        at += 2 + length
        if marker == 0xda:
            break
    assert data[-2:] == b"\xff\xd9"
    return data[at:-2]


def restart_markers(segment: bytes):
    """m of every RSTm in an entropy-coded segment, in order (0xFF is followed by 0x00 when it is data)"""
    return [segment[i + 1] - 0xd0 for i in range(len(segment) - 1) if segment[i] == 0xff and 0xd0 <= segment[i + 1] <= 0xd7]


# ---- test images ----
def recipe_image(H: int, W: int, seed: int = 0):
    """base = 128 + 100 [sin(x/17 + y/29), cos(x/23 - y/13), sin(x/11) cos(y/19)], integer noise in [-24, 24] shared by the three
    channels added, clipped to [0, 255]; every ninth row scaled by 0.3"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 128.0 + 100.0 * np.stack([np.sin(x / 17 + y / 29), np.cos(x / 23 - y / 13), np.sin(x / 11) * np.cos(y / 19)], axis=-1)
    noise = np.random.default_rng(seed).integers(-24, 25, size=(H, W, 1))
    img = np.clip(base + noise, 0, 255)
    img[::9] *= 0.3
    return img.astype(np.uint8)


def noise_image(H: int, W: int, seed: int = 1):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, 3), dtype=np.uint8)


RECIPE_SIZES = ((40, 56), (50, 70), (100, 150))
SMALL_SIZES = ((1, 1), (5, 7), (8, 8), (16, 16), (17, 23))


def image_set():
    """{name: u8 [H, W, 3]}: the recipe at its three sizes, noise, a constant, all 255, and the small shapes (recipe content)"""
    out = {f"recipe{h}x{w}": recipe_image(h, w) for h, w in RECIPE_SIZES}
    out["noise33x47"] = noise_image(33, 47)
    out["constant24x40"] = np.full((24, 40, 3), (200, 90, 30), np.uint8)
    out["white35x33"] = np.full((35, 33, 3), 255, np.uint8)
    out.update({f"small{h}x{w}": recipe_image(h, w, seed=h + w) for h, w in SMALL_SIZES})
    return out


def ycc_float(img):
    """fp64 [3, H, W]: the JFIF YCbCr of the source, unrounded"""
    r, g, b = (img[..., i].astype(np.float64) for i in range(3))
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b,
                     128.0 - 0.168735892 * r - 0.331264108 * g + 0.5 * b,
                     128.0 + 0.5 * r - 0.418687589 * g - 0.081312411 * b])


def psnr_planes(decoded_ycc, img):
    """[3] PSNR of a decoded u8 [H, W, 3] YCbCr image against the fp64 YCbCr of the source, per plane (inf for no error)"""
    ref = ycc_float(img)
    out = []
    for c in range(3):
        mse = float(np.mean((decoded_ycc[..., c].astype(np.float64) - ref[c]) ** 2))
        out.append(float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse))
    return out


# ---- RIFF ----
def _chunks(data: bytes, start: int, end: int):
    out, at = [], start
    while at < end:
        assert at + 8 <= end, f"chunk header at {at} runs past {end}"
        fourcc, (size,) = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])
        assert at + 8 + size <= end, f"chunk {fourcc!r} at {at} (size {size}) runs past {end}"
        if fourcc in (b"RIFF", b"LIST"):
            out.append({"id": fourcc, "type": data[at + 8:at + 12], "offset": at, "size": size, "children": _chunks(data, at + 12, at + 8 + size)})
        else:
            out.append({"id": fourcc, "offset": at, "size": size, "data": data[at + 8:at + 8 + size]})
        at += 8 + size + (size & 1)
    assert at == end or at == end + 1, (at, end)
    return out


def walk_avi(data: bytes):
    """the tree of a RIFF file: every chunk's size is checked against its parent's and the RIFF size against the file's length"""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _chunks(data, 0, len(data))
    assert len(top) == 1
    return top[0]


def find(node, fourcc: bytes, list_type: bytes = None):
    """the first chunk (depth first) with this id (and, for a LIST, this type)"""
    for c in node.get("children", ()):
        if c["id"] == fourcc and (list_type is None or c.get("type") == list_type):
            return c
        hit = find(c, fourcc, list_type)
        if hit is not None:
            return hit
    return None


# ---- what the CPU and the GPU tests share ----
QUALITIES = (1, 50, 75, 90, 95, 100)
_files = {}


def reference_file(name: str, quality: int, subsampling: str) -> bytes:
    """the restatement's file of image_set()[name], computed once per process"""
    key = (name, quality, subsampling)
    if key not in _files:
        if "images" not in _files:
            _files["images"] = image_set()
        _files[key] = encode(_files["images"][name], quality, subsampling)
    return _files[key]


def batch_of_three():
    """u8 [3, 40, 56, 3]: three different images for one call"""
    return np.stack([recipe_image(40, 56, seed=7), noise_image(40, 56, seed=8), np.full((40, 56, 3), 255, np.uint8)])


def pil_file(img, quality: int, subsampling: str) -> bytes:
    """PIL's file of the image with the same structure: one restart interval per MCU row, the typical Huffman tables"""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling, restart_marker_rows=1, optimize=False)
    return buf.getvalue()


def decode_ycc(data: bytes):
    """u8 [H, W, 3] YCbCr as the decoder leaves it: no colour conversion enters"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    return np.asarray(im)


def pil_gate(ours, img, quality: int, subsampling: str):
    """The rule that holds an encoder to PIL at one quality step: per plane, where PIL's PSNR rises strictly over q - 1, q, q + 1
    ours must reach PIL's at q - 1; where it does not, ours must reach PIL's at q minus the spread PIL itself shows over the three.
    Returns (per plane: (ours, PIL at q - 1, q, q + 1, strictly rising, bound), our length, PIL's three lengths)."""
    files = [pil_file(img, q, subsampling) for q in (quality - 1, quality, quality + 1)]
    theirs = [psnr_planes(decode_ycc(f), img) for f in files]
    mine = psnr_planes(decode_ycc(ours), img)
    planes = []
    for c in range(3):
        a, b, d = (t[c] for t in theirs)
        rising = a < b < d
        planes.append((mine[c], a, b, d, rising, a if rising else b - (max(a, b, d) - min(a, b, d))))
    return planes, len(ours), [len(f) for f in files]


def round_cases():
    """{name: (u8 [n, H, W, 3], quality, subsampling)}: the sizes at which a kernel goes round its loop again -- an interval of more
    than 256 blocks and of more than one 131072-bit window of the pack kernel (its blocks straddle the windows) and more than
    2048 bytes for the stuff kernel; a frame of more than 256 intervals; a batch of more than 256 frames"""
    return {"wide444": (noise_image(9, 700, seed=11)[None], 100, "4:4:4"),
            "wide420": (noise_image(17, 700, seed=12)[None], 100, "4:2:0"),
            "tall444": (recipe_image(2052, 8, seed=13)[None], 50, "4:4:4"),
            "many420": (np.stack([noise_image(8, 8, seed=100 + k) for k in range(257)]), 75, "4:2:0")}
