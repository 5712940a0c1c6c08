"""TEST INFRASTRUCTURE: the JPEG decoder of nice_slam_amd/csrc/nsr_jpegdec.h restated in numpy -- a plain sequential Huffman decode
(one bit position, no subsequences), then the DC sums, the inverse DCT, the upsampling and the colour conversion operation for
operation (the same integers at the same rounding points, so the same pixels) -- and the header parser's verdicts.  The image
makers are those of tests/jpeg_reference.py.  Nothing here imports the package.

    decode(data) -> (u8 [H, W, 3], status)       status 0, or bits 1 invalid code, 2 zig-zag overrun, 4 block count, 8 restart markers
    parse(data) -> dict                          the header; Unsupported(reason) for what the decoder does not take
    pil_file(img, **save_options) -> bytes       Pillow's file;  pil_pixels(data): Pillow's RGB pixels of a file
"""
import io
import struct

import numpy as np

from jpeg_reference import ZIGZAG, noise_image, recipe_image  # noqa: F401  (the tests take the image makers from here)

LUMA = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}
REFUSED_SOF = {0xc1: "extended", 0xc2: "progressive", 0xc3: "lossless", 0xc5: "hierarchical", 0xc6: "hierarchical", 0xc7: "hierarchical",
               0xc9: "arithmetic", 0xca: "arithmetic", 0xcb: "arithmetic", 0xcc: "arithmetic", 0xcd: "arithmetic", 0xce: "arithmetic",
               0xcf: "arithmetic"}


class Unsupported(Exception):
    pass


def huffman_is_valid(bits, nvals, dc, vals=()):
    """T.81 annex C with libjpeg's rule that the all-ones code stays free; as many symbols as codes; DC symbols <= 15"""
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if bits[length - 1] and code > (1 << length) - 1:
            return False
        code <<= 1
    return nvals == sum(bits) and not (dc and any(v > 15 for v in vals))


def parse(data: bytes) -> dict:
    if data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    at, qt, huff, sof, jfif, adobe, ri = 2, {}, {}, None, False, None, 0
    while True:
        if at + 4 > len(data):
            raise Unsupported("no scan")
        assert data[at] == 0xff
        m, (length,) = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])
        seg = data[at + 4:at + 2 + length]
        if m in REFUSED_SOF:
            raise Unsupported(REFUSED_SOF[m])
        if m == 0xc0:
            prec, h, w, nf = struct.unpack(">BHHB", seg[:6])
            sof = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)]
            if prec != 8 or h == 0 or w == 0:
                raise Unsupported("precision or size")
        elif m == 0xc4:
            p = 0
            while p < len(seg):
                bits = seg[p + 1:p + 17]
                vals = seg[p + 17:p + 17 + sum(bits)]
                if not huffman_is_valid(bits, len(vals), seg[p] >> 4 == 0, vals):
                    raise Unsupported("Huffman table")
                huff[(seg[p] >> 4, seg[p] & 15)] = (bits, vals)
                p += 17 + len(vals)
        elif m == 0xdb:
            for p in range(0, len(seg), 65):
                if seg[p] >> 4:
                    raise Unsupported("16-bit DQT")
                qt[seg[p] & 15] = np.frombuffer(seg[p + 1:p + 65], np.uint8).astype(np.int64)
        elif m == 0xdd:
            ri = struct.unpack(">H", seg)[0]
        elif m == 0xe0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xee and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xda:
            break
        at += 2 + length
    nf = len(sof)
    if nf == 1:
        if sof[0][1:3] != (1, 1):
            raise Unsupported("sampling")
        sampling = "grey"
    elif nf == 3:
        if sof[0][1:3] not in LUMA or sof[1][1:3] != (1, 1) or sof[2][1:3] != (1, 1):
            raise Unsupported("sampling")
        sampling = LUMA[sof[0][1:3]]
        if not jfif and ((adobe is not None and adobe != 1) or (adobe is None and [c[0] for c in sof] != [1, 2, 3])):
            raise Unsupported("colour space")
    else:
        raise Unsupported("components")
    if seg[0] != nf or tuple(seg[1 + 2 * nf:]) != (0, 63, 0):
        raise Unsupported("several scans")
    begin = at + 2 + length
    end = begin
    while end + 1 < len(data) and not (data[end] == 0xff and data[end + 1] not in (0x00, 0xff) and not 0xd0 <= data[end + 1] <= 0xd7):
        end += 1
    if end + 1 >= len(data):
        end = len(data)
    elif data[end + 1] != 0xd9:
        raise Unsupported("several scans or DNL")
    while end > begin and data[end - 1] == 0xff:
        end -= 1
    return {"height": h, "width": w, "sampling": sampling, "components": nf, "restart_interval": ri, "scan_begin": begin, "scan_end": end,
            "quant": [qt[c[3]] for c in sof], "dc": [huff[(0, seg[2 + 2 * i] >> 4)] for i in range(nf)],
            "ac": [huff[(1, seg[2 + 2 * i] & 15)] for i in range(nf)]}


def verdict(data: bytes):
    """None for a file the decoder takes, else the reason"""
    try:
        parse(data)
    except Unsupported as e:
        return str(e)
    return None


def geometry(p):
    hs, vs = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "grey": (1, 1)}[p["sampling"]]
    mcux, mcuy = -(-p["width"] // (8 * hs)), -(-p["height"] // (8 * vs))
    return hs, vs, mcux, mcuy, (1 if p["components"] == 1 else hs * vs + 2)


def chains(p, data):
    """the restart intervals of the scan as stuffed byte strings, and the numbers of the markers between them"""
    seg, parts, marks, i, start = data[p["scan_begin"]:p["scan_end"]], [], [], 0, 0
    while True:
        j = seg.find(b"\xff", i)
        if j < 0 or j + 1 >= len(seg):
            break
        if 0xd0 <= seg[j + 1] <= 0xd7:
            parts.append(seg[start:j])
            marks.append(seg[j + 1] & 7)
            start = j + 2
        i = j + 2 if seg[j + 1] == 0 or 0xd0 <= seg[j + 1] <= 0xd7 else j + 1
    parts.append(seg[start:])
    return parts, marks


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def entropy_decode(p, data):
    """(int64 [blocks, 64] zig-zag with the DC as a difference, status, block spans): one bit position walking each chain"""
    hs, vs, mcux, mcuy, bpm = geometry(p)
    M, ri = mcux * mcuy, p["restart_interval"]
    comp_of = [0 if (p["components"] == 1 or b < hs * vs) else b - hs * vs + 1 for b in range(bpm)]
    dc, ac = [_codes(*t) for t in p["dc"]], [_codes(*t) for t in p["ac"]]
    parts, marks = chains(p, data)
    nexp = -(-M // ri) if ri else 1
    status = 0 if len(parts) == nexp and marks == [j & 7 for j in range(len(marks))] else 8
    coef = np.zeros((M * bpm, 64), np.int64)
    for c in range(min(nexp, len(parts))):
        raw = parts[c].replace(b"\xff\x00", b"\xff")
        nbits = 8 * len(raw)
        stream = int.from_bytes(raw + b"\xff" * 8, "big")
        total = nbits + 64
        pos, first = 0, c * ri * bpm
        expb = (min(ri, M - c * ri) if ri else M) * bpm
        blk, k = 0, 0
        while blk < expb:
            if pos >= nbits:
                status |= 4
                break
            table = (dc if k == 0 else ac)[comp_of[blk % bpm]]
            window = (stream >> (total - pos - 32)) & 0xffffffff
            for length in range(1, 17):
                sym = table.get((length, window >> (32 - length)))
                if sym is not None:
                    break
            else:
                status |= 1
                pos += 1
                continue
            r, s = sym >> 4, sym & 15
            v = 0
            if s:
                x = (window >> (32 - length - s)) & ((1 << s) - 1)
                v = x if x >= 1 << (s - 1) else x - (1 << s) + 1
            pos += length + s
            if k == 0:
                coef[first + blk, 0] = v
                k = 1
            elif s == 0:
                k = k + 16 if r == 15 else 64
            else:
                k += r
                if k > 63:
                    status |= 2
                    k = 63
                coef[first + blk, k] = v
                k += 1
            if k >= 64:
                k, blk = 0, blk + 1
        else:
            if pos + 8 <= nbits:
                status |= 4
    return coef, status


def _idct8(v, shift):
    """jidctint on the last axis (8 values), int64"""
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * 4433
    e2, e3 = z1 + z3 * -15137, z1 + z2 * 6270
    z2, z3 = v[..., 0], v[..., 4]
    e0, e1 = (z2 + z3) << 13, (z2 - z3) << 13
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    o0, o1, o2, o3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    half = 1 << (shift - 1)
    return np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1) + half >> shift


def planes(p, coef):
    """the component planes u8, whole blocks wide and high: DC sums per interval, dequantisation, IDCT"""
    hs, vs, mcux, mcuy, bpm = geometry(p)
    M, ri = mcux * mcuy, p["restart_interval"]
    comp_of = np.array([0 if (p["components"] == 1 or b < hs * vs) else b - hs * vs + 1 for b in range(bpm)])
    comp = np.tile(comp_of, M)
    coef = coef.copy()
    step = (ri if ri else M) * bpm
    for a in range(0, M * bpm, step):
        for ci in range(p["components"]):
            idx = a + np.nonzero(comp[a:a + step] == ci)[0]
            coef[idx, 0] = ((np.cumsum(coef[idx, 0]) + 32768) & 0xffff) - 32768       # kept modulo 2^16
    q = np.stack(p["quant"])[comp]                                                     # zig-zag order, per block
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef * q
    w = nat.reshape(-1, 8, 8)
    w = _idct8(w.transpose(0, 2, 1), 11).transpose(0, 2, 1)                            # pass 1: columns
    px = np.clip(_idct8(w, 18) + 128, 0, 255).astype(np.uint8)                         # pass 2: rows
    out = [np.zeros((mcuy * vs * 8, mcux * hs * 8), np.uint8)] + [np.zeros((mcuy * 8, mcux * 8), np.uint8) for _ in range(p["components"] - 1)]
    px = px.reshape(mcuy, mcux, bpm, 8, 8)
    for b in range(bpm):
        c = comp_of[b]
        oy, ox, sy, sx = (b // hs, b % hs, vs, hs) if c == 0 else (0, 0, 1, 1)
        view = out[c].reshape(mcuy, sy * 8, mcux, sx * 8)
        view[:, 8 * oy:8 * oy + 8, :, 8 * ox:8 * ox + 8] = px[:, :, b].transpose(0, 2, 1, 3)
    return out


def upsample(c, hs, vs, H, W):
    """libjpeg-turbo's fancy upsampling of one chroma plane to int64 [H, W]"""
    cw, ch = -(-W // hs), -(-H // vs)
    c = c[:ch, :cw].astype(np.int64)
    if hs == 1:
        return c[:H, :W]
    left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    if vs == 1:
        even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
        even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
        out = np.stack([even, odd], -1).reshape(ch, 2 * cw)
        return out[:H, :W]
    rows = []
    for far in (np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])):       # the row above, the row below; edges repeated
        s = 3 * c + far
        sl, sr = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + sl + 8) >> 4, (3 * s + sr + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        rows.append(np.stack([even, odd], -1).reshape(ch, 2 * cw))
    return np.stack(rows, 1).reshape(2 * ch, 2 * cw)[:H, :W]


def decode(data: bytes):
    """(u8 [H, W, 3] RGB, status) of a supported file"""
    p = parse(data)
    hs, vs = geometry(p)[:2]
    H, W = p["height"], p["width"]
    coef, status = entropy_decode(p, data)
    pl = planes(p, coef)
    Y = pl[0][:H, :W].astype(np.int64)
    if p["components"] == 1:
        return np.repeat(Y[..., None], 3, -1).astype(np.uint8), status
    cb, cr = upsample(pl[1], hs, vs, H, W) - 128, upsample(pl[2], hs, vs, H, W) - 128
    rgb = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8), status


# ---- Pillow ----
def pil_file(img, **options) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **options)
    return buf.getvalue()


def pil_pixels(data: bytes):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"))


# ---- the cases the CPU and the GPU tests share ----
SIZES = ((1, 1), (5, 7), (8, 8), (16, 16), (17, 23), (33, 49), (50, 70))
SAMPLINGS = ("4:4:4", "4:2:2", "4:2:0", "grey")
RESTARTS = ({}, {"restart_marker_rows": 1}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 3})
_cache = {}


def content(kind: str, h: int, w: int):
    if kind == "recipe":
        return recipe_image(h, w, seed=h + w)
    if kind == "noise":
        return noise_image(h, w, seed=h * w)
    return np.full((h, w, 3), (200, 90, 30) if kind == "constant" else 255, np.uint8)


def case_file(kind, size, sampling, quality, optimize=False, restart=0, seed=None) -> bytes:
    """Pillow's file of one case, made once per process"""
    key = (kind, size, sampling, quality, optimize, restart, seed)
    if key not in _cache:
        img = content(kind, *size) if seed is None else noise_image(*size, seed=seed)
        opts = dict(quality=quality, optimize=optimize, **RESTARTS[restart])
        if sampling == "grey":
            img = img[..., 1].copy()
        else:
            opts["subsampling"] = sampling
        _cache[key] = pil_file(img, **opts)
    return _cache[key]


def reference(data: bytes):
    """decode(data), computed once per process"""
    if ("ref", data) not in _cache:
        _cache[("ref", data)] = decode(data)
    return _cache[("ref", data)]


def small_cases():
    """the cross product of the issue thinned to what a few seconds hold: every size x sampling, with content, quality, tables
    and restart setting rotating so that each value meets each size and each sampling"""
    kinds, quals, out, i = ("recipe", "noise", "constant", "white"), (1, 30, 90, 100), [], 0
    for size in SIZES:
        for sampling in SAMPLINGS:
            for r in range(4):
                out.append((kinds[(i + r) % 4], size, sampling, quals[(i // 4 + r) % 4], bool((i + r) & 1), r))
            i += 1
    return out


def split_pairs(data: bytes, sub: int) -> int:
    """FF 00 pairs of the scan's chains whose 00 is the first byte of a subsequence of `sub` bytes"""
    parts, _ = chains(parse(data), data)
    return sum(1 for part in parts for i in range(sub, len(part), sub) if part[i - 1] == 0xff and part[i] == 0)


def chain_lengths(data: bytes):
    """the bytes of every restart interval of the scan"""
    return [len(x) for x in chains(parse(data), data)[0]]


def block_ends(data: bytes):
    """the stuffed byte (within its chain) in which every block of an undamaged file ends, per chain: the sequential decode again,
    keeping positions only"""
    p = parse(data)
    hs, vs, mcux, mcuy, bpm = geometry(p)
    comp_of = [0 if (p["components"] == 1 or b < hs * vs) else b - hs * vs + 1 for b in range(bpm)]
    dc, ac = [_codes(*t) for t in p["dc"]], [_codes(*t) for t in p["ac"]]
    M, ri, out = mcux * mcuy, p["restart_interval"], []
    for c, part in enumerate(chains(p, data)[0]):
        raw = part.replace(b"\xff\x00", b"\xff")
        stuffed_at = np.arange(len(raw) + 1) + np.cumsum([0] + [b == 0xff for b in raw])   # unstuffed byte -> stuffed byte
        stream, total, pos, ends, k, blk = int.from_bytes(raw + b"\xff" * 8, "big"), 8 * len(raw) + 64, 0, [], 0, 0
        while blk < (min(ri, M - c * ri) if ri else M) * bpm:
            table = (dc if k == 0 else ac)[comp_of[blk % bpm]]
            window = (stream >> (total - pos - 32)) & 0xffffffff
            length, sym = next((n, table[(n, window >> (32 - n))]) for n in range(1, 17) if (n, window >> (32 - n)) in table)
            pos += length + (sym & 15)
            k = 1 if k == 0 else (k + 16 if sym == 0xf0 else 64) if sym & 15 == 0 else k + (sym >> 4) + 1
            if k >= 64:
                ends.append(int(stuffed_at[(pos - 1) >> 3]))
                k, blk = 0, blk + 1
        out.append(ends)
    return out
