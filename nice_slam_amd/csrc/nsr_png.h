// nsr_png.h -- a PNG decoder for a batch of files whose compressed bytes are on the device (include/nsr.h, "PNG decoding"): 8-bit and
// 16-bit grey, 8-bit RGB and RGBA, non-interlaced.  The host walks the chunks and checks their CRCs (nice_slam_amd/png.py) and
// hands over, per file, ONE zlib stream -- the concatenated IDAT payloads -- as a byte range of `streams`; the library returns the
// pixels Pillow gives for the file, bit for bit.  Included by nsr_api.cpp behind nsr_jpegdec.h.
//
// Two launches, a workgroup of ONE wave per file in each (a DEFLATE stream is serial, and so are the rows of a filtered image:
// the parallelism is across the files of the batch and, inside a file, across the bytes of a copy and the rows of a pass).
//
//   1 png_inflate_kernel   RFC 1950 / RFC 1951 as zlib's inflate reads them with a 32 KiB window: the zlib header (CM = 8,
//        CINFO <= 7, no FDICT, FCHECK), then stored, fixed and dynamic blocks in any number.  The wave decodes UNIFORMLY: every
//        lane holds the same bit buffer and takes the same branches, so the decoder's state sits in scalar registers.
//          input    kPngStageWords 32-bit words of the stream are staged in LDS by all lanes (a byte behind stream_end reads as 0)
//                   and refilled when the reader runs off them; the bit buffer takes a whole word when it holds <= 32 bits, so that
//                   a literal/length code with its extra bits (<= 20) and a distance code with its extra bits (<= 28) never wait.
//          tables   the block's code lengths go to LDS; lane 0 counts them, checks the set as zlib's inflate_table does (an
//                   over-subscribed set, or an incomplete one other than a single code of length 1, is an error; the code-length
//                   alphabet must be complete) and sorts the symbols by length; all lanes then fill the primary table: the code's
//                   first kPngLutBits bits -> symbol << 4 | length.  A longer code (table entry 0) is found by the canonical walk
//                   over the counts per length, bit by bit; no code at the walk's end is an invalid code.
//          output   a ring of kPngWindow bytes in LDS holds the last 64 KiB written, twice zlib's window.  Literals collect in a
//                   lane each and are stored 64 at a time; a match of length L at distance D is copied by all lanes at once, byte
//                   i from pos - D + (i mod D) -- all of them bytes from before the match, so an overlapping copy (D < L) needs no
//                   order among the lanes.  Every kPngFlush bytes the ring's oldest part is written to the file's slice of the
//                   workspace with 16-byte stores; the tail at the end.  Global memory is only ever stored to.
//        Bounds: the block loop ends at the stream's end (a block header takes 3 bits), the symbol loop at the expected size
//        H (1 + stride) or the stream's end; a literal or a copy that would pass the expected size is not stored; a distance beyond
//        the bytes written so far copies nothing; a stored block's bytes are fetched inside [stream_begin, stream_end).
//        Where this is laxer than zlib (none of it changes the pixels of a file zlib reads): the trailing Adler-32 is not read,
//        so a stream that ends right behind its last block, without those four bytes, has status 0 where zlib reports a
//        truncated stream; and the window is 32 KiB whatever CINFO says, so a stream that declares a smaller window (CINFO < 7)
//        and then reaches further back than it declared decodes, where zlib refuses the distance.
//   2 png_unfilter_kernel<bpp>   the filtered scanlines -> pixels.  A skewed wavefront: in a pass of 64 rows lane l works on row
//        r0 + l, one pixel behind lane l - 1, so that in step t it un-filters pixel x = t - l: a is its own previous pixel, b the
//        pixel lane l - 1 finished in step t - 1 (one lane shuffle), c the b of its own previous step.  The first row of a pass
//        reads b from the last row of the pass before, which lane 63 stored un-filtered over its scanline in the workspace; the
//        image's first row has b = c = 0, a row's first pixel a = c = 0.  None, Sub, Up, Average floor((a + b) / 2) on the 9-bit sum,
//        Paeth with the tie order a, b, c.  A filter byte above 4 sets status bit 16 (the row is then read as None).
//        Output: 16-bit samples host-endian; RGBA with or without alpha; 8-bit grey once or three times.
//
// status[f] (int32), written by the inflate kernel and or-ed into by the un-filter kernel (the file's own wave in both, no atomics):
//   1 zlib header, block type 3 or a stored block with LEN != ~NLEN     2 an invalid code set or an invalid code
//   4 a distance before the start of the output                         8 the stream is too short or holds too many bytes
//   16 a filter type above 4
// A frame with a nonzero status has unspecified pixels; the others are unaffected.
// Workspace (nsr_png_size): per file H (1 + stride) bytes of filtered scanlines, rounded up to 16.
#pragma once

namespace nsr {

constexpr int kPngThreads = 64;                   // one wave per file
constexpr int kPngLutBits = 10;                   // width of the primary decoding table; longer codes take the canonical walk
constexpr int kPngWindow = 65536;                 // the LDS ring of output bytes (a power of two >= 32768 + kPngFlush + 258 + 64)
constexpr int kPngFlush = 16384;                  // bytes the ring hands to global memory at a time
constexpr int kPngStageWords = 512;               // words of the stream staged in LDS
constexpr int kPngMaxStream = 1 << 30;            // bytes of one stream: bit positions are 64-bit, word indices 32-bit
constexpr int kPngAhead = 8;                      // pixels the un-filter kernel loads ahead of its dependent chain
constexpr unsigned char kPngClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct PngHuff {
    unsigned short lut[1 << kPngLutBits];         // symbol << 4 | length; 0: a longer code, or none
    unsigned short count[16], offs[16], first[16], next[16];   // per length: codes, index of the first in sym, its code, (build) cursor
    unsigned short sym[288];                      // symbols in code order
    int left, max, total;                         // what the set leaves of the code space; the longest length; coded symbols
};
struct alignas(16) PngU4 { unsigned x, y, z, w; };

// ring | staged words | code lengths (288 + 32) | literal/length table | distance table (also the code-length alphabet's)
constexpr int kPngLensOff = kPngWindow + 4 * kPngStageWords;
constexpr int kPngHuffOff = kPngLensOff + 320;
constexpr int kPngInflateLds = kPngHuffOff + 2 * (int)sizeof(PngHuff);

struct PngParams {
    const unsigned char *streams;
    const nsr_png_frame *desc;                    // [n]
    unsigned char *filtered;                      // [n][slice]: H rows of 1 + stride bytes
    void *out;                                    // [n][H][W][out_channels] u8, or [n][H][W] u16
    int *status;                                  // [n]
    long long slice;
    int n, H, W, kind, bpp, out_channels;
};

// ---- the bit reader: wave-uniform state -----------------------------------------------------------------------------------------
struct PngBits {
    const unsigned char *src;                     // the stream's first byte
    unsigned *stage;                              // LDS
    long long nbytes;
    unsigned long long bb;
    int bc, nw, sbase, lane;                      // bits in bb; the next word to take; the first staged word

    NSR_DEV void stage_at(int w0) {
        block_sync();                             // every lane has read what it needed of the words staged before
        for (int k = lane; k < kPngStageWords; k += kPngThreads) {
            const long long b = 4ll * (w0 + k);
            unsigned v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (b + j < nbytes) v |= (unsigned)src[b + j] << (8 * j);
            stage[k] = v;
        }
        sbase = w0;
        block_sync();
    }
    NSR_DEV unsigned word() {
        if (nw - sbase >= kPngStageWords) stage_at(nw);
        return (unsigned)uniform((int)stage[nw - sbase]);
    }
    NSR_DEV void seek(long long bytepos) {
        nw = (int)(bytepos >> 2);
        if (nw < sbase || nw - sbase >= kPngStageWords) stage_at(nw);
        const int skip = 8 * (int)(bytepos & 3);
        bb = (unsigned long long)(word() >> skip);
        bc = 32 - skip;
        ++nw;
    }
    NSR_DEV void need() {                         // afterwards bb holds more than 32 bits
        if (bc <= 32) {
            bb |= (unsigned long long)word() << bc;
            bc += 32;
            ++nw;
        }
    }
    NSR_DEV unsigned take(int n) {
        const unsigned v = (unsigned)bb & ((1u << n) - 1u);
        bb >>= n;
        bc -= n;
        return v;
    }
    NSR_DEV long long used_bits() const { return 32ll * nw - bc; }
    NSR_DEV bool over() const { return used_bits() > 8 * nbytes; }
};

// ---- decoding tables ---------------------------------------------------------------------------------------------------------------
// the table of `n` code lengths (LDS, written by lane 0).  0, or status bit 2 for a set zlib's inflate_table refuses.
NSR_DEV int png_build(PngHuff *h, const unsigned char *lens, int n, bool complete_only, int lane) {
    block_sync();                                 // the lengths are written, the table's last reader is done
    for (int i = lane; i < (1 << kPngLutBits); i += kPngThreads) h->lut[i] = 0;
    if (lane == 0) {
        for (int l = 0; l < 16; ++l) h->count[l] = 0;
        for (int s = 0; s < n; ++s) h->count[lens[s] & 15]++;
        int left = 1, max = 0, code = 0, prev = 0, off = 0;
        for (int l = 1; l < 16; ++l) {
            const int c = h->count[l];
            if (left >= 0) left = 2 * left - c;   // (stays negative once over-subscribed)
            if (c) max = l;
            code = (code + prev) << 1;
            prev = c;
            h->first[l] = (unsigned short)code;
            h->offs[l] = h->next[l] = (unsigned short)off;
            off += c;
        }
        for (int s = 0; s < n; ++s) {
            const int l = lens[s] & 15;
            if (l) h->sym[h->next[l]++] = (unsigned short)s;
        }
        h->left = left;
        h->max = max;
        h->total = off;
    }
    block_sync();
    const int left = uniform(h->left), max = uniform(h->max), total = uniform(h->total);
    int bad = 0;
    if (max != 0 && (left < 0 || (left > 0 && (complete_only || max != 1)))) bad = 2;
    if (!bad)
        for (int i = lane; i < total; i += kPngThreads) {
            const int s = h->sym[i], l = lens[s] & 15;
            if (l > kPngLutBits) continue;
            const unsigned code = (unsigned)h->first[l] + (unsigned)(i - h->offs[l]);
            unsigned rev = 0;
            for (int k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
            for (unsigned k = rev; k < (1u << kPngLutBits); k += 1u << l) h->lut[k] = (unsigned short)(s << 4 | l);
        }
    block_sync();
    return bad;
}

// the symbol at the head of `bits` and its length; -1: no such code
NSR_DEV int png_symbol(const PngHuff *h, unsigned long long bits, int &len) {
    const int e = uniform((int)h->lut[(unsigned)bits & ((1u << kPngLutBits) - 1u)]);
    if (e) {
        len = e & 15;
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(bits >> (l - 1)) & 1;
        const int c = uniform((int)h->count[l]);
        if (code - c < first) {
            len = l;
            return uniform((int)h->sym[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    len = 0;
    return -1;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------
struct PngOut {
    unsigned char *ring;                          // LDS
    unsigned char *dst;                           // the file's slice
    long long pos, flushed, expected;             // bytes written to the ring; handed to global memory; H (1 + stride)
    unsigned lit;                                 // this lane's pending literal
    int npend, lane;

    NSR_DEV void store_literals() {
        if (npend) {
            if (lane < npend) ring[(pos + lane) & (kPngWindow - 1)] = (unsigned char)lit;
            pos += npend;
            npend = 0;
        }
    }
    NSR_DEV void flush() {                        // (pos <= expected: the chunk lies inside the slice)
        if (pos - flushed >= kPngFlush) {
            block_sync();
            for (int o = 16 * lane; o < kPngFlush; o += 16 * kPngThreads)
                *reinterpret_cast<PngU4 *>(dst + flushed + o) = *reinterpret_cast<const PngU4 *>(ring + ((flushed + o) & (kPngWindow - 1)));
            flushed += kPngFlush;
        }
    }
    NSR_DEV void finish() {
        store_literals();
        flush();
        block_sync();
        for (long long o = flushed + lane; o < pos; o += kPngThreads) dst[o] = ring[o & (kPngWindow - 1)];
    }
};

NSR_KERNEL NSR_BOUNDS(kPngThreads) void png_inflate_kernel(const PngParams P) {
    char *lds = lds_base();
    const int lane = tid(), f = bid_x();
    unsigned char *lens = reinterpret_cast<unsigned char *>(lds + kPngLensOff);
    PngHuff *hl = reinterpret_cast<PngHuff *>(lds + kPngHuffOff), *hd = hl + 1;
    const nsr_png_frame d = P.desc[f];
    long long nbytes = d.stream_end - d.stream_begin;
    if (d.stream_begin < 0 || nbytes < 0) nbytes = 0;
    if (nbytes > kPngMaxStream) nbytes = kPngMaxStream;

    PngBits in;
    in.src = P.streams + (nbytes ? d.stream_begin : 0);
    in.stage = reinterpret_cast<unsigned *>(lds + kPngWindow);
    in.nbytes = nbytes;
    in.lane = lane;
    in.sbase = -kPngStageWords;
    in.seek(0);
    PngOut out;
    out.ring = reinterpret_cast<unsigned char *>(lds);
    out.dst = P.filtered + f * P.slice;
    out.pos = out.flushed = 0;
    out.expected = (long long)P.H * (1 + (long long)P.W * P.bpp);
    out.lit = 0;
    out.npend = 0;
    out.lane = lane;

    int st = 0;
    in.need();
    const unsigned cmf = in.take(8), flg = in.take(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 32u) || ((cmf << 8 | flg) % 31u)) st |= 1;
    int last = 0;
    bool fixed_ready = false;                     // the two tables in LDS are the fixed block's
    while (!st && !last) {
        in.need();
        last = (int)in.take(1);
        const int type = (int)in.take(2);
        if (type == 3) {
            st |= 1;
        } else if (type == 0) {
            in.take(in.bc & 7);
            in.need();
            const unsigned len = in.take(16);
            in.need();
            const unsigned nlen = in.take(16);
            const long long at = in.used_bits() >> 3;
            if ((len ^ nlen) != 0xffffu) st |= 1;
            else if (at + len > nbytes || out.pos + out.npend + len > out.expected) st |= 8;
            else {
                out.store_literals();
                for (unsigned o = 0; o < len; o += kPngThreads) {
                    if (o + lane < len) out.ring[(out.pos + lane) & (kPngWindow - 1)] = in.src[at + o + lane];
                    out.pos += len - o < (unsigned)kPngThreads ? len - o : kPngThreads;
                    out.flush();
                }
                in.seek(at + len);
            }
        } else {
            if (type == 1) {
                if (!fixed_ready) {               // (a stream of many small fixed blocks -- Z_FIXED, flush points -- builds them once)
                    block_sync();                 // the last reader of the lengths is done
                    for (int s = lane; s < 320; s += kPngThreads) lens[s] = (unsigned char)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                    st |= png_build(hl, lens, 288, false, lane);
                    st |= png_build(hd, lens + 288, 32, false, lane);
                    fixed_ready = true;
                }
            } else {
                fixed_ready = false;
                const int nlen = (int)in.take(5) + 257, ndist = (int)in.take(5) + 1, ncode = (int)in.take(4) + 4;
                if (nlen > 286 || ndist > 30) st |= 2;
                if (!st) {
                    block_sync();
                    if (lane == 0)
                        for (int k = 0; k < 19; ++k) lens[k] = 0;
                    for (int k = 0; k < ncode; ++k) {
                        in.need();
                        const unsigned v = in.take(3);
                        if (lane == 0) lens[kPngClOrder[k]] = (unsigned char)v;
                    }
                    st |= png_build(hd, lens, 19, true, lane);
                }
                int have = 0, prev = 0;
                while (!st && have < nlen + ndist) {
                    in.need();
                    int l;
                    const int s = png_symbol(hd, in.bb, l);
                    if (s < 0) { st |= 2; break; }
                    in.take(l);
                    int rep = 1, val = s;
                    if (s == 16) {
                        if (!have) { st |= 2; break; }
                        val = prev;
                        rep = 3 + (int)in.take(2);
                    } else if (s == 17) {
                        val = 0;
                        rep = 3 + (int)in.take(3);
                    } else if (s == 18) {
                        val = 0;
                        rep = 11 + (int)in.take(7);
                    }
                    if (have + rep > nlen + ndist) { st |= 2; break; }
                    if (lane == 0)
                        for (int k = 0; k < rep; ++k) lens[have + k] = (unsigned char)val;
                    have += rep;
                    prev = val;
                    if (in.over()) st |= 8;
                }
                if (!st) {
                    block_sync();
                    if (uniform((int)lens[256]) == 0) st |= 2;              // no end-of-block code
                }
                if (!st) st |= png_build(hl, lens, nlen, false, lane);
                if (!st) st |= png_build(hd, lens + nlen, ndist, false, lane);
            }
            while (!st) {
                if (in.over()) { st |= 8; break; }
                in.need();
                int l;
                const int s = png_symbol(hl, in.bb, l);
                if (s < 0) { st |= 2; break; }
                in.take(l);
                if (s < 256) {
                    if (out.pos + out.npend >= out.expected) { st |= 8; break; }
                    if (lane == out.npend) out.lit = (unsigned)s;
                    if (++out.npend == kPngThreads) {
                        out.store_literals();
                        out.flush();
                    }
                    continue;
                }
                if (s == 256) break;
                if (s > 285) { st |= 2; break; }
                const int lc = s - 257;
                int len = 258;
                if (lc < 8) len = 3 + lc;
                else if (lc < 28) {
                    const int eb = (lc >> 2) - 1;
                    len = 3 + ((4 + (lc & 3)) << eb) + (int)in.take(eb);
                }
                in.need();
                const int ds = png_symbol(hd, in.bb, l);
                if (ds < 0 || ds > 29) { st |= 2; break; }
                in.take(l);
                int dist = 1 + ds;
                if (ds >= 4) {
                    const int eb = (ds >> 1) - 1;
                    dist = 1 + ((2 + (ds & 1)) << eb) + (int)in.take(eb);
                }
                out.store_literals();
                if (dist > out.pos) { st |= 4; break; }
                if (out.pos + len > out.expected) { st |= 8; break; }
                block_sync();                     // the bytes before the match are in the ring
                const long long from = out.pos - dist;
                for (int i = lane; i < len; i += kPngThreads) {
                    const int k = dist >= len ? i : i % dist;
                    out.ring[(out.pos + i) & (kPngWindow - 1)] = out.ring[(from + k) & (kPngWindow - 1)];
                }
                out.pos += len;
                out.flush();
            }
        }
        if (in.over()) st |= 8;
    }
    out.finish();
    if (!st && out.pos != out.expected) st |= 8;
    if (lane == 0) P.status[f] = st;
}

// ---- un-filter -------------------------------------------------------------------------------------------------------------------
template <int BPP>
NSR_DEV unsigned png_pixel(const unsigned char *p) {
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < BPP; ++k) v |= (unsigned)p[k] << (8 * k);
    return v;
}

template <int BPP>
NSR_KERNEL NSR_BOUNDS(kPngThreads) void png_unfilter_kernel(const PngParams P) {
    const int lane = tid(), f = bid_x(), H = P.H, W = P.W, oc = P.out_channels;
    const long long rb = 1 + (long long)W * BPP;
    unsigned char *slice = P.filtered + f * P.slice;
    bool bad = false;
    for (int r0 = 0; r0 < H; r0 += kPngThreads) {
        const int r = r0 + lane;
        const bool live = r < H;
        unsigned char *row = slice + (live ? r : 0) * rb + 1;
        const unsigned char *above = row - rb;                 // read by lane 0 alone, from the second pass on
        int ft = live ? row[-1] : 0;
        if (ft > 4) {
            bad = true;
            ft = 0;
        }
        const long long opix = ((long long)f * H + r) * W;
        unsigned a = 0, c = 0, cur = 0;
        for (int t0 = 0; t0 < W + kPngThreads - 1; t0 += kPngAhead) {
            unsigned raw[kPngAhead], top[kPngAhead];
#pragma unroll
            for (int j = 0; j < kPngAhead; ++j) {
                const int x = t0 + j - lane;
                const bool act = live && x >= 0 && x < W;
                raw[j] = act ? png_pixel<BPP>(row + (long long)x * BPP) : 0u;
                top[j] = act && lane == 0 && r0 > 0 ? png_pixel<BPP>(above + (long long)x * BPP) : 0u;
            }
#pragma unroll
            for (int j = 0; j < kPngAhead; ++j) {
                const int x = t0 + j - lane;
                const bool act = live && x >= 0 && x < W;
                unsigned b = (unsigned)shfl_i((int)cur, lane - 1);      // the pixel above: the neighbour's last one
                if (lane == 0) b = top[j];
                if (!act) continue;
                unsigned v = 0;
#pragma unroll
                for (int k = 0; k < BPP; ++k) {
                    const int A = (int)(a >> (8 * k)) & 255, B = (int)(b >> (8 * k)) & 255, C = (int)(c >> (8 * k)) & 255;
                    int pred = 0;
                    if (ft == 1) pred = A;
                    else if (ft == 2) pred = B;
                    else if (ft == 3) pred = (A + B) >> 1;
                    else if (ft == 4) {
                        const int p = A + B - C;
                        const int pa = p > A ? p - A : A - p, pb = p > B ? p - B : B - p, pc = p > C ? p - C : C - p;
                        pred = pa <= pb && pa <= pc ? A : (pb <= pc ? B : C);
                    }
                    v |= (((raw[j] >> (8 * k)) + (unsigned)pred) & 255u) << (8 * k);
                }
                if (lane == kPngThreads - 1 && r + 1 < H) {            // the row the next pass starts from
#pragma unroll
                    for (int k = 0; k < BPP; ++k) row[(long long)x * BPP + k] = (unsigned char)(v >> (8 * k));
                }
                if (BPP == 2) {
                    reinterpret_cast<unsigned short *>(P.out)[opix + x] = (unsigned short)((v & 255u) << 8 | v >> 8);
                } else {
                    unsigned char *o = reinterpret_cast<unsigned char *>(P.out) + (opix + x) * oc;
                    for (int k = 0; k < oc; ++k) o[k] = (unsigned char)(BPP == 1 ? v : v >> (8 * k));
                }
                a = cur = v;
                c = b;
            }
        }
        block_sync();                                                   // lane 63's row is in memory before lane 0 reads it
    }
    const bool any = ballot64(bad) != 0ull;
    if (lane == 0 && any) P.status[f] |= 16;
}

}  // namespace nsr
