// nsr_jpegdec.h -- a baseline JPEG decoder (ITU-T T.81 sequential DCT, 8 bit, Huffman coded) for a batch of files whose bytes are
// on the device (include/nsr.h, "JPEG decoding").  The host walks the markers and hands over one nsr_jpegdec_frame per file -- the
// tables, the restart interval and the byte range of the entropy-coded segment (nice_slam_amd/jpeg.py); the library returns
// u8 [n][H][W][3] RGB with the pixels libjpeg-turbo's default decoder gives (what Pillow returns for im.convert("RGB")), bit for
// bit.  Included by nsr_api.cpp behind nsr_jpeg.h, whose fixed-order workgroup scan (jpg_scan) and zig-zag table it shares.
//
// Accepted (everything else is refused by the host parser before anything is launched): SOF0, one interleaved scan over all
// components; 1 component, or 3 components Y Cb Cr with luma sampling 1 x 1, 2 x 1 or 2 x 2 and chroma 1 x 1 (4:4:4, 4:2:2, 4:2:0);
// any 8-bit DQT, any DHT (4 DC + 4 AC tables), any DRI or none; H, W in [1, 65535].  All frames of a call share H, W and sampling;
// each has its own tables and stream.
//
// Numerical contract (tests/jpegdec_reference.py restates it in numpy, operation for operation).  Integers end to end; `>>` is the
// arithmetic shift; no floating point, no atomics on global memory, every scan in a fixed order.
//   Stream     0xFF 0x00 is a stuffed 0xFF; 0xFF 0xD0..D7 ends a restart interval.  At the start of interval i the stream is
//              byte-aligned, the DC predictors are 0 and the MCU index is i Ri.  Bytes behind an interval's end read as 0xFF.
//   Entropy    T.81 annex F: a DC symbol s <= 15 followed by s bits, AC symbols r << 4 | s followed by s bits, 0x00 = end of block,
//              0xF0 = 16 zeros (a symbol r << 4 | 0 with r < 15 ends the block, as in libjpeg); s bits x stand for x if
//              x >= 2^(s - 1), else x - 2^s + 1.  Coefficients are kept int16 [block][64] in zig-zag order, the DC as a difference.
//   DC         the running sum of the differences per component within an interval, kept modulo 2^16 (libjpeg's cast to JCOEF).
//   IDCT       libjpeg's jidctint ("islow") on coef x Q, 64-bit intermediates: pass 1 over columns, descaled (x + 2^10) >> 11,
//              pass 2 over rows, descaled (x + 2^17) >> 18, then + 128 and clamped to [0, 255].  The 13-bit constants are
//              2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172.
//   Upsample   libjpeg-turbo's "fancy" upsampling of the chroma planes cropped to cw x ch = ceil(W / h) x ceil(H / v):
//              h2v2: s[x] = 3 near[x] + far[x] (the far row is the row above for an even output row, below for an odd one, the
//                    edge row repeated); even pixel (3 s[x] + s[x - 1] + 8) >> 4, odd (3 s[x] + s[x + 1] + 7) >> 4; the first
//                    and the last column (4 s + 8) >> 4 and (4 s + 7) >> 4
//              h2v1: even (3 p[x] + p[x - 1] + 1) >> 2, odd (3 p[x] + p[x + 1] + 2) >> 2; the first and last column copied
//   Colour     R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' + 32768) >> 16),
//              B = Y + ((116130 Cb' + 32768) >> 16), Cb' = Cb - 128, Cr' = Cr - 128, clamped to [0, 255]; one component: R = G = B.
//
// Six launches.  `chain` = one restart interval of one frame (the whole scan without DRI); M = MCUs of a frame.
//   1 jpegdec_clear_kernel    zero-fills the coefficients
//   2 jpegdec_markers_kernel  a workgroup per frame, a lane per 8 bytes: finds FF D0..D7, a fixed-order scan compacts the interval
//                             starts; a marker whose number is not its index mod 8 sets status bit 8
//   3 jpegdec_huffman_kernel  a workgroup walks a chain in tiles of 1024 subsequences of `subsequence_bytes` of the stuffed stream
//                             (self-synchronising decoding, Weissenberger & Schmidt): every lane decodes its subsequence
//                             speculatively from its first bit -- a symbol belongs to the subsequence it starts in -- and leaves
//                             its exit state (bit position, block of the MCU, zig-zag index) and the blocks it completed in LDS;
//                             lane 0 starts from the true state carried over from the tile before.  In each round a lane whose
//                             predecessor's exit state is not the state it started from decodes again from there; after round r
//                             the first r + 1 subsequences are final, so the loop runs at most (subsequences of the tile - 1)
//                             rounds and leaves early when no exit state changed.  A fixed-order scan of the block counts gives
//                             every subsequence its first block, and a last pass decodes once more and stores the coefficients.
//                             Speculation and synchronisation stay inside the tile, so no per-subsequence state goes through
//                             global memory.  The Huffman tables sit in LDS: a 9-bit lookup (length << 8 | symbol), behind it the
//                             maxcode / valoff walk of T.81 F.2.2.3 for the longer codes (8 tables, 11 KB).
//   4 jpegdec_dc_kernel       a workgroup per chain: the prefix sum of the DC differences per component; workgroup 0 of a frame
//                             also folds the chains' flags into the frame's status
//   5 jpegdec_idct_kernel     a lane per block, in registers: dequantise, IDCT, store 8 x 8 samples into the component's plane
//   6 jpegdec_color_kernel    a lane per pixel: upsample, convert, store
// Robustness (wrong-phase speculative decoding reads garbage by design): every stream fetch is clamped to its chain's bytes inside
// the frame's scan range, every table index is masked, an invalid code advances one bit, a zig-zag index is clamped to 63, every
// coefficient store is guarded by the chain's and the frame's block count.  status[f] (int32) is set in the last, synchronised pass:
// 1 an invalid code, 2 a zig-zag overrun, 4 a chain whose bytes and blocks do not end together (a block count other than the
// frame header's), 8 restart markers out of sequence or not as many as the restart interval asks for.  A frame with a nonzero
// status has unspecified pixels; the others are unaffected.
// Workspace (nsr_jpegdec_size): coefficients 128 B per block, the component planes, M + 1 interval starts and M chain flags per frame.
#pragma once

namespace nsr {

constexpr int kJpdMaxGridX = 1024;                // chains are dealt to at most this many workgroups per frame
constexpr int kJpdMaxScan = 1 << 28;              // bytes of one scan: bit positions are 32-bit
constexpr int kJpdMarkerBytes = 8;                // bytes per lane and round of the markers kernel
constexpr int kJpdThreads = 1024;                 // the Huffman kernel's workgroup = the subsequences of a tile: 4 waves per SIMD

struct JpdHuff {
    unsigned short lut[512];                      // the code's first 9 bits -> length << 8 | symbol, 0: longer than 9 bits (or none)
    int maxcode[18], valoff[18];                  // per length 1..16: the largest code (-1: none), index of its first symbol - its first code
    unsigned char vals[256];
};
constexpr int kJpdHuffLds = 8 * (int)sizeof(JpdHuff);
// tables | scan | exit positions | exit (block, zig-zag) | flags: changed[2], status[6] | block tables
constexpr int kJpdHuffmanLds = kJpdHuffLds + 2 * 4 * kJpdThreads + 2 * 4 * kJpdThreads + 4 * 8 + 16;

struct JpegDecParams {
    const unsigned char *files;
    const nsr_jpegdec_frame *desc;                // [n]
    short *coef;                                  // [n][nblk][64], zig-zag
    unsigned char *planes;                        // [n][plane_bytes]: Y, then Cb, Cr
    int *istart;                                  // [n][M + 1]: an interval's first byte in its scan
    int *nfound;                                  // [n]: restart markers in the scan
    int *mflags;                                  // [n]: the markers kernel's status bits
    int *cstat;                                   // [n][M]: the chains' status bits
    unsigned char *out;                           // [n][H][W][3]
    int *status;                                  // [n]
    long long nblk, plane_bytes, poff_c;          // blocks of a frame; a frame's planes; offset of Cb (Cr behind it)
    int n, H, W, hs, vs, ncomp, bpm, mcux, mcuy, M, sub_bytes;
    int pw_y, pw_c, ph_c, cw, ch;                 // plane widths (whole blocks); chroma plane height; the cropped chroma size
};

NSR_DEV int jpd_scan_len(const nsr_jpegdec_frame &d) {
    const long long len = d.scan_end - d.scan_begin;
    return len < 0 ? 0 : (len > kJpdMaxScan ? kJpdMaxScan : (int)len);
}
NSR_DEV int jpd_comp_of_block(const JpegDecParams &P, int b) { return P.ncomp == 1 || b < P.hs * P.vs ? 0 : b - P.hs * P.vs + 1; }
NSR_DEV int jpd_intervals(const JpegDecParams &P, int ri) { return ri > 0 ? (P.M + ri - 1) / ri : 1; }

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpegdec_clear_kernel(const JpegDecParams P) {
    const long long i = (long long)bid_x() * kJpgThreads + tid();              // 16 bytes each
    if (i >= P.n * P.nblk * 8) return;
    unsigned long long *p = reinterpret_cast<unsigned long long *>(P.coef) + 2 * i;
    p[0] = 0ull;
    p[1] = 0ull;
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpegdec_markers_kernel(const JpegDecParams P) {
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base());
    int *bad = reinterpret_cast<int *>(lds_base() + kJpgScanLds);
    const int t = tid(), f = bid_x();
    const nsr_jpegdec_frame &d = P.desc[f];
    const int len = jpd_scan_len(d);
    const unsigned char *s = P.files + d.scan_begin;
    int *ist = P.istart + (long long)f * (P.M + 1);
    if (t == 0) {
        ist[0] = 0;
        bad[0] = 0;
    }
    block_sync();
    unsigned long long carry = 0, total;
    for (int c0 = 0; c0 < len; c0 += kJpdMarkerBytes * kJpgThreads) {
        const int at = c0 + kJpdMarkerBytes * t;
        unsigned hit = 0, cnt = 0;
        unsigned prev = at < len ? s[at] : 0u;
#pragma unroll
        for (int k = 0; k < kJpdMarkerBytes; ++k) {
            const unsigned next = at + k + 1 < len ? s[at + k + 1] : 0u;
            if (prev == 0xffu && (next & 0xf8u) == 0xd0u) {
                hit |= 1u << k;
                ++cnt;
            }
            prev = next;
        }
        unsigned long long j = carry + jpg_scan(scan, t, cnt, total);
#pragma unroll
        for (int k = 0; k < kJpdMarkerBytes; ++k)
            if (hit >> k & 1u) {
                if ((s[at + k + 1] & 7u) != (unsigned)(j & 7ull)) bad[0] = 8;
                if (j < (unsigned long long)P.M) ist[j + 1] = at + k + 2;
                ++j;
            }
        carry += total;
    }
    block_sync();
    if (t == 0) {
        P.nfound[f] = carry > 0x7fffffffull ? 0x7fffffff : (int)carry;
        P.mflags[f] = bad[0];
    }
}

// A bit reader over the stuffed bytes [0, end) of a chain.  `pos` is the position of the next bit in the STUFFED stream (8 x byte +
// bit); it never points into a stuffed 0x00: `marks` flags the first bit of every buffered byte that stands behind a skipped one.
// Bytes behind the chain's end read as 0xFF.
struct JpdReader {
    const unsigned char *s;
    unsigned end, next, pos;
    unsigned long long buf, marks;                // the next bits, first bit = bit 63
    int nb;                                       // bits in buf
    bool pend, prevff;                            // the byte to load next stands behind a skipped 0x00; the last byte was 0xFF
    NSR_DEV unsigned byte(unsigned i) const { return i < end ? s[i] : 0xffu; }
    NSR_DEV void refill() {
        while (nb <= 56) {
            const unsigned c = byte(next);
            ++next;
            if (prevff && c == 0u) {              // a stuffed byte
                pend = true;
                prevff = false;
                continue;
            }
            buf |= (unsigned long long)c << (56 - nb);
            if (pend) marks |= 1ull << (63 - nb);
            pend = false;
            prevff = c == 0xffu;
            nb += 8;
        }
    }
    NSR_DEV void skip(int n) {                    // 1 <= n <= 31 <= nb - 26
        const unsigned long long m = (marks << 1) >> (64 - n);
        pos += (unsigned)n + 8u * (unsigned)__builtin_popcountll(m);
        buf <<= n;
        marks <<= n;
        nb -= n;
    }
    NSR_DEV void start(unsigned p) {              // p: a position that is not inside a stuffed 0x00
        buf = marks = 0ull;
        nb = 0;
        pend = prevff = false;
        next = p >> 3;
        pos = p & ~7u;
        refill();
        if (p & 7u) skip((int)(p & 7u));
    }
};

struct JpdChain {
    const JpdHuff *huff;                          // LDS: DC tables 0..3, AC tables 0..3
    const unsigned char *bdc, *bac;               // LDS: a block of the MCU -> its DC and AC table
    short *coef;                                  // the chain's first block
    int bpm, expb;                                // blocks per MCU, blocks of the chain
    long long room;                               // blocks from the chain's first to the frame's last
};

// Decodes the symbols that start before bit `sub_end`, from R's position in state (b, k): b the block of the MCU, k the zig-zag
// index of the next coefficient (0: the DC symbol is next).  `blk` counts the chain's blocks: with WRITE it is the block being
// decoded, coefficients are stored, decoding stops at the chain's last block and `st` collects status bits.
template <bool WRITE>
NSR_DEV void jpd_decode(const JpdChain &X, JpdReader &R, int &b, int &k, unsigned sub_end, int &blk, int &st) {
    while (R.pos < sub_end && (!WRITE || blk < X.expb)) {
        R.refill();
        const JpdHuff &T = X.huff[(k == 0 ? X.bdc[b & 7] : X.bac[b & 7]) & 7];
        const unsigned w = (unsigned)(R.buf >> 32);
        const unsigned e = T.lut[w >> 23];
        int len = (int)(e >> 8), sym = (int)(e & 255u);
        if (len == 0) {
            const int code = (int)(w >> 16);
            for (len = 10; len <= 16; ++len) {
                const int c = code >> (16 - len);
                if (c <= T.maxcode[len]) {
                    sym = T.vals[(c + T.valoff[len]) & 255];
                    break;
                }
            }
            if (len > 16) {                                          // no code: one bit on
                if (WRITE) st |= 1;
                R.skip(1);
                continue;
            }
        }
        const int s = sym & 15, r = sym >> 4;
        int v = 0;
        if (s) {
            const unsigned x = (w << len) >> (32 - s);
            v = x < (1u << (s - 1)) ? (int)x - (1 << s) + 1 : (int)x;
        }
        R.skip(len + s);
        const bool store = WRITE && blk < X.room;
        if (k == 0) {
            if (WRITE && r) st |= 1;                                 // a DC symbol above 15
            if (store) X.coef[64ll * blk] = (short)v;
            k = 1;
        } else if (s == 0) {
            k = r == 15 ? k + 16 : 64;
        } else {
            k += r;
            if (k > 63) {
                if (WRITE) st |= 2;
                k = 63;
            }
            if (store) X.coef[64ll * blk + k] = (short)v;
            ++k;
        }
        if (k >= 64) {
            k = 0;
            b = b + 1 >= X.bpm ? 0 : b + 1;
            ++blk;
        }
    }
}

// jpg_scan over the kJpdThreads lanes of the Huffman kernel's workgroup: the sum of the lower lanes' values, `total` that of all
NSR_DEV unsigned jpd_scan(unsigned *s, int t, unsigned v, unsigned &total) {
    int cur = 0;
    s[t] = v;
    block_sync();
    for (int d = 1; d < kJpdThreads; d <<= 1) {
        unsigned x = s[cur * kJpdThreads + t];
        if (t >= d) x += s[cur * kJpdThreads + t - d];
        cur ^= 1;
        s[cur * kJpdThreads + t] = x;
        block_sync();
    }
    const unsigned incl = s[cur * kJpdThreads + t];
    total = s[cur * kJpdThreads + kJpdThreads - 1];
    block_sync();
    return incl - v;
}

NSR_KERNEL NSR_BOUNDS(kJpdThreads) void jpegdec_huffman_kernel(const JpegDecParams P) {
    JpdHuff *huff = reinterpret_cast<JpdHuff *>(lds_base());
    unsigned *scan = reinterpret_cast<unsigned *>(lds_base() + kJpdHuffLds);
    unsigned *xpos = scan + 2 * kJpdThreads;
    int *xbk = reinterpret_cast<int *>(xpos + kJpdThreads);
    int *changed = xbk + kJpdThreads;                               // [2]
    int *stat = changed + 2;                                         // [4]: one word per status bit (plain stores of 1)
    unsigned char *bdc = reinterpret_cast<unsigned char *>(stat + 6), *bac = bdc + 8;
    const int t = tid(), f = bid_y();
    const nsr_jpegdec_frame &d = P.desc[f];
    const int len = jpd_scan_len(d), ri = d.restart_interval > 0 ? d.restart_interval : 0, nexp = jpd_intervals(P, ri);
    if (bid_x() >= nexp) return;                                     // more workgroups than the frame has chains

    // the frame's tables
    if (t < 8) {
        JpdHuff &T = huff[t];
        int code = 0, p = 0;
        T.maxcode[0] = -1;
        T.valoff[0] = 0;
        for (int l = 1; l <= 16; ++l) {
            const int nl = d.huff_bits[t][l - 1];
            T.valoff[l] = p - code;
            T.maxcode[l] = nl ? code + nl - 1 : -1;
            p += nl;
            code = (code + nl) << 1;
        }
        T.maxcode[17] = -1;
        T.valoff[17] = 0;
        const int comp = jpd_comp_of_block(P, t);
        bdc[t] = (unsigned char)(d.dc_table[comp & 3] & 3);
        bac[t] = (unsigned char)(4 + (d.ac_table[comp & 3] & 3));
    }
    for (int e = t; e < 8 * 256; e += kJpdThreads) huff[e >> 8].vals[e & 255] = d.huff_vals[e >> 8][e & 255];
    block_sync();
    for (int e = t; e < 8 * 512; e += kJpdThreads) {
        JpdHuff &T = huff[e >> 9];
        const int idx = e & 511;
        unsigned short v = 0;
        for (int l = 1; l <= 9; ++l) {
            const int c = idx >> (9 - l);
            if (c <= T.maxcode[l]) {
                v = (unsigned short)(l << 8 | T.vals[(c + T.valoff[l]) & 255]);
                break;
            }
        }
        T.lut[idx] = v;
    }
    block_sync();

    const int found = P.nfound[f], nuse = found + 1 < nexp ? found + 1 : nexp;
    const int *ist = P.istart + (long long)f * (P.M + 1);
    const unsigned SB = (unsigned)P.sub_bytes, L = (unsigned)kJpdThreads;
    for (int c = bid_x(); c < nexp; c += nblk_x()) {
        if (c >= nuse) {                                             // the scan holds no such interval
            if (t == 0) P.cstat[(long long)f * P.M + c] = 8;
            continue;
        }
        const int begin = ist[c], stop = c + 1 <= found ? ist[c + 1] - 2 : len;
        const unsigned clen = stop > begin ? (unsigned)(stop - begin) : 0u;
        const int mcus = ri > 0 ? (P.M - c * ri < ri ? P.M - c * ri : ri) : P.M;
        const long long first = (long long)c * ri * P.bpm;
        JpdChain X;
        X.huff = huff; X.bdc = bdc; X.bac = bac; X.bpm = P.bpm;
        X.expb = mcus * P.bpm;
        X.room = P.nblk - first;
        X.coef = P.coef + 64 * ((long long)f * P.nblk + first);
        JpdReader R;
        R.s = P.files + d.scan_begin + begin;
        R.end = clen;
        if (t < 4) stat[t] = 0;
        const unsigned nsub = (clen + SB - 1) / SB;
        // the last byte that holds bits: a chain may end in a stuffed pair
        const unsigned cbits = 8u * (clen >= 2u && R.s[clen - 2] == 0xffu && R.s[clen - 1] == 0u ? clen - 1u : clen);
        unsigned cpos = 0;                                           // the true state at the tile's first subsequence
        int cb = 0, ck = 0, cblk = 0, st = 0;
        block_sync();
        for (unsigned t0 = 0; t0 < nsub; t0 += L) {
            const unsigned i = t0 + t, nt = nsub - t0 < L ? nsub - t0 : L;
            const bool active = (unsigned)t < nt;
            const unsigned sub_end = 8u * ((i + 1) * SB < clen ? (i + 1) * SB : clen);
            unsigned spos = cpos, epos = 0;                          // the state this lane started from, and where it ended
            int sb = cb, sk = ck, eb = 0, ek = 0, cnt = 0;
            if (active) {
                if (t > 0) {                                         // speculation: the subsequence's first bit, a block's start
                    unsigned byte = i * SB;
                    if (R.byte(byte - 1) == 0xffu && R.byte(byte) == 0u) ++byte;      // (inside a stuffed pair)
                    spos = 8u * byte;
                    sb = sk = 0;
                }
                R.start(spos);
                eb = sb; ek = sk;
                jpd_decode<false>(X, R, eb, ek, sub_end, cnt, st);
                epos = R.pos;
            }
            xpos[t] = epos; xbk[t] = eb << 8 | ek;
            block_sync();
            for (unsigned r = 1; r < nt; ++r) {                      // at most nt - 1 rounds: after round r, r + 1 lanes are final
                bool redo = false;
                if (t == 0) changed[r & 1] = 0;
                if (active && t > 0 && (xpos[t - 1] != spos || xbk[t - 1] != (sb << 8 | sk))) {
                    spos = xpos[t - 1]; sb = xbk[t - 1] >> 8; sk = xbk[t - 1] & 255;
                    R.start(spos);
                    int nb = sb, nk = sk;
                    cnt = 0;
                    jpd_decode<false>(X, R, nb, nk, sub_end, cnt, st);
                    redo = R.pos != epos || nb != eb || nk != ek;
                    epos = R.pos; eb = nb; ek = nk;
                }
                block_sync();
                if (redo) {
                    xpos[t] = epos; xbk[t] = eb << 8 | ek;
                    changed[r & 1] = 1;
                }
                block_sync();
                if (!changed[r & 1]) break;
            }
            unsigned total;
            const unsigned before = jpd_scan(scan, t, active ? (unsigned)cnt : 0u, total);
            if (active) {
                const unsigned long long fb = (unsigned long long)cblk + before;
                int blk = fb > (unsigned long long)X.expb ? X.expb : (int)fb, wst = 0;
                R.start(spos);
                const bool open = blk < X.expb;
                jpd_decode<true>(X, R, sb, sk, sub_end, blk, wst);
                // the chain's bytes end before its blocks do, or its blocks a byte or more before its bytes
                if ((i == nsub - 1 && blk < X.expb) || (open && blk == X.expb && R.pos + 8u <= cbits)) wst |= 4;
                for (int q = 0; q < 3; ++q)
                    if (wst >> q & 1) stat[q] = 1;
            }
            cpos = xpos[nt - 1]; cb = xbk[nt - 1] >> 8; ck = xbk[nt - 1] & 255;
            cblk = (unsigned long long)cblk + total > (unsigned long long)X.expb ? X.expb : cblk + (int)total;
            block_sync();
        }
        if (t == 0) P.cstat[(long long)f * P.M + c] = (stat[0] ? 1 : 0) | (stat[1] ? 2 : 0) | (stat[2] || (nsub == 0 && X.expb > 0) ? 4 : 0);
        block_sync();
    }
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpegdec_dc_kernel(const JpegDecParams P) {
    unsigned long long *scan = reinterpret_cast<unsigned long long *>(lds_base());
    int *flags = reinterpret_cast<int *>(lds_base() + kJpgScanLds);  // [4]
    const int t = tid(), f = bid_y();
    const nsr_jpegdec_frame &d = P.desc[f];
    const int ri = d.restart_interval > 0 ? d.restart_interval : 0, nexp = jpd_intervals(P, ri);
    if (bid_x() == 0) {                                              // the frame's status
        if (t < 4) flags[t] = 0;
        block_sync();
        int st = 0;
        for (int c = t; c < nexp; c += kJpgThreads) st |= P.cstat[(long long)f * P.M + c];
        for (int q = 0; q < 4; ++q)
            if (st >> q & 1) flags[q] = 1;
        block_sync();
        if (t == 0) P.status[f] = P.mflags[f] | (P.nfound[f] + 1 != nexp ? 8 : 0) | (flags[0] ? 1 : 0) | (flags[1] ? 2 : 0) | (flags[2] ? 4 : 0) | (flags[3] ? 8 : 0);
    }
    for (int c = bid_x(); c < nexp; c += nblk_x()) {
        const int mcus = ri > 0 ? (P.M - c * ri < ri ? P.M - c * ri : ri) : P.M, expb = mcus * P.bpm;
        short *coef = P.coef + 64 * ((long long)f * P.nblk + (long long)c * ri * P.bpm);
        unsigned carry[3] = {0u, 0u, 0u};
        for (int j0 = 0; j0 < expb; j0 += kJpgThreads) {
            const int j = j0 + t, comp = jpd_comp_of_block(P, j % P.bpm);
            const unsigned v = j < expb ? (unsigned)(unsigned short)coef[64ll * j] : 0u;
            unsigned mine = 0;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                if (ci >= P.ncomp) break;
                unsigned long long total;
                const unsigned long long before = jpg_scan(scan, t, comp == ci ? v : 0u, total);
                if (comp == ci) mine = carry[ci] + (unsigned)before + v;
                carry[ci] += (unsigned)total;
            }
            if (j < expb) coef[64ll * j] = (short)(unsigned short)(mine & 0xffffu);
        }
    }
}

// libjpeg's jidctint on 8 values (a column of coef x Q, or a row of pass 1's results); SHIFT 11 in pass 1, 18 in pass 2
template <int SHIFT>
NSR_DEV void jpd_idct8(const int *in, int *out) {
    typedef long long L;
    L z2 = in[2], z3 = in[6];
    L z1 = (z2 + z3) * 4433;
    const L e2 = z1 + z3 * (-15137), e3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4];
    const L e0 = (z2 + z3) << 13, e1 = (z2 - z3) << 13;
    const L t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    L o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
    z1 = o0 + o3;
    z2 = o1 + o2;
    z3 = o0 + o2;
    L z4 = o1 + o3;
    const L z5 = (z3 + z4) * 9633;
    o0 *= 2446;
    o1 *= 16819;
    o2 *= 25172;
    o3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    constexpr L half = 1ll << (SHIFT - 1);
    out[0] = (int)((t10 + o3 + half) >> SHIFT);
    out[7] = (int)((t10 - o3 + half) >> SHIFT);
    out[1] = (int)((t11 + o2 + half) >> SHIFT);
    out[6] = (int)((t11 - o2 + half) >> SHIFT);
    out[2] = (int)((t12 + o1 + half) >> SHIFT);
    out[5] = (int)((t12 - o1 + half) >> SHIFT);
    out[3] = (int)((t13 + o0 + half) >> SHIFT);
    out[4] = (int)((t13 - o0 + half) >> SHIFT);
}

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpegdec_idct_kernel(const JpegDecParams P) {
    const long long g = (long long)bid_x() * kJpgThreads + tid();
    if (g >= P.n * P.nblk) return;
    const long long f = g / P.nblk, j = g - f * P.nblk, mcu = j / P.bpm;
    const int b = (int)(j - mcu * P.bpm), comp = jpd_comp_of_block(P, b);
    const int my = (int)(mcu / P.mcux), mx = (int)(mcu - (long long)my * P.mcux);
    const unsigned char *q = P.desc[f].quant[comp];
    const unsigned *src = reinterpret_cast<const unsigned *>(P.coef + 64 * g);           // 128-byte aligned
    int w[64];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const unsigned u = src[k];
        w[kJpgZigzag[2 * k]] = (int)(short)(u & 0xffffu) * (int)q[2 * k];
        w[kJpgZigzag[2 * k + 1]] = (int)(short)(u >> 16) * (int)q[2 * k + 1];
    }
    int in[8], o[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {                                    // pass 1: columns
#pragma unroll
        for (int y = 0; y < 8; ++y) in[y] = w[8 * y + x];
        jpd_idct8<11>(in, o);
#pragma unroll
        for (int y = 0; y < 8; ++y) w[8 * y + x] = o[y];
    }
    int pw, bx, by;
    unsigned char *plane = P.planes + f * P.plane_bytes;
    if (comp == 0) {
        pw = P.pw_y;
        bx = mx * P.hs + b % P.hs;
        by = my * P.vs + b / P.hs;
    } else {
        pw = P.pw_c;
        bx = mx;
        by = my;
        plane += P.poff_c + (long long)(comp - 1) * P.pw_c * P.ph_c;
    }
    unsigned char *dst = plane + 8ll * by * pw + 8 * bx;
#pragma unroll
    for (int y = 0; y < 8; ++y) {                                    // pass 2: rows
        jpd_idct8<18>(w + 8 * y, o);
        unsigned long long row = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int v = o[x] + 128;
            row |= (unsigned long long)(v < 0 ? 0 : (v > 255 ? 255 : v)) << (8 * x);
        }
        *reinterpret_cast<unsigned long long *>(dst + (long long)y * pw) = row;          // (planes and their widths are multiples of 8 bytes)
    }
}

// the chroma sample of plane c (cw x ch of a plane pw_c wide) at output pixel (x, y), upsampled
NSR_DEV int jpd_chroma(const JpegDecParams &P, const unsigned char *c, int x, int y) {
    if (P.hs == 1) return c[(long long)y * P.pw_c + x];
    const int cx = x >> 1, last = P.cw - 1;
    if (P.vs == 1) {                                                 // h2v1
        const unsigned char *r = c + (long long)y * P.pw_c;
        const int p = r[cx];
        if (x & 1) return cx == last ? p : (3 * p + r[cx + 1] + 2) >> 2;
        return cx == 0 ? p : (3 * p + r[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;                                           // h2v2
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > P.ch - 1 ? P.ch - 1 : fy);
    const unsigned char *near = c + (long long)cy * P.pw_c, *far = c + (long long)fy * P.pw_c;
    const int s = 3 * near[cx] + far[cx];
    if (x & 1) return cx == last ? (4 * s + 7) >> 4 : (3 * s + 3 * near[cx + 1] + far[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[cx - 1] + far[cx - 1] + 8) >> 4;
}

NSR_DEV int jpd_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

NSR_KERNEL NSR_BOUNDS(kJpgThreads) void jpegdec_color_kernel(const JpegDecParams P) {
    const long long g = (long long)bid_x() * kJpgThreads + tid(), hw = (long long)P.H * P.W;
    if (g >= P.n * hw) return;
    const long long f = g / hw, p = g - f * hw;
    const int y = (int)(p / P.W), x = (int)(p - (long long)y * P.W);
    const unsigned char *plane = P.planes + f * P.plane_bytes;
    const int Y = plane[(long long)y * P.pw_y + x];
    unsigned char *dst = P.out + 3 * g;
    if (P.ncomp == 1) {
        dst[0] = dst[1] = dst[2] = (unsigned char)Y;
        return;
    }
    const unsigned char *cbp = plane + P.poff_c, *crp = cbp + (long long)P.pw_c * P.ph_c;
    const int cb = jpd_chroma(P, cbp, x, y) - 128, cr = jpd_chroma(P, crp, x, y) - 128;
    dst[0] = (unsigned char)jpd_clamp255(Y + ((91881 * cr + 32768) >> 16));
    dst[1] = (unsigned char)jpd_clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[2] = (unsigned char)jpd_clamp255(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace nsr
