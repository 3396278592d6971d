// bfq_gzip.h -- plain gzip (RFC 1952 members around one long deflate stream each, RFC 1951), inflated side by side.  Plain
// C++, shared by the kernels (k_gzip.hip), the host side (bfq_gzip.hip) and the sanitizer program (tests/cxx/test_gzip.cpp).
// The bit reader, the table builder, the symbol decoder and the CRC combine are bfq_bgzf.h's.
//
// A gzip member has no directory, so the starts of independent work are found and proved instead of read:
//   pieces      the compressed bytes are cut at multiples of `chunk`.  Piece 0 starts at the first member's first block.  The
//               *candidate* of a later piece is the first bit offset inside it at which the block-start rule holds
//               (bfq_gzip_cheap, then bfq_gzip_full): BFINAL = 0, BTYPE = 2 and a header that passes every check the inflate
//               makes.  A piece without a candidate has no decoder: its bytes belong to the decoder before it.
//   pass 1      every decoder runs from its start, block by block (bfq_gzip_run without an output), until a block ends
//               exactly on a later piece's candidate (its *landing*), the final block of the last member ends, or an error.
//               It crosses member ends: trailer, next header.  The host walks the landings from piece 0: the *chain*
//               (bfq_gzip_plan).  Decoders off the chain -- false candidates -- are discarded.  Nothing rests on a candidate
//               being true: what counts is the chain, and in the end every member's CRC32.
//   pass 2      the chain's decoders run again and write one u16 per output byte: 0..255 a literal byte, 0x8000 | w byte w
//               of the 32 KiB before the decoder's first byte (w = 32767: the byte just before it).  Matches copy symbols,
//               so markers replicate.
//   windows     the resolved last 32 KiB in front of every chain decoder, in chain order (bfq_gzip_window_sym).
//   resolve     every symbol becomes a byte (bfq_gzip_resolve_sym).  A marker that reaches before its member's first byte
//               is the DIST_FAR the decoder could not see (it did not know where its member began).
//   CRC32       of every member from equal sub-ranges of the text, combined with bfq_crc32_shift (bfq_gzip_crc_range).
// bfq_gzip_host() runs all of it in one thread; the device runs the same functions with 64 lanes per decoder.
#pragma once
#include <new>
#include <vector>
#include "bfq_bgzf.h"

#define BFQ_GZIP_WIN 32768u                       // the deflate window
#define BFQ_GZIP_MIN_CHUNK 512u
#define BFQ_GZIP_DEF_CHUNK 131072u                // the default piece (profiles/gzip/README.md)
#define BFQ_GZIP_CRC_RANGE 4096u                  // bytes of text per CRC sub-range
#define BFQ_GZIP_NONE (~0ull)

// reasons beside bfq_bgzf.h's
enum {
    BFQ_GZIP_E_RESERVED = BFQ_BGZF_E_NUM,         // FLG bits 5..7
    BFQ_GZIP_E_HCRC,                              // FHCRC differs from the CRC16 of the header
    BFQ_GZIP_E_FIELD,                             // FEXTRA, FNAME, FCOMMENT or FHCRC runs past the end of the input
    BFQ_GZIP_E_GARBAGE,                           // bytes after a member that are neither zero to the end nor a member
    BFQ_GZIP_E_TRAILER,                           // the input ends inside CRC32 + ISIZE
    BFQ_GZIP_E_NUM
};
BFQ_HD const char *bfq_gzip_reason(int r)
{
    switch (r) {
    case BFQ_GZIP_E_RESERVED: return "reserved gzip flag bits are set";
    case BFQ_GZIP_E_HCRC: return "header CRC16 mismatch";
    case BFQ_GZIP_E_FIELD: return "a header field runs past the end of the input";
    case BFQ_GZIP_E_GARBAGE: return "trailing bytes that are neither zero nor a gzip member";
    case BFQ_GZIP_E_TRAILER: return "the input ends inside the member trailer";
    }
    return bfq_bgzf_reason(r);
}

// what a decoder leaves (pass 1)
enum { BFQ_GZIP_ST_LAND = 0, BFQ_GZIP_ST_END = 1, BFQ_GZIP_ST_NONE = 2, BFQ_GZIP_ST_ERR = 0x100 };   // ERR | reason
struct bfq_gzip_rec {
    u64 endBit;          // where it stopped
    u64 produced;        // bytes of text
    u64 tail;            // ... of them in the member it stopped in (known != 0), else = produced
    u64 lastHdr;         // offset of the header of the member it stopped in, NONE: that member began before this decoder
    u32 land;            // ST_LAND: the piece whose candidate it stopped on
    u32 nEnds;           // member ends it crossed
    u32 status;
    u32 known;           // it crossed a member start (or is piece 0): it knows where its last member began
};
// a decoder of the chain (pass 2)
struct bfq_gzip_job {
    u64 startBit, outOff, produced, endsOff;
    u64 memberPre;       // bytes of its first member that precede its first byte
    u32 nEnds, first;    // first: piece 0, which begins with the member header at byte 0
};
struct bfq_gzip_end { u64 outPos, nextHdr; u32 crc, isize; };   // member i ends before text byte outPos; the next header, NONE: the stream ends

// ---------------------------------------------------------------- member header (RFC 1952)
BFQ_HD u32 bfq_gzip_crc_byte(u32 c, u8 v) { return bfq_crc32_entry((c ^ v) & 0xFFu) ^ (c >> 8); }
// the member at in[off]: *dataOff = where its deflate data begins
BFQ_HD int bfq_gzip_member_header(const u8 *in, u64 len, u64 off, u64 *dataOff)
{
    const u64 avail = len - off;
    const u8 *p = in + off;
    if (avail < 2) return BFQ_BGZF_E_SHORT;
    if (p[0] != 0x1F || p[1] != 0x8B) return BFQ_BGZF_E_NOT_GZIP;
    if (avail < 10) return BFQ_BGZF_E_SHORT;
    if (p[2] != 8) return BFQ_BGZF_E_NOT_GZIP;
    const u32 flg = p[3];
    if (flg & 0xE0u) return BFQ_GZIP_E_RESERVED;
    u64 q = 10;
    if (flg & 4u) {
        if (avail - q < 2) return BFQ_GZIP_E_FIELD;
        const u32 xlen = bfq_bgzf_le16(p + q);
        q += 2;
        if (avail - q < xlen) return BFQ_GZIP_E_FIELD;
        q += xlen;
    }
    for (u32 f = 8; f <= 16; f <<= 1)             // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (q < avail && p[q]) q++;
            if (q >= avail) return BFQ_GZIP_E_FIELD;
            q++;
        }
    if (flg & 2u) {
        if (avail - q < 2) return BFQ_GZIP_E_FIELD;
        u32 c = 0xFFFFFFFFu;
        for (u64 i = 0; i < q; i++) c = bfq_gzip_crc_byte(c, p[i]);
        if ((~c & 0xFFFFu) != bfq_bgzf_le16(p + q)) return BFQ_GZIP_E_HCRC;
        q += 2;
    }
    *dataOff = off + q;
    return BFQ_BGZF_OK;
}

// ---------------------------------------------------------------- the bit reader over a whole file
// bfq_bgzf_bits counts in 32 bits: it is pointed at the byte of a bit offset and sees at most 2 GiB from there; the symbol
// loop moves it on long before that runs out.
BFQ_HD void bfq_gzip_seek(bfq_bgzf_bits &b, const u8 *in, u64 len, u64 bit)       // bit <= 8 len
{
    const u64 byte = bit >> 3, left = len - byte;
    b.p = in + byte; b.n = left > 0x80000000ull ? 0x80000000u : (u32)left;
    b.pos = 0; b.buf = 0; b.cnt = 0;
    bfq_bgzf_refill(b);
    if (bit & 7u) bfq_bgzf_take(b, (u32)(bit & 7u));
}
BFQ_HD u64 bfq_gzip_tell(const bfq_bgzf_bits &b, const u8 *in) { return ((u64)(b.p - in) + b.pos) * 8 - b.cnt; }
// n <= 57 bits from a bit offset; bits past the end of the input read as zero
BFQ_HD u64 bfq_gzip_peek(const u8 *in, u64 len, u64 bit, u32 n)
{
    const u64 byte = bit >> 3;
    u64 v = 0;
    for (u32 i = 0; i < 8; i++)
        if (byte + i < len) v |= (u64)in[byte + i] << (8 * i);
    return (v >> (bit & 7u)) & ((1ull << n) - 1ull);
}

// ---------------------------------------------------------------- the block-start rule
// cheap: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a complete code-length code (Kraft sum over the HCLEN lengths)
BFQ_HD bool bfq_gzip_head17(u32 v) { return (v & 7u) == 4u && ((v >> 3) & 31u) <= 29u && ((v >> 8) & 31u) <= 29u; }
BFQ_HD bool bfq_gzip_cheap(const u8 *in, u64 len, u64 bit)
{
    const u32 v = (u32)bfq_gzip_peek(in, len, bit, 17);
    if (!bfq_gzip_head17(v)) return false;
    const u32 hclen = ((v >> 13) & 15u) + 4;
    if (bit + 17 + 3 * hclen > 8 * len) return false;
    const u64 w = bfq_gzip_peek(in, len, bit + 17, 57);
    u32 kraft = 0;
    for (u32 i = 0; i < hclen; i++) {
        const u32 l = (u32)(w >> (3 * i)) & 7u;
        if (l) kraft += 128u >> l;
    }
    return kraft == 128u;
}
// full: the code lengths decode (no bad repeat), symbol 256 has a code, the literal/length set is complete, the distance set
// is complete, empty, or the single one-bit code.  One lane; H is its scratch.
struct bfq_gzip_hdrtab { u16 fast[128], sym[19], count[16], offs[16]; u8 cl[20]; };
BFQ_HD bool bfq_gzip_full(const u8 *in, u64 len, u64 bit, bfq_gzip_hdrtab *H)
{
    bfq_bgzf_bits b;
    bfq_gzip_seek(b, in, len, bit);
    if (b.cnt < 17) return false;
    bfq_bgzf_take(b, 3);
    const u32 hlit = bfq_bgzf_take(b, 5) + 257, hdist = bfq_bgzf_take(b, 5) + 1, hclen = bfq_bgzf_take(b, 4) + 4;
    if (hlit > 286 || hdist > 30) return false;
    for (u32 i = 0; i < 19; i++) H->cl[i] = 0;
    const char *order = "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017";
    for (u32 i = 0; i < hclen; i++) {
        bfq_bgzf_refill(b);
        if (b.cnt < 3) return false;
        H->cl[(u8)order[i]] = (u8)bfq_bgzf_take(b, 3);
    }
    if (bfq_bgzf_build(H->cl, 19, H->count, H->sym, H->offs, H->fast, 7) != 0) return false;
    u32 lc[16], dc[16];
    for (u32 i = 0; i < 16; i++) lc[i] = dc[i] = 0;
    u32 idx = 0, prev = 0;
    const u32 want = hlit + hdist;
    bool eob = false;
    while (idx < want) {
        bfq_bgzf_refill(b);
        const int s = bfq_bgzf_decode(b, H->fast, 7, H->count, H->sym);
        if (s < 0) return false;
        u32 rep = 1, val = 0;
        if (s < 16) val = (u32)s;
        else if (s == 16) {
            if (idx == 0 || b.cnt < 2) return false;
            rep = 3 + bfq_bgzf_take(b, 2); val = prev;
        } else if (s == 17) {
            if (b.cnt < 3) return false;
            rep = 3 + bfq_bgzf_take(b, 3);
        } else {
            if (b.cnt < 7) return false;
            rep = 11 + bfq_bgzf_take(b, 7);
        }
        if (rep > want - idx) return false;
        for (u32 r = 0; r < rep; r++) {
            if (idx + r < hlit) { lc[val]++; if (idx + r == 256 && val) eob = true; }
            else dc[val]++;
        }
        idx += rep; prev = val;
    }
    if (!eob) return false;
    int left = 1;
    for (u32 l = 1; l <= 15; l++) { left <<= 1; left -= (int)lc[l]; if (left < 0) return false; }
    if (left) return false;
    if (dc[0] == hdist) return true;
    left = 1;
    u32 codes = 0;
    for (u32 l = 1; l <= 15; l++) { left <<= 1; left -= (int)dc[l]; codes += dc[l]; if (left < 0) return false; }
    return left == 0 || (codes == 1 && dc[1] == 1);
}
// the candidate of piece k >= 1 (one thread): the first bit offset of the piece where the rule holds, NONE: nowhere
BFQ_HD u64 bfq_gzip_candidate(const u8 *in, u64 len, u64 chunk, u64 k, bfq_gzip_hdrtab *H)
{
    const u64 lo = k * chunk * 8, hi = (k + 1) * chunk < len ? (k + 1) * chunk * 8 : len * 8;
    for (u64 bit = lo; bit < hi; bit++)
        if (bfq_gzip_cheap(in, len, bit) && bfq_gzip_full(in, len, bit, H)) return bit;
    return BFQ_GZIP_NONE;
}

// ---------------------------------------------------------------- one decoder (pass 1: sym == ends == nullptr; pass 2: both given)
// `nl` cooperating lanes, this one `lane`: control flow is the same in every lane (bfq_bgzf.h).  sym = the symbols of this
// decoder, [0, J.produced): nothing is written outside them; ends = its member ends, [0, J.nEnds).  Reads nothing outside
// in[0, len).  Every loop consumes input bits or ends.
BFQ_HD void bfq_gzip_run(const u8 *in, u64 len, u64 chunk, const u64 *cand, u64 npieces, const bfq_gzip_job &J, u16 *sym, bfq_gzip_end *ends,
                         bfq_bgzf_tables *T, u32 lane, u32 nl, bfq_gzip_rec *R)
{
    bfq_bgzf_bits b;
    u64 op = 0, base = 0, hdrOff = BFQ_GZIP_NONE, bit = J.startBit;
    u32 nEnds = 0, known = 0, land = 0;
    int st = -1;                                                  // -1: running
    bool begun = false, fixedBuilt = false;
    if (J.first) {
        hdrOff = 0; known = 1;
        u64 data = 0;
        const int r = len ? bfq_gzip_member_header(in, len, 0, &data) : BFQ_BGZF_E_SHORT;
        if (r) st = BFQ_GZIP_ST_ERR | r;
        bit = data * 8;
    }
    if (st < 0) bfq_gzip_seek(b, in, len, bit);
    else { b.p = in; b.n = 0; b.pos = 0; b.buf = 0; b.cnt = 0; }
#define BFQ_GZIP_FAIL(r) { st = BFQ_GZIP_ST_ERR | (r); break; }
    while (st < 0) {
        if (begun) {
            const u64 P = bfq_gzip_tell(b, in), q = P / (chunk * 8);
            if (q > 0 && q < npieces && cand[q] == P) { land = (u32)q; st = BFQ_GZIP_ST_LAND; break; }
        }
        begun = true;
        bfq_bgzf_refill(b);
        if (b.cnt < 3) BFQ_GZIP_FAIL(BFQ_BGZF_E_PAYLOAD_END)
        const u32 last = bfq_bgzf_take(b, 1), type = bfq_bgzf_take(b, 2);
        if (type == 3) BFQ_GZIP_FAIL(BFQ_BGZF_E_BTYPE)
        if (type == 0) {
            bfq_bgzf_take(b, b.cnt & 7u);
            u64 src = (u64)(b.p - in) + b.pos - b.cnt / 8;
            if (len - src < 4) BFQ_GZIP_FAIL(BFQ_BGZF_E_PAYLOAD_END)
            const u32 n = bfq_bgzf_le16(in + src), nn = bfq_bgzf_le16(in + src + 2);
            src += 4;
            if (n != (~nn & 0xFFFFu)) BFQ_GZIP_FAIL(BFQ_BGZF_E_STORED_LEN)
            if (n > len - src) BFQ_GZIP_FAIL(BFQ_BGZF_E_STORED_RUN)
            if (sym)
                for (u32 i = lane; i < n; i += nl)
                    if (op + i < J.produced) sym[op + i] = in[src + i];
            op += n;
            bfq_gzip_seek(b, in, len, (src + n) * 8);
        } else {
            if (type == 1) {
                if (!fixedBuilt) {
                    BFQ_BGZF_SYNC();
                    if (lane == 0) {
                        for (u32 i = 0; i < 288; i++) T->lens[i] = (u8)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                        for (u32 i = 288; i < 320; i++) T->lens[i] = 5;
                        bfq_bgzf_build(T->lens, 288, T->lcount, T->lsym, T->offs, T->lfast, BFQ_BGZF_LBITS);
                        bfq_bgzf_build(T->lens + 288, 32, T->dcount, T->dsym, T->offs, T->dfast, BFQ_BGZF_DBITS);
                    }
                    BFQ_BGZF_SYNC();
                    fixedBuilt = true;
                }
            } else {
                fixedBuilt = false;
                bfq_bgzf_refill(b);
                if (b.cnt < 14) BFQ_GZIP_FAIL(BFQ_BGZF_E_PAYLOAD_END)
                const u32 hlit = bfq_bgzf_take(b, 5) + 257, hdist = bfq_bgzf_take(b, 5) + 1, hclen = bfq_bgzf_take(b, 4) + 4;
                if (hlit > 286 || hdist > 30) BFQ_GZIP_FAIL(BFQ_BGZF_E_HLIT_HDIST)
                BFQ_BGZF_SYNC();
                if (lane == 0)
                    for (u32 i = 0; i < 19; i++) T->cl[i] = 0;
                const char *order = "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017";
                int hs = 0;
                for (u32 i = 0; i < hclen; i++) {
                    bfq_bgzf_refill(b);
                    if (b.cnt < 3) { hs = BFQ_BGZF_E_PAYLOAD_END; break; }
                    const u32 v = bfq_bgzf_take(b, 3);
                    if (lane == 0) T->cl[(u8)order[i]] = (u8)v;
                }
                if (hs) BFQ_GZIP_FAIL(hs)
                if (lane == 0) {
                    const int r = bfq_bgzf_build(T->cl, 19, T->dcount, T->dsym, T->offs, T->dfast, 7);
                    T->st = r < 0 ? BFQ_BGZF_E_OVERSUB : r > 0 ? BFQ_BGZF_E_INCOMPLETE : BFQ_BGZF_OK;
                }
                BFQ_BGZF_SYNC();
                if (T->st) BFQ_GZIP_FAIL(T->st)
                u32 idx = 0, prev = 0;
                const u32 want = hlit + hdist;
                while (idx < want) {
                    bfq_bgzf_refill(b);
                    const int s = bfq_bgzf_decode(b, T->dfast, 7, T->dcount, T->dsym);
                    if (s < 0) { hs = s == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE; break; }
                    if (s < 16) {
                        if (lane == 0) T->lens[idx] = (u8)s;
                        idx++; prev = (u32)s;
                        continue;
                    }
                    u32 rep, val = 0;
                    if (s == 16) {
                        if (idx == 0) { hs = BFQ_BGZF_E_REP_FIRST; break; }
                        if (b.cnt < 2) { hs = BFQ_BGZF_E_PAYLOAD_END; break; }
                        rep = 3 + bfq_bgzf_take(b, 2); val = prev;
                    } else if (s == 17) {
                        if (b.cnt < 3) { hs = BFQ_BGZF_E_PAYLOAD_END; break; }
                        rep = 3 + bfq_bgzf_take(b, 3);
                    } else {
                        if (b.cnt < 7) { hs = BFQ_BGZF_E_PAYLOAD_END; break; }
                        rep = 11 + bfq_bgzf_take(b, 7);
                    }
                    if (rep > want - idx) { hs = BFQ_BGZF_E_REP_OVER; break; }
                    if (lane == 0)
                        for (u32 i = 0; i < rep; i++) T->lens[idx + i] = (u8)val;
                    idx += rep; prev = val;
                }
                if (hs) BFQ_GZIP_FAIL(hs)
                BFQ_BGZF_SYNC();
                if (lane == 0) {
                    int ts = BFQ_BGZF_OK;
                    if (T->lens[256] == 0) ts = BFQ_BGZF_E_NO_EOB;
                    if (!ts) {
                        const int r = bfq_bgzf_build(T->lens, hlit, T->lcount, T->lsym, T->offs, T->lfast, BFQ_BGZF_LBITS);
                        ts = r < 0 ? BFQ_BGZF_E_OVERSUB : r > 0 ? BFQ_BGZF_E_INCOMPLETE : BFQ_BGZF_OK;
                    }
                    if (!ts) {
                        // (the single one-bit distance code and the empty distance set stand: bfq_bgzf.h)
                        const int r = bfq_bgzf_build(T->lens + hlit, hdist, T->dcount, T->dsym, T->offs, T->dfast, BFQ_BGZF_DBITS);
                        if (r < 0) ts = BFQ_BGZF_E_OVERSUB;
                        else if (r == 1) {
                            u32 codes = 0;
                            for (u32 l = 1; l <= 15; l++) codes += T->dcount[l];
                            if (!(codes == 1 && T->dcount[1] == 1)) ts = BFQ_BGZF_E_INCOMPLETE;
                        }
                    }
                    T->st = ts;
                }
                BFQ_BGZF_SYNC();
                if (T->st) BFQ_GZIP_FAIL(T->st)
            }
            // the block's symbols
            int bs = 0;
            for (;;) {
                if (b.pos > (1u << 30)) bfq_gzip_seek(b, in, len, bfq_gzip_tell(b, in));
                bfq_bgzf_refill(b);
                const int s = bfq_bgzf_decode(b, T->lfast, BFQ_BGZF_LBITS, T->lcount, T->lsym);
                if (s < 0) { bs = s == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE; break; }
                if (s < 256) {
                    if (sym && lane == 0 && op < J.produced) sym[op] = (u16)s;
                    op++;
                    continue;
                }
                if (s == 256) break;
                if (s >= 286) { bs = BFQ_BGZF_E_LITSYM; break; }
                u32 n;
                if (s == 285) n = 258;
                else {
                    const u32 i = (u32)s - 257;
                    if (i < 8) n = 3 + i;
                    else {
                        const u32 ext = (i >> 2) - 1;
                        if (b.cnt < ext) { bs = BFQ_BGZF_E_PAYLOAD_END; break; }
                        n = 3 + ((4 + (i & 3u)) << ext) + bfq_bgzf_take(b, ext);
                    }
                }
                bfq_bgzf_refill(b);
                const int ds = bfq_bgzf_decode(b, T->dfast, BFQ_BGZF_DBITS, T->dcount, T->dsym);
                if (ds < 0) { bs = ds == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE; break; }
                if (ds >= 30) { bs = BFQ_BGZF_E_DISTSYM; break; }
                u32 dist;
                if (ds < 4) dist = 1 + (u32)ds;
                else {
                    const u32 ext = ((u32)ds >> 1) - 1;
                    if (b.cnt < ext) { bs = BFQ_BGZF_E_PAYLOAD_END; break; }
                    dist = 1 + ((2 + ((u32)ds & 1u)) << ext) + bfq_bgzf_take(b, ext);
                }
                // a decoder that knows where its member began sees a far distance itself; one that does not leaves markers
                if (known && dist > op - base) { bs = BFQ_BGZF_E_DIST_FAR; break; }
                if (sym) {
                    BFQ_BGZF_SYNC();                              // the symbols of earlier tokens, stored by other lanes
                    for (u32 i = lane; i < n; i += nl) {
                        const long long p = (long long)op - (long long)dist + (long long)(i % dist);
                        const u16 v = p >= 0 ? sym[p] : (u16)(0x8000u | (u32)((long long)BFQ_GZIP_WIN + p));
                        if (op + i < J.produced) sym[op + i] = v;
                    }
                }
                op += n;
            }
            if (bs) BFQ_GZIP_FAIL(bs)
        }
        if (!last) continue;
        // the member ends: CRC32, ISIZE, and what follows -- nothing, zero bytes to the end, or the next member
        const u64 tr = (bfq_gzip_tell(b, in) + 7) >> 3;
        if (len - tr < 8) BFQ_GZIP_FAIL(BFQ_GZIP_E_TRAILER)
        const u64 nxt = tr + 8;
        bool more = nxt < len, garbage = false;
        if (more && in[nxt] != 0x1F) {
            BFQ_BGZF_SYNC();
            u32 nz = 0;
            for (u64 i = nxt + lane; i < len; i += nl) nz |= in[i];
            T->crc[lane] = nz;
            BFQ_BGZF_SYNC();
            nz = 0;
            for (u32 i = 0; i < nl; i++) nz |= T->crc[i];
            more = false; garbage = nz != 0;
        }
        if (ends && lane == 0 && nEnds < J.nEnds)
            ends[nEnds] = bfq_gzip_end{J.outOff + op, more || garbage ? nxt : BFQ_GZIP_NONE, bfq_bgzf_le32(in + tr), bfq_bgzf_le32(in + tr + 4)};
        nEnds++;
        if (garbage) { hdrOff = nxt; known = 1; base = op; BFQ_GZIP_FAIL(BFQ_GZIP_E_GARBAGE) }
        if (!more) { st = BFQ_GZIP_ST_END; bfq_gzip_seek(b, in, len, len * 8); break; }
        hdrOff = nxt; known = 1; base = op;
        u64 data = 0;
        const int r = bfq_gzip_member_header(in, len, nxt, &data);
        if (r) BFQ_GZIP_FAIL(r)
        bfq_gzip_seek(b, in, len, data * 8);
    }
#undef BFQ_GZIP_FAIL
    if (lane == 0) {
        R->endBit = bfq_gzip_tell(b, in); R->produced = op; R->tail = op - base; R->lastHdr = hdrOff;
        R->land = land; R->nEnds = nEnds; R->status = (u32)st; R->known = known;
    }
}

// ---------------------------------------------------------------- windows and resolve
// entry i of the window behind a decoder of `produced` symbols s[], from the window W in front of it
BFQ_HD u8 bfq_gzip_window_sym(const u16 *s, u64 produced, const u8 *W, u32 i)
{
    u16 v;
    if (produced >= BFQ_GZIP_WIN) v = s[produced - BFQ_GZIP_WIN + i];
    else if (i < BFQ_GZIP_WIN - produced) return W[i + produced];
    else v = s[i - (BFQ_GZIP_WIN - produced)];
    return v < 0x8000u ? (u8)v : W[v & 0x7FFFu];
}
// a symbol as a byte; *far when it reaches before the first byte of the member (memberPre bytes of which precede the decoder)
BFQ_HD u8 bfq_gzip_resolve_sym(u16 v, const u8 *W, u64 memberPre, bool *far)
{
    if (v < 0x8000u) return (u8)v;
    const u32 w = v & 0x7FFFu;
    if (BFQ_GZIP_WIN - w > memberPre) *far = true;
    return W[w];
}

// ---------------------------------------------------------------- CRC32 of the members
// the first member that ends behind text byte p
BFQ_HD u64 bfq_gzip_member_of(const bfq_gzip_end *ends, u64 nEnds, u64 p)
{
    u64 lo = 0, hi = nEnds;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (ends[mid].outPos <= p) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// sub-range r of the text: the CRC of its share of every member it touches, moved to the member's end; the XOR of a
// member's shares is its CRC32.  add(m, v): crc[m] ^= v (atomic on the device).
template <class Add> BFQ_HD void bfq_gzip_crc_range(const u32 *tab, const u8 *text, u64 raw, u64 r, const bfq_gzip_end *ends, u64 nEnds, Add add)
{
    u64 lo = r * BFQ_GZIP_CRC_RANGE;
    const u64 hi = lo + BFQ_GZIP_CRC_RANGE < raw ? lo + BFQ_GZIP_CRC_RANGE : raw;
    u64 m = bfq_gzip_member_of(ends, nEnds, lo);
    while (lo < hi && m < nEnds) {
        const u64 end = ends[m].outPos, to = end < hi ? end : hi;
        add(m, bfq_crc32_shift(bfq_crc32_serial(tab, text + lo, to - lo), end - to));
        lo = to;
        if (lo == end) m = bfq_gzip_member_of(ends, nEnds, lo);
    }
}

// ---------------------------------------------------------------- the chain (host)
struct bfq_gzip_err { int reason = 0; u64 member = 0, off = 0; };
// Walks the landings from piece 0.  jobs = the chain; *raw = bytes of text, *nEnds = member ends of the chain.  A chain that
// ends in an error leaves it in *E (reason != 0); its jobs still stand (the text in front of the error is resolved to look
// for a far distance, which lies lower in the stream).
inline void bfq_gzip_plan(const bfq_gzip_rec *recs, const u64 *cand, u64 npieces, u64 chunk, std::vector<bfq_gzip_job> &jobs, bfq_gzip_stats *S,
                          u64 *raw, u64 *nEnds, bfq_gzip_err *E)
{
    jobs.clear();
    *E = bfq_gzip_err{};
    u64 out = 0, ends = 0, pre = 0, hdr = 0, k = 0, skipped = 0, started = 1;
    for (u64 q = 1; q < npieces; q++) started += cand[q] != BFQ_GZIP_NONE;
    for (;;) {
        const bfq_gzip_rec &r = recs[k];
        jobs.push_back(bfq_gzip_job{k ? cand[k] : 0, out, r.produced, ends, pre, r.nEnds, k == 0 ? 1u : 0u});
        out += r.produced; ends += r.nEnds;
        pre = r.known ? r.tail : pre + r.produced;
        if (r.lastHdr != BFQ_GZIP_NONE) hdr = r.lastHdr;
        // the candidates this decoder ran past
        const u64 qEnd = r.endBit / (chunk * 8);
        for (u64 q = k + 1; q < npieces && q <= qEnd; q++)
            if (cand[q] != BFQ_GZIP_NONE && cand[q] < r.endBit && !(r.status == BFQ_GZIP_ST_LAND && q == r.land)) skipped++;
        if (r.status == BFQ_GZIP_ST_LAND) { k = r.land; continue; }
        if (r.status != BFQ_GZIP_ST_END) { E->reason = (int)(r.status & 0xFFu); E->member = ends; E->off = hdr; }
        break;
    }
    *raw = out; *nEnds = ends;
    S->members = ends; S->pieces = npieces; S->decoders = started; S->chain = jobs.size(); S->skipped = skipped; S->discarded = started - jobs.size();
}
// the member that holds text byte p and where its header lies
inline void bfq_gzip_locate(const bfq_gzip_end *ends, u64 nEnds, u64 p, u64 *member, u64 *off)
{
    *member = bfq_gzip_member_of(ends, nEnds, p);
    *off = *member ? ends[*member - 1].nextHdr : 0;
}
// CRC32 and length (mod 2^32) of every member against its trailer, lowest member first
inline void bfq_gzip_check_members(const bfq_gzip_end *ends, u64 nEnds, const u32 *crc, bfq_gzip_err *E)
{
    for (u64 m = 0; m < nEnds && !E->reason; m++) {
        const u64 from = m ? ends[m - 1].outPos : 0;
        if ((u32)(ends[m].outPos - from) != ends[m].isize) E->reason = BFQ_BGZF_E_LENGTH;
        else if (crc[m] != ends[m].crc) E->reason = BFQ_BGZF_E_CRC;
        if (E->reason) { E->member = m; E->off = m ? ends[m - 1].nextHdr : 0; }
    }
}
inline u64 bfq_gzip_pieces(u64 len, u64 chunk) { return len ? (len + chunk - 1) / chunk : 1; }
inline bool bfq_gzip_chunk_ok(u64 chunk) { return chunk >= BFQ_GZIP_MIN_CHUNK && (chunk & (chunk - 1)) == 0; }

// All of it in one thread.  out == nullptr: steps 2-3 only (*rawLen, *S).  0: done; 1: refused (*E); 2: cap < *rawLen
// (nothing written); 3: out of memory.
inline int bfq_gzip_host(const u8 *in, u64 len, u64 chunk, u8 *out, u64 cap, bool measure, u64 *rawLen, bfq_gzip_stats *S, bfq_gzip_err *E)
{
    try {
        const u64 np = bfq_gzip_pieces(len, chunk);
        std::vector<u64> cand(np, BFQ_GZIP_NONE);
        std::vector<bfq_gzip_rec> recs(np);
        std::vector<bfq_bgzf_tables> T(1);
        bfq_gzip_hdrtab H;
        for (u64 k = 1; k < np; k++) cand[k] = bfq_gzip_candidate(in, len, chunk, k, &H);
        for (u64 k = 0; k < np; k++) {
            recs[k] = bfq_gzip_rec{};
            recs[k].status = BFQ_GZIP_ST_NONE;
            if (k && cand[k] == BFQ_GZIP_NONE) continue;
            const bfq_gzip_job J{cand[k], 0, 0, 0, 0, 0, k == 0 ? 1u : 0u};
            bfq_gzip_run(in, len, chunk, cand.data(), np, J, nullptr, nullptr, T.data(), 0, 1, &recs[k]);
        }
        std::vector<bfq_gzip_job> jobs;
        u64 raw = 0, nEnds = 0;
        bfq_gzip_plan(recs.data(), cand.data(), np, chunk, jobs, S, &raw, &nEnds, E);
        *rawLen = raw;
        if (measure) return E->reason ? 1 : 0;
        if (!E->reason && raw > cap) return 2;
        // pass 2
        std::vector<u16> sym(raw + 1);
        std::vector<bfq_gzip_end> ends(nEnds + 1);
        for (const bfq_gzip_job &J : jobs) {
            bfq_gzip_rec r;
            bfq_gzip_run(in, len, chunk, cand.data(), np, J, sym.data() + J.outOff, ends.data() + J.endsOff, T.data(), 0, 1, &r);
        }
        // windows
        std::vector<u8> W(jobs.size() * (size_t)BFQ_GZIP_WIN, 0);
        for (size_t j = 0; j + 1 < jobs.size(); j++)
            for (u32 i = 0; i < BFQ_GZIP_WIN; i++)
                W[(j + 1) * BFQ_GZIP_WIN + i] = bfq_gzip_window_sym(sym.data() + jobs[j].outOff, jobs[j].produced, &W[j * BFQ_GZIP_WIN], i);
        // resolve: into the caller's buffer, or nowhere when the chain ended in an error
        u64 farPos = BFQ_GZIP_NONE;
        for (size_t j = 0; j < jobs.size(); j++)
            for (u64 i = 0; i < jobs[j].produced; i++) {
                bool far = false;
                const u8 v = bfq_gzip_resolve_sym(sym[jobs[j].outOff + i], &W[j * BFQ_GZIP_WIN], jobs[j].memberPre, &far);
                if (far && farPos == BFQ_GZIP_NONE) farPos = jobs[j].outOff + i;
                if (!E->reason) out[jobs[j].outOff + i] = v;
            }
        if (farPos != BFQ_GZIP_NONE) {
            E->reason = BFQ_BGZF_E_DIST_FAR;
            bfq_gzip_locate(ends.data(), nEnds, farPos, &E->member, &E->off);
        }
        if (E->reason) return 1;
        u32 tab[256];
        for (u32 i = 0; i < 256; i++) tab[i] = bfq_crc32_entry(i);
        std::vector<u32> crc(nEnds + 1, 0);
        u32 *pc = crc.data();
        for (u64 r = 0; r * BFQ_GZIP_CRC_RANGE < raw; r++)
            bfq_gzip_crc_range(tab, out, raw, r, ends.data(), nEnds, [pc](u64 m, u32 v) { pc[m] ^= v; });
        bfq_gzip_check_members(ends.data(), nEnds, crc.data(), E);
        return E->reason ? 1 : 0;
    } catch (const std::bad_alloc &) {
        return 3;
    }
}
