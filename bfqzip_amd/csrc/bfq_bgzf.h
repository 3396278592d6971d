// bfq_bgzf.h -- the BGZF subset of gzip, host and device: the member header walk (RFC 1952 + the BGZF section of the SAM
// specification), the inflate of one member (RFC 1951) and its CRC32.  Plain C++, shared by the kernel (k_bgzf.hip), the
// host side (bfq_bgzf.hip) and the sanitizer program (tests/cxx/test_bgzf.cpp): everything that decides a bound is here.
//
// A BGZF file is a chain of independent gzip members of at most 64 KiB in and out.  Every member states its own size in its
// header ('B','C' subfield: total - 1) and its CRC32 and raw size in its trailer, so the directory (in_off, out_off) of a
// whole file is known before a byte is decoded, and every member can be inflated on its own.
//
// The inflate is written for `nl` cooperating lanes of which this is lane `lane` (the host: lane 0 of 1; the kernel: one
// wave64 per member).  Control flow is the same in every lane: all of them read the same bits and decode the same symbols,
// lane 0 alone writes tables and literals, and all lanes share the copies (stored runs, matches, the CRC sub-ranges).
// BFQ_BGZF_SYNC() stands wherever a lane reads what another lane wrote (tables in LDS, earlier output bytes).
#pragma once
#include "bfq_common.h"
#include "../../include/bfqzip_hip.h"      // bfq_bgzf_member: the directory entry

#define BFQ_BGZF_MAX_RAW 65536u                   // ISIZE of a member
#define BFQ_BGZF_EOF_LEN 28u                      // the empty member htslib ends a file with

// why a member is refused (0: it is fine).  One code per rule; bfq_bgzf_reason() words them.
enum {
    BFQ_BGZF_OK = 0,
    BFQ_BGZF_E_SHORT,        // the input ends inside the member's header
    BFQ_BGZF_E_NOT_GZIP,     // not 1f 8b 08
    BFQ_BGZF_E_FLG,          // FLG != 4 (gzip, but no extra field: not BGZF)
    BFQ_BGZF_E_SUBFIELD,     // a subfield runs past XLEN
    BFQ_BGZF_E_NO_BC,        // no 'B','C' subfield of length 2 (gzip, but not BGZF)
    BFQ_BGZF_E_TOTAL,        // the stated member size is below XLEN + 20 or runs past the end of the input
    BFQ_BGZF_E_ISIZE,        // ISIZE > 65536
    BFQ_BGZF_E_PAYLOAD_END,  // the deflate data needs bits past the payload
    BFQ_BGZF_E_OUT_OVER,     // output past ISIZE
    BFQ_BGZF_E_DIST_FAR,     // a match distance reaches before the member's first byte
    BFQ_BGZF_E_OVERSUB,      // an over-subscribed set of code lengths
    BFQ_BGZF_E_INCOMPLETE,   // an incomplete set of code lengths (other than the single one-bit distance code)
    BFQ_BGZF_E_LITSYM,       // literal/length symbol 286 or 287
    BFQ_BGZF_E_DISTSYM,      // distance symbol 30 or 31
    BFQ_BGZF_E_NO_EOB,       // no code for the end-of-block symbol
    BFQ_BGZF_E_REP_FIRST,    // repeat code 16 with no length before it
    BFQ_BGZF_E_REP_OVER,     // a repeat runs past HLIT + HDIST
    BFQ_BGZF_E_HLIT_HDIST,   // HLIT > 286 or HDIST > 30
    BFQ_BGZF_E_STORED_LEN,   // stored block: LEN != ~NLEN
    BFQ_BGZF_E_STORED_RUN,   // stored block: the run goes past the payload
    BFQ_BGZF_E_BTYPE,        // block type 3
    BFQ_BGZF_E_BADCODE,      // bits that are no code of the block's (incomplete or empty) set
    BFQ_BGZF_E_LENGTH,       // the final block ends with a length other than ISIZE
    BFQ_BGZF_E_CRC,          // CRC32 of the output differs from the trailer
    BFQ_BGZF_E_TRAILING,     // payload bytes left over after the final block
    BFQ_BGZF_E_NUM
};

BFQ_HD const char *bfq_bgzf_reason(int r)
{
    switch (r) {
    case BFQ_BGZF_OK: return "ok";
    case BFQ_BGZF_E_SHORT: return "the input ends inside the member header";
    case BFQ_BGZF_E_NOT_GZIP: return "no gzip member here (1f 8b 08 expected)";
    case BFQ_BGZF_E_FLG: return "gzip flags are not 4 (extra field only): not a BGZF member";
    case BFQ_BGZF_E_SUBFIELD: return "an extra subfield runs past XLEN";
    case BFQ_BGZF_E_NO_BC: return "no BC subfield: not a BGZF member";
    case BFQ_BGZF_E_TOTAL: return "the member size in the BC subfield is too small or runs past the end of the input";
    case BFQ_BGZF_E_ISIZE: return "ISIZE above 65536";
    case BFQ_BGZF_E_PAYLOAD_END: return "the deflate data runs past the payload";
    case BFQ_BGZF_E_OUT_OVER: return "the deflate data produces more than ISIZE bytes";
    case BFQ_BGZF_E_DIST_FAR: return "a match distance reaches before the start of the member";
    case BFQ_BGZF_E_OVERSUB: return "over-subscribed code lengths";
    case BFQ_BGZF_E_INCOMPLETE: return "incomplete code lengths";
    case BFQ_BGZF_E_LITSYM: return "literal/length symbol 286 or 287";
    case BFQ_BGZF_E_DISTSYM: return "distance symbol 30 or 31";
    case BFQ_BGZF_E_NO_EOB: return "no end-of-block code";
    case BFQ_BGZF_E_REP_FIRST: return "repeat code with no length before it";
    case BFQ_BGZF_E_REP_OVER: return "a repeat runs past HLIT + HDIST";
    case BFQ_BGZF_E_HLIT_HDIST: return "HLIT above 286 or HDIST above 30";
    case BFQ_BGZF_E_STORED_LEN: return "stored block: LEN is not the complement of NLEN";
    case BFQ_BGZF_E_STORED_RUN: return "stored block: the run goes past the payload";
    case BFQ_BGZF_E_BTYPE: return "block type 3";
    case BFQ_BGZF_E_BADCODE: return "bits that are no code of the block's code set";
    case BFQ_BGZF_E_LENGTH: return "the inflated length differs from ISIZE";
    case BFQ_BGZF_E_CRC: return "CRC32 mismatch";
    case BFQ_BGZF_E_TRAILING: return "payload bytes left over after the final block";
    }
    return "unknown reason";
}

// ---------------------------------------------------------------- CRC32 (gzip polynomial, reflected)
// Serial form: the usual byte table.  Parallel form: a lane takes the CRC of its own sub-range (a CRC of its own, from 0),
// and multiplies it by x^(8 * bytes that follow it) mod P; the CRC of the whole is the XOR of the lanes' values.
#define BFQ_CRC32_POLY 0xEDB88320u
BFQ_HD u32 bfq_crc32_entry(u32 i)
{
    u32 c = i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? BFQ_CRC32_POLY ^ (c >> 1) : c >> 1;
    return c;
}
BFQ_HD u32 bfq_crc32_serial(const u32 *tab, const u8 *p, u64 n)
{
    u32 c = 0xFFFFFFFFu;
    for (u64 i = 0; i < n; i++) c = tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return ~c;
}
BFQ_HD u32 bfq_crc32_mulmod(u32 a, u32 b)           // a(x) * b(x) mod P, bit 31 = x^0
{
    u32 p = 0;
    for (int k = 0; k < 32; k++) {
        if (a & (0x80000000u >> k)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ BFQ_CRC32_POLY : b >> 1;
    }
    return p;
}
BFQ_HD u32 bfq_crc32_xpow8(u64 n)                   // x^(8 n) mod P
{
    u32 r = 0x80000000u, b = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) r = bfq_crc32_mulmod(b, r);
        b = bfq_crc32_mulmod(b, b);
    }
    return r;
}
BFQ_HD u32 bfq_crc32_shift(u32 crc, u64 after) { return bfq_crc32_mulmod(bfq_crc32_xpow8(after), crc); }
// lane's share of the CRC of p[0, n): XOR over all lanes = bfq_crc32_serial(tab, p, n)
BFQ_HD u32 bfq_crc32_part(const u32 *tab, const u8 *p, u32 n, u32 lane, u32 nl)
{
    const u32 chunk = (n + nl - 1) / nl;
    const u32 lo = lane * chunk < n ? lane * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    if (hi == lo) return 0;
    return bfq_crc32_shift(bfq_crc32_serial(tab, p + lo, hi - lo), n - hi);
}

// ---------------------------------------------------------------- member header
struct bfq_bgzf_hdr { u32 total, payOff, payLen, crc, isize; };
BFQ_HD u32 bfq_bgzf_le16(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8); }
BFQ_HD u32 bfq_bgzf_le32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
// the member that starts at p, of which `avail` bytes exist
BFQ_HD int bfq_bgzf_member_header(const u8 *p, u64 avail, bfq_bgzf_hdr *h)
{
    if (avail < 2) return BFQ_BGZF_E_SHORT;
    if (p[0] != 0x1F || p[1] != 0x8B) return BFQ_BGZF_E_NOT_GZIP;
    if (avail < 12) return BFQ_BGZF_E_SHORT;
    if (p[2] != 8) return BFQ_BGZF_E_NOT_GZIP;
    if (p[3] != 4) return BFQ_BGZF_E_FLG;
    const u32 xlen = bfq_bgzf_le16(p + 10), end = 12 + xlen;
    if (end > avail) return BFQ_BGZF_E_SHORT;
    u32 q = 12, bsize = 0;
    bool have = false;
    while (q < end) {
        if (q + 4 > end) return BFQ_BGZF_E_SUBFIELD;
        const u32 slen = bfq_bgzf_le16(p + q + 2);
        if (q + 4 + slen > end) return BFQ_BGZF_E_SUBFIELD;
        if (!have && p[q] == (u8)'B' && p[q + 1] == (u8)'C' && slen == 2) { bsize = bfq_bgzf_le16(p + q + 4); have = true; }
        q += 4 + slen;
    }
    if (!have) return BFQ_BGZF_E_NO_BC;
    const u32 total = bsize + 1;
    if (total < xlen + 20 || total > avail) return BFQ_BGZF_E_TOTAL;
    h->total = total;
    h->payOff = end;
    h->payLen = total - xlen - 20;
    h->crc = bfq_bgzf_le32(p + total - 8);
    h->isize = bfq_bgzf_le32(p + total - 4);
    if (h->isize > BFQ_BGZF_MAX_RAW) return BFQ_BGZF_E_ISIZE;
    return BFQ_BGZF_OK;
}

// ---------------------------------------------------------------- inflate of one member
// Tables of one member being decoded (the kernel: one per wave, in LDS; 3.9 KiB).  A code set is kept twice: count[] / sym[]
// in canonical order, which decode any code one bit at a time, and fast[], indexed by the next LBITS / DBITS input bits,
// which answers the codes that short at once: symbol << 4 | length, 0 = take the slow way.
#define BFQ_BGZF_LBITS 10
#define BFQ_BGZF_DBITS 8
struct bfq_bgzf_tables {
    u16 lfast[1u << BFQ_BGZF_LBITS], dfast[1u << BFQ_BGZF_DBITS];
    u16 lsym[288], dsym[32];
    u16 lcount[16], dcount[16], offs[16];
    u8 lens[320];                                   // code lengths of the block header: HLIT literal/length ones, then HDIST distance ones
    u8 cl[20];                                      // lengths of the code-length code
    u32 crc[64];                                    // the lanes' CRC shares
    int st;                                         // what lane 0 found while it built a table
};

struct bfq_bgzf_bits { const u8 *p; u32 n, pos; u64 buf; u32 cnt; };   // cnt valid bits in buf, everything above them zero
// at least 33 bits afterwards unless the payload ends first; never reads p[n] or beyond
BFQ_HD void bfq_bgzf_refill(bfq_bgzf_bits &b)
{
    if (b.cnt > 32) return;
    if (b.pos + 4 <= b.n) {
        const u8 *q = b.p + b.pos;
        b.buf |= (u64)bfq_bgzf_le32(q) << b.cnt;
        b.cnt += 32; b.pos += 4;
        return;
    }
    while (b.cnt <= 56 && b.pos < b.n) { b.buf |= (u64)b.p[b.pos++] << b.cnt; b.cnt += 8; }
}
BFQ_HD u32 bfq_bgzf_take(bfq_bgzf_bits &b, u32 k)    // k <= b.cnt, k < 32
{
    const u32 v = (u32)b.buf & ((1u << k) - 1u);
    b.buf >>= k; b.cnt -= k;
    return v;
}
// the next symbol; -1: the bits are no code of this set, -2: the payload ends inside the code
BFQ_HD int bfq_bgzf_decode(bfq_bgzf_bits &b, const u16 *fast, u32 fastBits, const u16 *count, const u16 *sym)
{
    const u32 e = fast[(u32)b.buf & ((1u << fastBits) - 1u)];
    if (e) {
        if ((e & 15u) > b.cnt) return -2;
        b.buf >>= (e & 15u); b.cnt -= (e & 15u);
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (u32 len = 1; len <= 15; len++) {
        if (len > b.cnt) return -2;
        code |= (int)((b.buf >> (len - 1)) & 1u);
        const int cnt = count[len];
        if (code - cnt < first) {
            b.buf >>= len; b.cnt -= len;
            return sym[index + (code - first)];
        }
        index += cnt; first += cnt;
        first <<= 1; code <<= 1;
    }
    return -1;
}
// one code set from n code lengths (one lane).  0: complete, 1: incomplete, 2: no code at all, -1: over-subscribed
BFQ_HD int bfq_bgzf_build(const u8 *lens, u32 n, u16 *count, u16 *sym, u16 *offs, u16 *fast, u32 fastBits)
{
    for (u32 l = 0; l < 16; l++) count[l] = 0;
    for (u32 i = 0; i < n; i++) count[lens[i]]++;
    for (u32 i = 0; i < (1u << fastBits); i++) fast[i] = 0;
    if (count[0] == n) return 2;
    int left = 1;
    for (u32 l = 1; l <= 15; l++) {
        left <<= 1;
        left -= (int)count[l];
        if (left < 0) return -1;
    }
    offs[1] = 0;
    for (u32 l = 1; l < 15; l++) offs[l + 1] = (u16)(offs[l] + count[l]);
    for (u32 i = 0; i < n; i++)
        if (lens[i]) sym[offs[lens[i]]++] = (u16)i;
    u32 code = 0, idx = 0;
    for (u32 l = 1; l <= fastBits; l++) {
        for (u32 k = 0; k < count[l]; k++, code++, idx++) {
            u32 rev = 0;
            for (u32 j = 0; j < l; j++) rev |= ((code >> j) & 1u) << (l - 1 - j);
            for (u32 j = rev; j < (1u << fastBits); j += 1u << l) fast[j] = (u16)((u32)sym[idx] << 4 | l);
        }
        code <<= 1;
    }
    return left > 0 ? 1 : 0;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define BFQ_BGZF_SYNC() do { __threadfence_block(); __builtin_amdgcn_wave_barrier(); } while (0)
#else
#define BFQ_BGZF_SYNC() do { } while (0)
#endif

// The deflate payload pay[0, plen) into out[0, isize); crcWant and isize are the member's trailer.  Reads nothing outside
// the payload and writes nothing outside out[0, isize), whatever the payload holds.  Returns a BFQ_BGZF_* code, the same in
// every lane.
BFQ_HD int bfq_bgzf_inflate_payload(const u8 *pay, u32 plen, u8 *out, u32 isize, u32 crcWant, bfq_bgzf_tables *T, const u32 *crcTab,
                                    u32 lane, u32 nl)
{
    bfq_bgzf_bits b{pay, plen, 0, 0, 0};
    u32 op = 0, last = 0;
    bool fixedBuilt = false;
    do {
        bfq_bgzf_refill(b);
        if (b.cnt < 3) return BFQ_BGZF_E_PAYLOAD_END;
        last = bfq_bgzf_take(b, 1);
        const u32 type = bfq_bgzf_take(b, 2);
        if (type == 3) return BFQ_BGZF_E_BTYPE;
        if (type == 0) {
            bfq_bgzf_take(b, b.cnt & 7u);
            u32 src = b.pos - b.cnt / 8;                          // whole bytes are left in the buffer: hand them back
            if (plen - src < 4) return BFQ_BGZF_E_PAYLOAD_END;
            const u32 len = bfq_bgzf_le16(pay + src), nlen = bfq_bgzf_le16(pay + src + 2);
            src += 4;
            if (len != (~nlen & 0xFFFFu)) return BFQ_BGZF_E_STORED_LEN;
            if (len > plen - src) return BFQ_BGZF_E_STORED_RUN;
            if (len > isize - op) return BFQ_BGZF_E_OUT_OVER;
            for (u32 i = lane; i < len; i += nl) out[op + i] = pay[src + i];
            op += len;
            b.pos = src + len; b.buf = 0; b.cnt = 0;
            continue;
        }
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
            if (b.cnt < 14) return BFQ_BGZF_E_PAYLOAD_END;
            const u32 hlit = bfq_bgzf_take(b, 5) + 257, hdist = bfq_bgzf_take(b, 5) + 1, hclen = bfq_bgzf_take(b, 4) + 4;
            if (hlit > 286 || hdist > 30) return BFQ_BGZF_E_HLIT_HDIST;
            // the code-length code, kept where the distance set goes afterwards
            BFQ_BGZF_SYNC();
            if (lane == 0)
                for (u32 i = 0; i < 19; i++) T->cl[i] = 0;
            const char *order = "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017";
            for (u32 i = 0; i < hclen; i++) {
                bfq_bgzf_refill(b);
                if (b.cnt < 3) return BFQ_BGZF_E_PAYLOAD_END;
                const u32 v = bfq_bgzf_take(b, 3);
                if (lane == 0) T->cl[(u8)order[i]] = (u8)v;
            }
            if (lane == 0) {
                const int r = bfq_bgzf_build(T->cl, 19, T->dcount, T->dsym, T->offs, T->dfast, 7);
                T->st = r < 0 ? BFQ_BGZF_E_OVERSUB : r > 0 ? BFQ_BGZF_E_INCOMPLETE : BFQ_BGZF_OK;
            }
            BFQ_BGZF_SYNC();
            if (T->st) return T->st;
            u32 idx = 0, prev = 0;
            const u32 want = hlit + hdist;
            while (idx < want) {
                bfq_bgzf_refill(b);
                const int s = bfq_bgzf_decode(b, T->dfast, 7, T->dcount, T->dsym);
                if (s < 0) return s == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE;
                if (s < 16) {
                    if (lane == 0) T->lens[idx] = (u8)s;
                    idx++; prev = (u32)s;
                    continue;
                }
                u32 rep, val = 0;
                if (s == 16) {
                    if (idx == 0) return BFQ_BGZF_E_REP_FIRST;
                    if (b.cnt < 2) return BFQ_BGZF_E_PAYLOAD_END;
                    rep = 3 + bfq_bgzf_take(b, 2); val = prev;
                } else if (s == 17) {
                    if (b.cnt < 3) return BFQ_BGZF_E_PAYLOAD_END;
                    rep = 3 + bfq_bgzf_take(b, 3);
                } else {
                    if (b.cnt < 7) return BFQ_BGZF_E_PAYLOAD_END;
                    rep = 11 + bfq_bgzf_take(b, 7);
                }
                if (rep > want - idx) return BFQ_BGZF_E_REP_OVER;
                if (lane == 0)
                    for (u32 i = 0; i < rep; i++) T->lens[idx + i] = (u8)val;
                idx += rep; prev = val;
            }
            BFQ_BGZF_SYNC();
            if (lane == 0) {
                int st = BFQ_BGZF_OK;
                if (T->lens[256] == 0) st = BFQ_BGZF_E_NO_EOB;
                if (!st) {
                    const int r = bfq_bgzf_build(T->lens, hlit, T->lcount, T->lsym, T->offs, T->lfast, BFQ_BGZF_LBITS);
                    st = r < 0 ? BFQ_BGZF_E_OVERSUB : r > 0 ? BFQ_BGZF_E_INCOMPLETE : BFQ_BGZF_OK;
                }
                if (!st) {
                    // incomplete distance sets: the single one-bit code (zlib writes it for a block with one distance) and
                    // the set with no code at all (RFC 1951: a block of literals only) stand; a match under either meets
                    // bits that are no code
                    const int r = bfq_bgzf_build(T->lens + hlit, hdist, T->dcount, T->dsym, T->offs, T->dfast, BFQ_BGZF_DBITS);
                    if (r < 0) st = BFQ_BGZF_E_OVERSUB;
                    else if (r == 1) {
                        u32 codes = 0;
                        for (u32 l = 1; l <= 15; l++) codes += T->dcount[l];
                        if (!(codes == 1 && T->dcount[1] == 1)) st = BFQ_BGZF_E_INCOMPLETE;
                    }
                }
                T->st = st;
            }
            BFQ_BGZF_SYNC();
            if (T->st) return T->st;
        }
        // the block's symbols
        for (;;) {
            bfq_bgzf_refill(b);
            const int s = bfq_bgzf_decode(b, T->lfast, BFQ_BGZF_LBITS, T->lcount, T->lsym);
            if (s < 0) return s == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE;
            if (s < 256) {
                if (op >= isize) return BFQ_BGZF_E_OUT_OVER;
                if (lane == 0) out[op] = (u8)s;
                op++;
                continue;
            }
            if (s == 256) break;
            if (s >= 286) return BFQ_BGZF_E_LITSYM;
            u32 len;
            if (s == 285) len = 258;
            else {
                const u32 i = (u32)s - 257;
                if (i < 8) len = 3 + i;
                else {
                    const u32 ext = (i >> 2) - 1;
                    if (b.cnt < ext) return BFQ_BGZF_E_PAYLOAD_END;
                    len = 3 + ((4 + (i & 3u)) << ext) + bfq_bgzf_take(b, ext);
                }
            }
            bfq_bgzf_refill(b);
            const int ds = bfq_bgzf_decode(b, T->dfast, BFQ_BGZF_DBITS, T->dcount, T->dsym);
            if (ds < 0) return ds == -2 ? BFQ_BGZF_E_PAYLOAD_END : BFQ_BGZF_E_BADCODE;
            if (ds >= 30) return BFQ_BGZF_E_DISTSYM;
            u32 dist;
            if (ds < 4) dist = 1 + (u32)ds;
            else {
                const u32 ext = ((u32)ds >> 1) - 1;
                if (b.cnt < ext) return BFQ_BGZF_E_PAYLOAD_END;
                dist = 1 + ((2 + ((u32)ds & 1u)) << ext) + bfq_bgzf_take(b, ext);
            }
            if (dist > op) return BFQ_BGZF_E_DIST_FAR;
            if (len > isize - op) return BFQ_BGZF_E_OUT_OVER;
            BFQ_BGZF_SYNC();                                      // the bytes of earlier tokens, stored by other lanes
            const u8 *from = out + (op - dist);
            for (u32 i = lane; i < len; i += nl) out[op + i] = from[i % dist];
            op += len;
        }
    } while (!last);
    if (b.cnt / 8 + (plen - b.pos) != 0) return BFQ_BGZF_E_TRAILING;
    if (op != isize) return BFQ_BGZF_E_LENGTH;
    BFQ_BGZF_SYNC();
    T->crc[lane] = bfq_crc32_part(crcTab, out, isize, lane, nl);
    BFQ_BGZF_SYNC();
    u32 crc = 0;
    for (u32 i = 0; i < nl; i++) crc ^= T->crc[i];
    return crc == crcWant ? BFQ_BGZF_OK : BFQ_BGZF_E_CRC;
}

// ---------------------------------------------------------------- the directory of a file (host side)
// Walks the members of h[0, len): fills m[0, min(n, cap)) when m is given.  Returns BFQ_BGZF_OK, or the reason the member
// *n (at byte *badOff) is refused.  A file need not end with the EOF member.
inline int bfq_bgzf_walk(const u8 *h, u64 len, bfq_bgzf_member *m, u64 cap, u64 *n, u64 *rawLen, u64 *badOff)
{
    u64 at = 0, raw = 0, k = 0;
    while (at < len) {
        bfq_bgzf_hdr hd;
        const int r = bfq_bgzf_member_header(h + at, len - at, &hd);
        if (r) { *n = k; *rawLen = raw; *badOff = at; return r; }
        if (m && k < cap) m[k] = bfq_bgzf_member{at, raw, hd.total, hd.isize};
        at += hd.total; raw += hd.isize; k++;
    }
    *n = k; *rawLen = raw; *badOff = len;
    return BFQ_BGZF_OK;
}
