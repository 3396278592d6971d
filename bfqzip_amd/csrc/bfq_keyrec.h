// bfq_keyrec.h -- the sort record of one text position, built in one place (plain C++ like bfq_common.h: host and device).
//
// Row p of the unsorted record array is text position p: its record is a pure function of the packed text around p
// (the 16-symbol key) and of the symbol and quality before p (the payload).  k_build_keys (k_text.hip) writes these
// records to memory for the fallback route; the sort's generating first pass (k_radix.hip) makes them in registers and
// never stores them unsorted.  Both call bfq_keyrec(), so both produce the same bits.
//
// The key is what bfq_skey_of(bfq_mask_key(window)) of bfq_common.h gives, computed on the 16 symbols alone as two 24-bit
// halves: all 32-bit arithmetic, about half the instructions of the 63-bit route -- the generating pass is bound by its
// arithmetic, not by memory.  tests/cxx/test_keyrec.cpp holds both against a byte-wise restatement.
#pragma once
#include "bfq_common.h"

BFQ_HD int bfq_clz32(u32 x)          // x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __clz((int)x);
#else
    return __builtin_clz(x);
#endif
}

// The first 16 symbols of the suffix at offset o (symbols, 0..20) of packed word a, bnext being the packed word after a:
// two halves of 8 symbols (24 bits, first symbol on top) with everything from the first terminator on cleared, and the
// number of symbols before that terminator (16: none)
BFQ_HD void bfq_keyrec_halves(u64 a, u64 bnext, u32 o, u32 *hi, u32 *lo, u32 *len)
{
    const u32 o3 = o * 3u;
    const u64 W = ((a << o3) & BFQ_M63) | (bnext >> (63u - o3));      // bit 63 of a packed word is 0: nothing comes in at o = 0
    u32 H = (u32)(W >> 39), L = (u32)(W >> 15) & 0xFFFFFFu;
    const u32 F = 0x249249u;                                          // bit 0 of each of the 8 fields
    const u32 zh = ~(H | (H >> 1) | (H >> 2)) & F, zl = ~(L | (L >> 1) | (L >> 2)) & F;
    const u32 z = zh ? zh : zl;
    u32 n = BFQ_KEY_SYMS;
    if (z) {
        const u32 b = 31u - (u32)bfq_clz32(z);                        // low bit of the first zero field of its half (0, 3, .., 21)
        const u32 keep = 0u - (8u << b);                              // the fields above it
        n = 7u - ((b * 11u) >> 5);                                    // 7 - b / 3
        if (zh) { H &= keep; L = 0; }
        else { L &= keep; n += 8u; }
    }
    *hi = H; *lo = L; *len = n;
}

// 8 symbols (24 bits) -> 4 groups of 5 bits: two symbols (c0, c1) -> 0 for a terminator first, else 6 c0 + c1 - 5 (bfq_common.h)
BFQ_HD u32 bfq_keyrec_groups(u32 x)
{
    const u32 M7 = 0x1C71C7u;
    const u32 A = (x >> 3) & M7, B = x & M7;                          // c0 / c1 of the 4 pairs, one pair per 6-bit lane
    const u32 nz = (A | (A >> 1) | (A >> 2)) & 0x041041u;
    const u32 S = A * 6u + B - nz * 5u;                               // <= 30: stays inside the lane
    const u32 v = (S & 0x03F03Fu) | ((S & 0xFC0FC0u) >> 1);           // 4 x 6 -> 2 x 10 -> 20 bits
    return (v & 0xFFFu) | ((v & 0xFFF000u) >> 2);
}

// the sort key (key40 | L << 40) of that suffix
BFQ_HD u64 bfq_keyrec_skey(u64 a, u64 bnext, u32 o)
{
    u32 hi, lo, len;
    bfq_keyrec_halves(a, bnext, o, &hi, &lo, &len);
    return ((u64)bfq_keyrec_groups(hi) << 20) | (u64)bfq_keyrec_groups(lo) | ((u64)len << 40);
}

// the payload of text position pos: prevCode / prevQual are the symbol code and the quality at pos - 1 (ignored at
// pos == 0, which has no predecessor: it counts as following a terminator); after a terminator the quality is '#'
BFQ_HD u64 bfq_keyrec_pay(u64 pos, u32 prevCode, u32 prevQual)
{
    const u32 pc = pos ? (prevCode & 0xFFu) : 0u;
    const u32 pq = pc ? (prevQual & 0xFFu) : (u32)'#';
    return bfq_pack_val(pos, pc, pq);
}

// the record of text position pos = 21 * (index of a) + o: w0 and the (w1, w2) pair as the sort's two arrays hold them
BFQ_HD void bfq_keyrec(u64 a, u64 bnext, u32 o, u64 pos, u32 prevCode, u32 prevQual, u32 *w0, u64 *w12)
{
    u32 hi, lo, len;
    bfq_keyrec_halves(a, bnext, o, &hi, &lo, &len);
    const u32 kh = bfq_keyrec_groups(hi), kl = bfq_keyrec_groups(lo);  // key40 = kh << 20 | kl
    const u64 pay = bfq_keyrec_pay(pos, prevCode, prevQual);
    *w0 = (kh << 12) | (kl >> 8);                                     // = bfq_rec_w0(skey)
    const u32 w1 = (kl << 24) | (len << 16) | (u32)(pay >> 32);       // = bfq_rec_w1(skey, pay)
    *w12 = ((u64)bfq_rec_w2(pay) << 32) | w1;
}

// digit 0 of the LSD sort (the low byte of the key) as the record carries it in bits 24..31 of w1: the last four symbols decide it
BFQ_HD u32 bfq_keyrec_digit0(u64 a, u64 bnext, u32 o)
{
    u32 hi, lo, len;
    bfq_keyrec_halves(a, bnext, o, &hi, &lo, &len);
    return bfq_keyrec_groups(lo & 0xFFFu) & 255u;
}

// the same from the arrays: T8 / Q8 the byte text and its qualities, text3 the packed text in its sector layout
BFQ_HD void bfq_keyrec_at(const u8 *T8, const u8 *Q8, const u64 *text3, u64 pos, u32 *w0, u64 *w12)
{
    const u64 w = pos / BFQ_SYMS_PER_WORD;
    const u32 o = (u32)(pos - w * BFQ_SYMS_PER_WORD);
    const u64 *t = text3 + bfq_t3_at(w);
    bfq_keyrec(t[0], t[1], o, pos, pos ? T8[pos - 1] : 0u, pos ? Q8[pos - 1] : 0u, w0, w12);
}

// small exact divisions for index arithmetic relative to a tile's first position (no 64-bit division per row)
BFQ_HD u32 bfq_div21_small(u32 q) { return (q * 3121u) >> 16; }      // q / 21 for q < 4096
BFQ_HD u32 bfq_div6_small(u32 e) { return (e * 171u) >> 10; }        // e / 6 for e < 256
