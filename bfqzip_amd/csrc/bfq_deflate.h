// bfq_deflate.h -- the BGZF writer, host and device: a text cut into members of 65 280 bytes (htslib's size), each member a
// raw deflate payload (RFC 1951) between the 18-byte BGZF header and CRC32 + ISIZE.  Plain C++, shared by the kernel
// (k_deflate.hip), the host side (bfq_deflate.hip) and the sanitizer program (tests/cxx/test_deflate.cpp).  The host form
// (one lane) is the statement of the format: the kernel gives the same bytes, whatever the batch and the grid.
//
// A member is written for `nl` cooperating lanes (nl <= 64) of which this is lane `lane` (the host: lane 0 of 1; the kernel:
// one wave64 per member).  Control flow is the same in every lane; BFQ_DEFL_SYNC() stands wherever a lane reads what another
// lane wrote.  What the bytes depend on is defined without the lanes:
//   parse    the literal histogram of the member gives every byte a cost (the lengths of a Huffman code over it).  The text is
//            matched in steps of BFQ_DEFL_STEP positions: a position's candidates are the one position that earlier steps left
//            in its hash slot (the highest with that hash of BFQ_DEFL_HBYTES bytes: a max, so the order of insertion is
//            nothing) and the position before it (distance 1: runs of one byte).  The longer of the two is kept when it is
//            at least 3 long, at most 32 768 back and estimated to cost fewer bits than its literals.  Selection is greedy
//            from the member's first byte, step by step (one lane; the search skips what the cursor already covers).
//   coding   one dynamic block: literal/length and distance codes limited to 15 bits, the code-length code to 7, the header
//            run-length coded (16 / 17 / 18).  Every lane codes an equal share of the tokens at a bit offset that a sum over
//            the lanes' bit counts gives; bits are ORed into the zeroed slot, word by word.
//   stored   a member whose coded form would be no shorter than the stored form (piece + 31 bytes) is one stored block.
// Bounds: every loop runs to the member's length (or a constant); a match compare ends at the member's last byte; the coded
// size is known before a bit is written and every word is checked against the slot besides (overflow: stored form).
#pragma once
#include <stdlib.h>
#include <string.h>
#include "bfq_bgzf.h"

#define BFQ_DEFL_PIECE 65280u                     // text bytes per member
#define BFQ_DEFL_OVER 31u                         // a member is at most its piece + this (the stored form)
#define BFQ_DEFL_SLOT 65312u                      // piece + 31, rounded up to whole words: a member's slot
#define BFQ_DEFL_STEP 64u                         // positions per matching step
#define BFQ_DEFL_HBITS 12                         // hash slots (log2)
#define BFQ_DEFL_HBYTES 4u                        // bytes hashed at a position
#define BFQ_DEFL_MAX_LANES 64u
#define BFQ_DEFL_MATCH 0x80000000u                // token: a match, (length - 3) | (distance - 1) << 8; else the literal byte
#define BFQ_DEFL_LSYM_BITS 9u                     // what a match is estimated to cost: its length symbol ...
#define BFQ_DEFL_DSYM_BITS 6u                     // ... and its distance symbol, beside their extra bits

BFQ_HD u64 bfq_defl_members(u64 len) { return (len + BFQ_DEFL_PIECE - 1) / BFQ_DEFL_PIECE; }
BFQ_HD u64 bfq_defl_bound(u64 len) { return len + BFQ_DEFL_OVER * bfq_defl_members(len) + BFQ_BGZF_EOF_LEN; }
BFQ_HD u8 bfq_defl_eof_byte(u32 i)                // htslib's empty member
{
    return (u8)(i == 0 ? 0x1F : i == 1 ? 0x8B : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xFF : i == 10 ? 6 : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2 : i == 16 ? 0x1B : i == 18 ? 3 : 0);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define BFQ_DEFL_SYNC() do { __threadfence_block(); __builtin_amdgcn_wave_barrier(); } while (0)
#define BFQ_DEFL_ADD(p) atomicAdd((p), 1u)
#define BFQ_DEFL_MAX(p, v) atomicMax((p), (v))
#define BFQ_DEFL_OR(p, v) atomicOr((p), (v))
#else
#define BFQ_DEFL_SYNC() do { } while (0)
#define BFQ_DEFL_ADD(p) (void)(*(p) += 1u)
#define BFQ_DEFL_MAX(p, v) (void)(*(p) = *(p) < (v) ? (v) : *(p))
#define BFQ_DEFL_OR(p, v) (void)(*(p) |= (v))
#endif

// what one member being written needs beside its tokens (the kernel: one per wave, in LDS; 24 KiB)
struct bfq_defl_work {
    u32 table[1u << BFQ_DEFL_HBITS];                // hash slot -> highest position + 1 of the steps before (0: none)
    u32 freq[320];                                  // literal/length symbols at 0, distance symbols at 288
    u32 stepTok[BFQ_DEFL_STEP];                     // the step's positions: the token that would start there
    u32 laneBits[BFQ_DEFL_MAX_LANES], crc[BFQ_DEFL_MAX_LANES];
    u32 clFreq[19];
    u32 hw[288];                                    // code construction: weights of the inner nodes
    u16 hsym[288], hpar[576];                       // ... the used symbols by weight, every node's parent
    u16 lcode[288], dcode[32], clCode[19];          // codes, bit-reversed (deflate packs them from the top bit)
    u16 seq[320];                                   // the block header's code-length symbols: symbol | extra bits << 8
    u8 lens[320];                                   // code lengths: literal/length at 0, distance at 288
    u8 litCost[256], clLen[19], hdep[288];
    u32 cur, ntok, nseq, hlit, hdist, hclen, hdrBits, over;
};

BFQ_HD u32 bfq_defl_log2(u32 x) { return 31u - (u32)__builtin_clz(x); }      // x > 0
BFQ_HD u32 bfq_defl_lsym(u32 len)                   // length 3..258 -> symbol 257..285
{
    const u32 l = len - 3;
    if (l < 8) return 257 + l;
    if (len == 258) return 285;
    const u32 ext = bfq_defl_log2(l) - 2;
    return 257 + 4 * (ext + 1) + ((l >> ext) & 3u);
}
BFQ_HD u32 bfq_defl_lext(u32 len) { const u32 l = len - 3; return l < 8 || len == 258 ? 0 : bfq_defl_log2(l) - 2; }
BFQ_HD u32 bfq_defl_dsym(u32 dist)                  // distance 1..32768 -> symbol 0..29
{
    const u32 d = dist - 1;
    if (d < 4) return d;
    const u32 nb = bfq_defl_log2(d);
    return 2 * nb + ((d >> (nb - 1)) & 1u);
}
BFQ_HD u32 bfq_defl_dext(u32 dist) { const u32 d = dist - 1; return d < 4 ? 0 : bfq_defl_log2(d) - 1; }

// ---------------------------------------------------------------- code lengths (one lane)
// lens[0, n) for freq[0, n): no length above `limit`; with two or more used symbols the Kraft sum is exactly 1; one used symbol
// gets one bit (zlib's convention for a lone distance code).  The lengths of a Huffman tree (two queues over the sorted
// weights) are clamped to the limit; every unit the Kraft sum then has too much (in 2^-limit) is taken back the way zlib
// does it: a leaf of the deepest level above the limit becomes an inner node over itself and a leaf taken from the limit
// level.  The lengths go to the symbols by weight, the longest to the lightest (ties: the lower symbol is the lighter one).
BFQ_HD void bfq_defl_lengths(const u32 *freq, u32 n, u32 limit, u8 *lens, bfq_defl_work *W)
{
    u32 m = 0;
    for (u32 i = 0; i < n; i++) {
        lens[i] = 0;
        if (!freq[i]) continue;
        u32 j = m++;
        while (j > 0 && freq[W->hsym[j - 1]] > freq[i]) { W->hsym[j] = W->hsym[j - 1]; j--; }
        W->hsym[j] = (u16)i;
    }
    if (m == 0) return;
    if (m == 1) { lens[W->hsym[0]] = 1; return; }
    u32 a = 0, b = 0, made = 0;
    while (made < m - 1) {
        u32 w = 0;
        for (u32 t = 0; t < 2; t++) {
            const bool leaf = a < m && (b >= made || freq[W->hsym[a]] <= W->hw[b]);
            if (leaf) { w += freq[W->hsym[a]]; W->hpar[a++] = (u16)(m + made); }
            else { w += W->hw[b]; W->hpar[m + b] = (u16)(m + made); b++; }
        }
        W->hw[made++] = w;
    }
    u32 cnt[17];
    for (u32 l = 0; l <= 16; l++) cnt[l] = 0;
    W->hdep[m - 2] = 0;
    for (u32 k = m - 2; k-- > 0;) { const u32 d = W->hdep[W->hpar[m + k] - m]; W->hdep[k] = (u8)(d < 255 ? d + 1 : 255); }
    for (u32 k = 0; k < m; k++) { const u32 d = (u32)W->hdep[W->hpar[k] - m] + 1; cnt[d < limit ? d : limit]++; }
    u32 kraft = 0;
    for (u32 l = 1; l <= limit; l++) kraft += cnt[l] << (limit - l);
    for (u32 e = kraft - (1u << limit); e > 0; e--) {
        u32 bits = limit - 1;
        while (bits > 0 && cnt[bits] == 0) bits--;
        if (!bits) break;                                          // (cannot be: a sum above 1 has a code shorter than the limit)
        cnt[bits]--; cnt[bits + 1] += 2; cnt[limit]--;
    }
    u32 k = 0;
    for (u32 l = limit; l >= 1; l--)
        for (u32 q = 0; q < cnt[l] && k < m; q++) lens[W->hsym[k++]] = (u8)l;
}
// canonical codes of lens[0, n), bit-reversed
BFQ_HD void bfq_defl_codes(const u8 *lens, u32 n, u16 *codes)
{
    u32 cnt[16], next[16];
    for (u32 l = 0; l < 16; l++) cnt[l] = 0;
    for (u32 i = 0; i < n; i++) cnt[lens[i]]++;
    cnt[0] = 0;
    u32 code = 0;
    for (u32 l = 1; l < 16; l++) { code = (code + cnt[l - 1]) << 1; next[l] = code; }
    for (u32 i = 0; i < n; i++) {
        const u32 l = lens[i];
        u32 rev = 0;
        if (l) { const u32 c = next[l]++; for (u32 j = 0; j < l; j++) rev |= ((c >> j) & 1u) << (l - 1 - j); }
        codes[i] = (u16)rev;
    }
}

// ---------------------------------------------------------------- bits into a zeroed slot
struct bfq_defl_bw { u32 *w; u32 capWords, wi, cnt, over; u64 acc; };
BFQ_HD bfq_defl_bw bfq_defl_bw_at(u32 *w, u32 capWords, u32 bit) { return bfq_defl_bw{w, capWords, bit >> 5, bit & 31u, 0, 0}; }
BFQ_HD void bfq_defl_word(bfq_defl_bw &b)
{
    if (b.wi < b.capWords) BFQ_DEFL_OR(&b.w[b.wi], (u32)b.acc);
    else b.over = 1;
}
BFQ_HD void bfq_defl_put(bfq_defl_bw &b, u32 v, u32 k)           // k <= 32 bits of v, nothing above them
{
    b.acc |= (u64)v << b.cnt;
    b.cnt += k;
    if (b.cnt >= 32) { bfq_defl_word(b); b.wi++; b.acc >>= 32; b.cnt -= 32; }
}
BFQ_HD void bfq_defl_flush(bfq_defl_bw &b) { if (b.cnt && (u32)b.acc) bfq_defl_word(b); }

// ---------------------------------------------------------------- the parse
BFQ_HD u32 bfq_defl_hash(const u8 *p)
{
    u32 v = 0;
    for (u32 i = 0; i < BFQ_DEFL_HBYTES; i++) v |= (u32)p[i] << (8 * i);
    return (v * 0x9E3779B1u) >> (32 - BFQ_DEFL_HBITS);
}
// common prefix of t[c..] and t[p..], c < p, at most maxl <= n - p: no byte at or behind t[n] is read
BFQ_HD u32 bfq_defl_mlen(const u8 *t, u32 c, u32 p, u32 maxl)
{
    u32 i = 0;
    while (i + 8 <= maxl) {
        u64 x, y;
        __builtin_memcpy(&x, t + c + i, 8);
        __builtin_memcpy(&y, t + p + i, 8);
        if (x != y) return i + ((u32)__builtin_ctzll(x ^ y) >> 3);
        i += 8;
    }
    while (i < maxl && t[c + i] == t[p + i]) i++;
    return i;
}
// the token that would start at p: the literal, or a match that pays
BFQ_HD u32 bfq_defl_search(const u8 *t, u32 n, u32 p, const bfq_defl_work *W)
{
    const u32 lit = t[p], maxl = n - p < 258 ? n - p : 258;
    if (maxl < 3) return lit;
    u32 best = 0, dist = 0;
    if (p >= 1 && t[p - 1] == lit) { best = bfq_defl_mlen(t, p - 1, p, maxl); dist = 1; }
    if (p + BFQ_DEFL_HBYTES <= n) {
        const u32 c1 = W->table[bfq_defl_hash(t + p)];
        if (c1 && p - (c1 - 1) <= 32768u) {
            const u32 l = bfq_defl_mlen(t, c1 - 1, p, maxl);
            if (l > best) { best = l; dist = p - (c1 - 1); }
        }
    }
    if (best < 3) return lit;
    const u32 cost = BFQ_DEFL_LSYM_BITS + bfq_defl_lext(best) + BFQ_DEFL_DSYM_BITS + bfq_defl_dext(dist);
    u32 lits = 0;
    for (u32 i = 0; i < best && lits <= cost; i++) lits += W->litCost[t[p + i]];
    if (lits <= cost) return lit;
    return BFQ_DEFL_MATCH | (best - 3) | ((dist - 1) << 8);
}
// tok[0, W->ntok): the member's tokens; W->freq: how often every symbol is used
BFQ_HD void bfq_defl_parse(const u8 *t, u32 n, u32 *tok, bfq_defl_work *W, u32 lane, u32 nl)
{
    BFQ_DEFL_SYNC();
    for (u32 i = lane; i < (1u << BFQ_DEFL_HBITS); i += nl) W->table[i] = 0;
    for (u32 i = lane; i < 320; i += nl) W->freq[i] = 0;
    BFQ_DEFL_SYNC();
    for (u32 i = lane; i < n; i += nl) BFQ_DEFL_ADD(&W->freq[t[i]]);
    BFQ_DEFL_SYNC();
    if (lane == 0) {
        bfq_defl_lengths(W->freq, 256, 15, W->lens, W);
        for (u32 i = 0; i < 256; i++) { W->litCost[i] = W->lens[i]; W->freq[i] = 0; }
        W->cur = 0; W->ntok = 0;
    }
    BFQ_DEFL_SYNC();
    for (u32 base = 0; base < n; base += BFQ_DEFL_STEP) {
        const u32 cur = W->cur;
        for (u32 q = lane; q < BFQ_DEFL_STEP; q += nl) {
            const u32 p = base + q;
            if (p < n) W->stepTok[q] = p >= cur ? bfq_defl_search(t, n, p, W) : (u32)t[p];
        }
        BFQ_DEFL_SYNC();
        for (u32 q = lane; q < BFQ_DEFL_STEP; q += nl) {
            const u32 p = base + q;
            if (p + BFQ_DEFL_HBYTES <= n) BFQ_DEFL_MAX(&W->table[bfq_defl_hash(t + p)], p + 1);
        }
        if (lane == 0) {
            const u32 end = base + BFQ_DEFL_STEP < n ? base + BFQ_DEFL_STEP : n;
            u32 at = cur, nt = W->ntok;
            while (at < end) {
                const u32 tk = W->stepTok[at - base];
                tok[nt++] = tk;
                if (tk & BFQ_DEFL_MATCH) {
                    const u32 len = (tk & 255u) + 3, dist = ((tk >> 8) & 0x7FFFu) + 1;
                    W->freq[bfq_defl_lsym(len)]++;
                    W->freq[288 + bfq_defl_dsym(dist)]++;
                    at += len;
                } else { W->freq[tk]++; at++; }
            }
            W->cur = at; W->ntok = nt;
        }
        BFQ_DEFL_SYNC();
    }
}

// ---------------------------------------------------------------- the block header (one lane)
BFQ_HD void bfq_defl_seq(bfq_defl_work *W, u32 sym, u32 extra) { W->seq[W->nseq++] = (u16)(sym | extra << 8); W->clFreq[sym]++; }
BFQ_HD const char *bfq_defl_order() { return "\020\021\022\000\010\007\011\006\012\005\013\004\014\003\015\002\016\001\017"; }
BFQ_HD void bfq_defl_header_plan(bfq_defl_work *W)
{
    W->freq[256] = 1;
    bfq_defl_lengths(W->freq, 286, 15, W->lens, W);
    u32 dused = 0;
    for (u32 i = 0; i < 30; i++) dused += W->freq[288 + i] ? 1 : 0;
    if (!dused) W->freq[288] = 1;                                // no match: one distance code of one bit, never used
    bfq_defl_lengths(W->freq + 288, 30, 15, W->lens + 288, W);
    u32 hlit = 286, hdist = 30;
    while (hlit > 257 && !W->lens[hlit - 1]) hlit--;
    while (hdist > 1 && !W->lens[288 + hdist - 1]) hdist--;
    W->hlit = hlit; W->hdist = hdist;
    bfq_defl_codes(W->lens, 286, W->lcode);
    bfq_defl_codes(W->lens + 288, 30, W->dcode);
    // the lengths of both codes as one sequence, run-length coded
    for (u32 i = 0; i < 19; i++) W->clFreq[i] = 0;
    W->nseq = 0;
    const u32 want = hlit + hdist;
    for (u32 i = 0; i < want;) {
        const u32 v = W->lens[i < hlit ? i : 288 + i - hlit];
        u32 run = 1;
        while (i + run < want && W->lens[i + run < hlit ? i + run : 288 + i + run - hlit] == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11) { const u32 r = run < 138 ? run : 138; bfq_defl_seq(W, 18, r - 11); run -= r; }
            if (run >= 3) { bfq_defl_seq(W, 17, run - 3); run = 0; }
        } else {
            bfq_defl_seq(W, v, 0); run--;
            while (run >= 3) { const u32 r = run < 6 ? run : 6; bfq_defl_seq(W, 16, r - 3); run -= r; }
        }
        for (; run > 0; run--) bfq_defl_seq(W, v, 0);
    }
    u32 used = 0;
    for (u32 i = 0; i < 19; i++) used += W->clFreq[i] ? 1 : 0;
    if (used < 2) { if (!W->clFreq[0]) W->clFreq[0] = 1; else W->clFreq[18] = 1; }   // the code-length code has to be complete
    bfq_defl_lengths(W->clFreq, 19, 7, W->clLen, W);
    bfq_defl_codes(W->clLen, 19, W->clCode);
    const char *order = bfq_defl_order();
    u32 hclen = 19;
    while (hclen > 4 && !W->clLen[(u8)order[hclen - 1]]) hclen--;
    W->hclen = hclen;
    u32 bits = 3 + 14 + 3 * hclen;
    for (u32 i = 0; i < W->nseq; i++) {
        const u32 s = W->seq[i] & 255u;
        bits += W->clLen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
    }
    W->hdrBits = bits;
}
BFQ_HD void bfq_defl_header_put(const bfq_defl_work *W, bfq_defl_bw &b)
{
    bfq_defl_put(b, 1, 1); bfq_defl_put(b, 2, 2);
    bfq_defl_put(b, W->hlit - 257, 5); bfq_defl_put(b, W->hdist - 1, 5); bfq_defl_put(b, W->hclen - 4, 4);
    const char *order = bfq_defl_order();
    for (u32 i = 0; i < W->hclen; i++) bfq_defl_put(b, W->clLen[(u8)order[i]], 3);
    for (u32 i = 0; i < W->nseq; i++) {
        const u32 s = W->seq[i] & 255u, x = W->seq[i] >> 8;
        bfq_defl_put(b, W->clCode[s], W->clLen[s]);
        if (s >= 16) bfq_defl_put(b, x, s == 16 ? 2 : s == 17 ? 3 : 7);
    }
}
BFQ_HD u32 bfq_defl_tok_bits(const bfq_defl_work *W, u32 tk)
{
    if (!(tk & BFQ_DEFL_MATCH)) return W->lens[tk];
    const u32 len = (tk & 255u) + 3, dist = ((tk >> 8) & 0x7FFFu) + 1;
    return W->lens[bfq_defl_lsym(len)] + bfq_defl_lext(len) + W->lens[288 + bfq_defl_dsym(dist)] + bfq_defl_dext(dist);
}
BFQ_HD void bfq_defl_tok_put(const bfq_defl_work *W, u32 tk, bfq_defl_bw &b)
{
    if (!(tk & BFQ_DEFL_MATCH)) { bfq_defl_put(b, W->lcode[tk], W->lens[tk]); return; }
    const u32 len = (tk & 255u) + 3, dist = ((tk >> 8) & 0x7FFFu) + 1;
    const u32 ls = bfq_defl_lsym(len), lx = bfq_defl_lext(len), ds = bfq_defl_dsym(dist), dx = bfq_defl_dext(dist);
    bfq_defl_put(b, W->lcode[ls], W->lens[ls]);
    if (lx) bfq_defl_put(b, (len - 3) & ((1u << lx) - 1u), lx);
    bfq_defl_put(b, W->dcode[ds], W->lens[288 + ds]);
    if (dx) bfq_defl_put(b, (dist - 1) & ((1u << dx) - 1u), dx);
}

// ---------------------------------------------------------------- one member
// The member of t[0, n), 1 <= n <= 65280, into slot[0, cap): cap a multiple of 4 and at least n + 31, slot word-aligned.
// tok: room for n tokens.  level 0: stored.  Returns the member's size (<= n + 31), the same in every lane; nothing is
// written at or behind slot[cap].
BFQ_HD u32 bfq_defl_member(const u8 *t, u32 n, int level, u8 *slot, u32 cap, u32 *tok, bfq_defl_work *W, const u32 *crcTab, u32 lane, u32 nl)
{
    BFQ_DEFL_SYNC();
    W->crc[lane] = bfq_crc32_part(crcTab, t, n, lane, nl);
    if (lane == 0) W->over = 0;
    BFQ_DEFL_SYNC();
    u32 crc = 0;
    for (u32 i = 0; i < nl; i++) crc ^= W->crc[i];
    u32 pay = n + 5;                                             // payload bytes; the stored form's to begin with
    bool coded = false;
    if (level > 0) {
        bfq_defl_parse(t, n, tok, W, lane, nl);
        if (lane == 0) bfq_defl_header_plan(W);
        BFQ_DEFL_SYNC();
        const u32 ntok = W->ntok, chunk = (ntok + nl - 1) / nl;
        const u32 lo = lane * chunk < ntok ? lane * chunk : ntok, hi = lo + chunk < ntok ? lo + chunk : ntok;
        u32 mine = 0;
        for (u32 i = lo; i < hi; i++) mine += bfq_defl_tok_bits(W, tok[i]);
        W->laneBits[lane] = mine;
        BFQ_DEFL_SYNC();
        u32 start = W->hdrBits, total = W->hdrBits + W->lens[256];
        for (u32 i = 0; i < nl; i++) { if (i < lane) start += W->laneBits[i]; total += W->laneBits[i]; }
        const u32 codedPay = (total + 7) / 8;
        if (codedPay < pay && 18 + codedPay + 8 <= cap) {
            const u32 capWords = cap / 4, words = (18 + codedPay + 8 + 3) / 4;
            u32 *w = (u32 *)slot;
            for (u32 i = lane; i < words && i < capWords; i += nl) w[i] = 0;
            BFQ_DEFL_SYNC();
            bfq_defl_bw b = bfq_defl_bw_at(w, capWords, 18 * 8 + start);
            for (u32 i = lo; i < hi; i++) bfq_defl_tok_put(W, tok[i], b);
            bfq_defl_flush(b);
            u32 over = b.over;
            if (lane == 0) {
                const u32 size = 18 + codedPay + 8;
                b = bfq_defl_bw_at(w, capWords, 0);
                for (u32 i = 0; i < 16; i++) bfq_defl_put(b, bfq_defl_eof_byte(i), 8);
                bfq_defl_put(b, size - 1, 16);
                bfq_defl_header_put(W, b);
                bfq_defl_flush(b);
                over |= b.over;
                b = bfq_defl_bw_at(w, capWords, 18 * 8 + total - W->lens[256]);
                bfq_defl_put(b, W->lcode[256], W->lens[256]);
                bfq_defl_flush(b);
                over |= b.over;
                b = bfq_defl_bw_at(w, capWords, (18 + codedPay) * 8);
                bfq_defl_put(b, crc, 32); bfq_defl_put(b, n, 32);
                bfq_defl_flush(b);
                over |= b.over;
            }
            if (over) W->over = 1;
            BFQ_DEFL_SYNC();
            if (!W->over) { coded = true; pay = codedPay; }
        }
    }
    if (!coded) {
        if (lane == 0) {
            for (u32 i = 0; i < 16; i++) slot[i] = bfq_defl_eof_byte(i);
            const u32 size = 18 + pay + 8;
            slot[16] = (u8)((size - 1) & 255u); slot[17] = (u8)((size - 1) >> 8);
            slot[18] = 1;                                        // BFINAL, BTYPE 0, the rest of the byte
            slot[19] = (u8)(n & 255u); slot[20] = (u8)(n >> 8); slot[21] = (u8)(~n & 255u); slot[22] = (u8)((~n >> 8) & 255u);
            for (u32 i = 0; i < 4; i++) { slot[23 + n + i] = (u8)(crc >> (8 * i)); slot[27 + n + i] = (u8)(n >> (8 * i)); }
        }
        for (u32 i = lane; i < n; i += nl) slot[23 + i] = t[i];
    }
    BFQ_DEFL_SYNC();
    return 18 + pay + 8;
}

// The host form: the whole text, one lane.  0, or 1: cap below bfq_defl_bound(len) (nothing written), 2: no memory.
inline int bfq_defl_host(const u8 *in, u64 len, int level, u8 *out, u64 cap, u64 *outLen)
{
    *outLen = 0;
    if (cap < bfq_defl_bound(len)) return 1;
    bfq_defl_work *W = (bfq_defl_work *)malloc(sizeof(bfq_defl_work));
    u32 *tok = (u32 *)malloc(sizeof(u32) * BFQ_DEFL_PIECE), *slot = (u32 *)malloc(BFQ_DEFL_SLOT), crcTab[256];
    if (!W || !tok || !slot) { free(W); free(tok); free(slot); return 2; }
    for (u32 i = 0; i < 256; i++) crcTab[i] = bfq_crc32_entry(i);
    u64 at = 0;
    for (u64 off = 0; off < len; off += BFQ_DEFL_PIECE) {
        const u32 n = (u32)(len - off < BFQ_DEFL_PIECE ? len - off : BFQ_DEFL_PIECE);
        const u32 size = bfq_defl_member(in + off, n, level, (u8 *)slot, BFQ_DEFL_SLOT, tok, W, crcTab, 0, 1);
        memcpy(out + at, slot, size);
        at += size;
    }
    for (u32 i = 0; i < BFQ_BGZF_EOF_LEN; i++) out[at + i] = bfq_defl_eof_byte(i);
    *outLen = at + BFQ_BGZF_EOF_LEN;
    free(W); free(tok); free(slot);
    return 0;
}
