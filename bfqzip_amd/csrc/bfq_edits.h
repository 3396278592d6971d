// bfq_edits.h -- a run's base edits as a file: container BFQEDIT1 (include/bfqzip_hip.h), shared by the host statement
// (bfq_edits_encode / bfq_edits_decode / bfq_fastq_edits_host / bfq_fastq_unedit_host, bfq_edits_host.cpp) and the kernels
// that make, unpack and apply it (k_edits.hip).  Plain C++, no HIP types.
//   header   64 bytes: "BFQEDIT1" | u64 N | u64 T | u64 E | u32 S = 1024 | u32 flags = 0 | u64 shape | u64 target_sum | u64 payload
//   payload  u64 first[nseg] | u8 w[nseg], zero-padded to 8 | per segment ceil((c - 1) w / 64) u64 words of gaps | u8 byte[E],
//            zero-padded to 8;  nseg = ceil(E / S), c = the segment's edits; gap j of a segment in bits [j w, (j + 1) w) of its
//            words, bit b being bit b % 64 of word b / 64 (BFQPERM1's order)
// An edit is (g, byte): g = read_off[r] + j, byte = the INPUT's byte there; strictly ascending g.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../include/bfqzip_hip.h"
#include "bfq_common.h"
#include "bfq_reorder.h"                                  // bfq_fmix64

#define BFQ_EDIT_HDR 64
#define BFQ_EDIT_MAGIC "BFQEDIT1"
#define BFQ_EDIT_SEG 1024u
#define BFQ_EDIT_WMAX 56u
#define BFQ_EDIT_TMAX (1ull << 56)                        // T <= 2^56: a gap has at most 56 bits
#define BFQ_EDIT_NOPOS (~0ull)                            // first_bad of a fault in the header or the table

BFQ_HD u64 bfq_edit_shape_term(u64 r, u64 len) { return bfq_fmix64(r * 65536ull + len); }
BFQ_HD u64 bfq_edit_sum_term(u64 g, u32 b) { return bfq_fmix64(g * 256ull + b); }
BFQ_HD u32 bfq_edit_bitlen(u64 v) { return (u32)(64 - bfq_clz64(v)); }                       // 0 for 0
BFQ_HD u64 bfq_edit_pad8(u64 n) { return (n + 7) & ~7ull; }
BFQ_HD u64 bfq_edit_nseg(u64 E) { return (E + BFQ_EDIT_SEG - 1) / BFQ_EDIT_SEG; }
BFQ_HD u64 bfq_edit_seg_count(u64 E, u64 s) { const u64 k0 = s * BFQ_EDIT_SEG; return E - k0 < BFQ_EDIT_SEG ? E - k0 : BFQ_EDIT_SEG; }
BFQ_HD u64 bfq_edit_seg_words(u64 c, u32 w) { return ((c - 1) * w + 63) >> 6; }              // c >= 1, w <= 56
BFQ_HD bool bfq_edit_byte_ok(u32 b) { return b >= 33u && b <= 126u; }

// gap j of a segment's words (w >= 1)
BFQ_HD u64 bfq_edit_get(const u64 *words, u64 j, u32 w)
{
    const u64 bit = j * w, q = bit >> 6;
    const u32 sh = (u32)(bit & 63);
    u64 v = words[q] >> sh;
    if (sh + w > 64) v |= words[q + 1] << (64 - sh);     // (the gap ends inside the segment's words, so q + 1 exists)
    return v & ((1ull << w) - 1);
}
// word q of the gaps of the edits pos[0 .. ngaps] of one segment (w >= 1): the gaps that overlap bits [64 q, 64 q + 64)
BFQ_HD u64 bfq_edit_word(const u64 *pos, u64 ngaps, u32 w, u64 q)
{
    const u64 lo = q << 6;
    u64 j = lo / w, out = 0;
    for (; j < ngaps; j++) {
        const u64 bit = j * w;
        if (bit >= lo + 64) break;
        const u64 v = pos[j + 1] - pos[j] - 1;
        out |= bit >= lo ? v << (bit - lo) : v >> (lo - bit);
    }
    return out;
}

// ---- host side
static inline u64 bfq_edit_ld64(const u8 *p) { u64 v; memcpy(&v, p, 8); return v; }          // (little-endian hosts, as everywhere)
static inline u32 bfq_edit_ld32(const u8 *p) { u32 v; memcpy(&v, p, 4); return v; }

// one member as its header states it; offsets count from the member's first byte
struct BfqEditMember {
    u64 N = 0, T = 0, E = 0, shape = 0, targetSum = 0, payload = 0;
    u64 nseg = 0, offFirst = 0, offW = 0, offGaps = 0, offBytes = 0, gapWords = 0;
    u64 bytes() const { return BFQ_EDIT_HDR + payload; }
};

static inline u64 bfq_edits_bound_of(u64 E, u64 T)
{
    if (T > BFQ_EDIT_TMAX || E > T) return 0;
    const u64 nseg = bfq_edit_nseg(E);
    const u32 w = T >= 2 ? bfq_edit_bitlen(T - 2) : 0u;    // the largest gap a collection of T bases has room for
    return BFQ_EDIT_HDR + 8 * nseg + bfq_edit_pad8(nseg) + 8 * nseg * bfq_edit_seg_words(BFQ_EDIT_SEG, w) + bfq_edit_pad8(E);
}

// The header and the table of the member that starts at z, of which `avail` bytes are there.  nullptr: well formed so far;
// else what is wrong.  *badSeg (when the fault is a width above 56): that segment, else ~0.  No edit is looked at.
static inline const char *bfq_edits_member(const u8 *z, u64 avail, BfqEditMember *M, u64 *badSeg)
{
    if (badSeg) *badSeg = ~0ull;
    if (!z || avail < BFQ_EDIT_HDR || memcmp(z, BFQ_EDIT_MAGIC, 8)) return "not a BFQEDIT1 container (magic)";
    BfqEditMember m;
    m.N = bfq_edit_ld64(z + 8); m.T = bfq_edit_ld64(z + 16); m.E = bfq_edit_ld64(z + 24);
    const u32 S = bfq_edit_ld32(z + 32), flags = bfq_edit_ld32(z + 36);
    m.shape = bfq_edit_ld64(z + 40); m.targetSum = bfq_edit_ld64(z + 48); m.payload = bfq_edit_ld64(z + 56);
    if (S != BFQ_EDIT_SEG) return "damaged BFQEDIT1 container: S is not 1024";
    if (flags) return "damaged BFQEDIT1 container: flags set";
    if (m.T > BFQ_EDIT_TMAX || m.E > m.T) return "damaged BFQEDIT1 container: more edits than bases, or more than 2^56 bases";
    if (m.payload > avail - BFQ_EDIT_HDR) return "damaged BFQEDIT1 container: shorter than its stated length";
    m.nseg = bfq_edit_nseg(m.E);
    m.offFirst = BFQ_EDIT_HDR;
    m.offW = m.offFirst + 8 * m.nseg;
    m.offGaps = m.offW + bfq_edit_pad8(m.nseg);
    if (m.offGaps - BFQ_EDIT_HDR + bfq_edit_pad8(m.E) > m.payload) return "damaged BFQEDIT1 container: the stated length is not exact";
    for (u64 s = 0; s < m.nseg; s++) {
        const u32 w = z[m.offW + s];
        if (w > BFQ_EDIT_WMAX) { if (badSeg) *badSeg = s; return "damaged BFQEDIT1 container: a gap width above 56"; }
        m.gapWords += bfq_edit_seg_words(bfq_edit_seg_count(m.E, s), w);
        if (m.gapWords > m.payload / 8) return "damaged BFQEDIT1 container: the stated length is not exact";
    }
    m.offBytes = m.offGaps + 8 * m.gapWords;
    if (m.offBytes - BFQ_EDIT_HDR + bfq_edit_pad8(m.E) != m.payload) return "damaged BFQEDIT1 container: the stated length is not exact";
    for (u64 i = m.offW + m.nseg; i < m.offGaps; i++)
        if (z[i]) return "damaged BFQEDIT1 container: padding that is not zero";
    for (u64 i = m.offBytes + m.E; i < m.offBytes + bfq_edit_pad8(m.E); i++)
        if (z[i]) return "damaged BFQEDIT1 container: padding that is not zero";
    *M = m;
    return nullptr;
}

static inline void bfq_edits_put_header(u8 *out, u64 N, u64 T, u64 E, u64 shape, u64 targetSum, u64 payload)
{
    const u32 S = BFQ_EDIT_SEG, flags = 0;
    memcpy(out, BFQ_EDIT_MAGIC, 8);
    memcpy(out + 8, &N, 8); memcpy(out + 16, &T, 8); memcpy(out + 24, &E, 8); memcpy(out + 32, &S, 4); memcpy(out + 36, &flags, 4);
    memcpy(out + 40, &shape, 8); memcpy(out + 48, &targetSum, 8); memcpy(out + 56, &payload, 8);
}

// the statement of the encoder: pos[E] strictly ascending and below T, byte[E] in 33..126
static inline int bfq_edits_encode_host(const u64 *pos, const u8 *byte, u64 E, u64 N, u64 T, u64 shape, u64 targetSum, u8 *out, u64 cap,
                                        u64 *outLen)
{
    if (outLen) *outLen = 0;
    if ((E && (!pos || !byte)) || !out || T > BFQ_EDIT_TMAX || E > T) return BFQ_E_ARG;
    for (u64 k = 0; k < E; k++)
        if (pos[k] >= T || (k && pos[k] <= pos[k - 1]) || !bfq_edit_byte_ok(byte[k])) return BFQ_E_ARG;
    const u64 nseg = bfq_edit_nseg(E);
    u64 words = 0;
    for (u64 s = 0; s < nseg; s++) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(E, s);
        u64 mx = 0;
        for (u64 j = 0; j + 1 < c; j++) { const u64 g = pos[k0 + j + 1] - pos[k0 + j] - 1; mx = g > mx ? g : mx; }
        words += bfq_edit_seg_words(c, bfq_edit_bitlen(mx));
    }
    const u64 payload = 8 * nseg + bfq_edit_pad8(nseg) + 8 * words + bfq_edit_pad8(E);
    if (cap < BFQ_EDIT_HDR + payload) return BFQ_E_ARG;
    memset(out, 0, BFQ_EDIT_HDR + payload);
    bfq_edits_put_header(out, N, T, E, shape, targetSum, payload);
    u8 *first = out + BFQ_EDIT_HDR, *wt = first + 8 * nseg, *gw = wt + bfq_edit_pad8(nseg);
    for (u64 s = 0; s < nseg; s++) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(E, s);
        u64 mx = 0;
        for (u64 j = 0; j + 1 < c; j++) { const u64 g = pos[k0 + j + 1] - pos[k0 + j] - 1; mx = g > mx ? g : mx; }
        const u32 w = bfq_edit_bitlen(mx);
        memcpy(first + 8 * s, &pos[k0], 8);
        wt[s] = (u8)w;
        const u64 nw = bfq_edit_seg_words(c, w);
        for (u64 q = 0; q < nw; q++) { const u64 v = bfq_edit_word(pos + k0, c - 1, w, q); memcpy(gw + 8 * q, &v, 8); }
        gw += 8 * nw;
    }
    if (E) memcpy(gw, byte, E);
    if (outLen) *outLen = BFQ_EDIT_HDR + payload;
    return BFQ_OK;
}

// the statement of the decoder: ONE member of exactly len bytes.  Nothing is written unless the member is well formed.
// *firstBad: the smallest offending edit, BFQ_EDIT_NOPOS when the fault is in the header, the table or the arguments.
static inline int bfq_edits_decode_host(const u8 *z, u64 len, u64 *pos, u8 *byte, u64 capEntries, BfqEditMember *Mout, u64 *firstBad,
                                        const char **why)
{
    if (firstBad) *firstBad = BFQ_EDIT_NOPOS;
    BfqEditMember M;
    u64 badSeg = ~0ull;
    const char *e = bfq_edits_member(z, len, &M, &badSeg);
    if (!e && M.bytes() != len) e = "damaged BFQEDIT1 container: the stated length is not exact";
    if (e) { if (why) *why = e; if (firstBad && badSeg != ~0ull) *firstBad = badSeg * BFQ_EDIT_SEG; return BFQ_E_ARG; }
    if (why) *why = "damaged BFQEDIT1 container: a bad edit";
    u64 *tmp = (u64 *)malloc((size_t)(M.E ? M.E : 1) * 8);
    if (!tmp) return BFQ_E_NOMEM;
    u64 bad = BFQ_EDIT_NOPOS, wo = 0, prev = 0;
    for (u64 s = 0; s < M.nseg && bad == BFQ_EDIT_NOPOS; s++) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(M.E, s), nw = bfq_edit_seg_words(c, z[M.offW + s]);
        const u32 w = z[M.offW + s];
        const u8 *gw = z + M.offGaps + 8 * wo;
        u64 g = bfq_edit_ld64(z + M.offFirst + 8 * s), mx = 0;
        // the segment as a whole: its first position against the running one, the width, the padding of its last word
        bool segBad = s && g <= prev;
        std::vector<u64> words(nw + 1, 0);
        for (u64 q = 0; q < nw; q++) words[q] = bfq_edit_ld64(gw + 8 * q);
        for (u64 j = 0; j + 1 < c; j++) { const u64 v = w ? bfq_edit_get(words.data(), j, w) : 0; mx = v > mx ? v : mx; }
        segBad |= bfq_edit_bitlen(mx) != w;
        const u64 used = (c - 1) * w & 63;
        segBad |= nw && used && words[nw - 1] >> used;
        if (segBad) { bad = k0; break; }
        for (u64 j = 0; j < c; j++) {
            if (j) g += (w ? bfq_edit_get(words.data(), j - 1, w) : 0) + 1;
            if (g >= M.T || !bfq_edit_byte_ok(z[M.offBytes + k0 + j])) { bad = k0 + j; break; }
            tmp[k0 + j] = g;
        }
        prev = g;
        wo += nw;
    }
    if (bad != BFQ_EDIT_NOPOS) { free(tmp); if (firstBad) *firstBad = bad; return BFQ_E_ARG; }
    if (capEntries < M.E || (M.E && (!pos || !byte))) { free(tmp); if (why) *why = "bfq_edits_decode: cap_entries below the member's edits"; return BFQ_E_ARG; }
    if (M.E) { memcpy(pos, tmp, (size_t)M.E * 8); memcpy(byte, z + M.offBytes, (size_t)M.E); }
    free(tmp);
    if (Mout) *Mout = M;
    if (why) *why = nullptr;
    return BFQ_OK;
}
