// bfq_pairs.h -- interleaved paired FASTQ, host and device: the definition, the key of a record, the role of a record in a
// run of equal keys, the messages and the two host forms.  Plain C++, shared by the kernels (k_pairs.hip), the host side
// (bfq_pairs.hip) and the sanitizer program (tests/cxx/test_pairs.cpp).
//
// "One FASTQ text with the mates alternating" <-> "two texts of mates (and one of singletons)."  This project's definition:
//   The text: plain FASTQ as bfq_fastq_reorder reads it, four lines per record.  A record is its four lines byte for byte:
//     the header comment, what follows the '+' and CRs stay as they are.  A text whose last line lacks its LF gets one.
//     Malformed text keeps the words of bfq_fastq_run: "FASTQ: number of lines is not a multiple of 4", "FASTQ: len(DNA) !=
//     len(QS) in a record" (BFQ_E_ARG; CR before LF does not count), "read longer than BFQ_MAX_READ_LEN" (BFQ_E_TOO_LONG), looked
//     for in that order, text by text.  A text that begins with 1f 8b is refused: "... inflate the text first".
//   Key of a record: the bytes of the header line behind its first byte (the '@') up to the first blank, tab, CR or the line's
//     end.  With mate_suffix a trailing "/1" or "/2" is removed -- EITHER one, whichever text or position the record stands
//     at, where at least one byte remains.  Keys compare in full, at any length; two empty keys ("@" alone: what a run without
//     kept headers writes) are equal.  This is LAXER than bfq_ubam.h, which removes only the suffix that matches the text the
//     record came from: in orphan mode the role of a record is not known before the pairing, and one rule serves both modes
//     and both directions.  So "x/1" and "x/1" are a pair here.
//   Split, strict mode (orphans = 0): an odd record count N is refused, "interleaved FASTQ: <N> records, an odd number".
//     Record 2k goes to output 1, record 2k + 1 to output 2; output 0 stays empty.  With check_names the keys of the two
//     records of pair k must be equal, else "interleaved FASTQ: pair <k> (records <2k> and <2k+1>): the names differ": the
//     first offending pair of the file is named (the device: one atomicMin).
//   Split, orphan mode (orphans = 1): the file is cut into maximal runs of consecutive records with equal keys.  In a run that
//     starts at record s and has r records, records s + 2j and s + 2j + 1 are a pair for 2j + 1 < r: outputs 1 and 2.  With r
//     odd the run's last record is a singleton: output 0, in file order.  Nothing is refused for pairing; check_names is
//     implied.
//   Merge: text[1] and text[2] are the mates, an optional text[0] goes behind the pairs (the indices of bfq_fastq_to_bam).
//     Output: record k of text 1, record k of text 2, for every k, then the records of text 0.  An absent text holds no
//     reads.  Different read counts: "FASTQ interleave: text 1 holds <n> reads, text 2 holds <m>".  With check_names:
//     "FASTQ interleave: pair <k>: the names differ", the first one.
//   Repair (bfq_fastq_repair*): the mates are matched by name wherever they stand.  text[1], text[2] and text[0] as in the
//     merge; the global number g of a record counts the records of text 1, then those of text 2, then those of text 0.
//     Hint of a record: 1 from text 1, 2 from text 2; from text 0, with mate_suffix, 1 where the key lost a "/1", 2 where it
//     lost a "/2"; else 0 (none).  A group is all records of the call with equal keys, split in global order into the lists
//     L1, L2 and L0 by hint.  Pairs: (L1[k], L2[k]) for k < min(|L1|, |L2|), then (L0[2j], L0[2j + 1]) for 2j + 1 < |L0|;
//     the first of a pair goes to output 1, the second to output 2, every other record of the group to output 0.  Pairs
//     come in increasing global number of their output-1 record (a repaired R1 keeps R1's order), singletons in increasing
//     global number.  The outputs are a function of the texts and mate_suffix alone.
//     How: the records are sorted by the top hash_bits bits of a 64-bit hash of the key (bfq_repair_hash, below; stable, so a
//     run of equal sort keys is in global order), a run is cut into groups by the full hash and then the key's bytes.  A run of
//     more than BFQ_REPAIR_RUN_MAX records is refused, "FASTQ repair: more than 1024 records share a name or a name hash (the
//     first: record <i> of text <k>): names do not identify the mates": <i> is the smallest global number in such a run,
//     given relative to its text.  This bounds every loop of the grouping and refuses a file of "@"-only headers.
//     Statistics: dup_groups = groups of more than two records, mixed_runs = runs that hold more than one name, max_run = the
//     longest run; the last two depend on hash_bits and the seed, nothing else does.
//   All refusals but the too-long read are BFQ_E_ARG.  In every form a refusal writes nothing: sizes and checks are finished
//   before the first byte moves, and the output lengths are exact before anything is written.
// Out of scope: adding or rewriting "/1" "/2"; BGZF parts inside these calls (the front-ends inflate with bfq_bgzf_inflate* /
// bfq_gzip_inflate*); repair inside bfq_bam itself; interleaved output straight from bfq_restore.
#pragma once
#include "bfq_common.h"
#include "bfq_reorder.h"                            // bfq_fmix64
#include "../../include/bfqzip_hip.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

enum {
    BFQ_PAIRS_OK = 0,
    BFQ_PAIRS_E_RESERVED,    // bfq_pairs_opts.reserved != 0
    BFQ_PAIRS_E_GZIP,        // a text begins with 1f 8b
    BFQ_PAIRS_E_LINES,       // lines not a multiple of 4
    BFQ_PAIRS_E_FASTQ,       // len(DNA) != len(QS)
    BFQ_PAIRS_E_TOO_LONG,    // a read above BFQ_MAX_READ_LEN
    BFQ_PAIRS_E_ODD,         // strict split: an odd record count
    BFQ_PAIRS_E_COUNTS,      // merge: the mates' read counts differ
    BFQ_PAIRS_E_NAMES,       // the keys of a pair differ
    BFQ_PAIRS_E_CAP,         // an output below its text
    BFQ_PAIRS_E_HASH_BITS,   // repair: bfq_repair_opts.hash_bits outside 1..40
    BFQ_PAIRS_E_RUN          // repair: more than BFQ_REPAIR_RUN_MAX records in a run of equal sort keys
};
#define BFQ_REPAIR_RUN_MAX 1024u
#define BFQ_PAIRS_NONE (~0ull)
// what is refused: merge = 1 (0: the split, 2: the repair), text k, the two numbers the message names
struct bfq_pairs_err { u32 kind = 0, merge = 0, k = 0, pad = 0; u64 n = 0, m = 0; };
inline int bfq_pairs_code(const bfq_pairs_err &E) { return E.kind == BFQ_PAIRS_E_TOO_LONG ? BFQ_E_TOO_LONG : BFQ_E_ARG; }
inline std::string bfq_pairs_message(const bfq_pairs_err &E)
{
    char b[320];
    switch (E.kind) {
    case BFQ_PAIRS_E_RESERVED: return E.merge == 2 ? "bfq_repair_opts.reserved: must be 0" : "bfq_pairs_opts.reserved: must be 0";
    case BFQ_PAIRS_E_HASH_BITS: return "bfq_repair_opts.hash_bits: must be 1..40";
    case BFQ_PAIRS_E_RUN:
        snprintf(b, sizeof b, "FASTQ repair: more than %u records share a name or a name hash (the first: record %llu of text %u): names do not identify the mates",
                 BFQ_REPAIR_RUN_MAX, E.n, E.k);
        return b;
    case BFQ_PAIRS_E_LINES: return "FASTQ: number of lines is not a multiple of 4";
    case BFQ_PAIRS_E_FASTQ: return "FASTQ: len(DNA) != len(QS) in a record";
    case BFQ_PAIRS_E_TOO_LONG: return "read longer than BFQ_MAX_READ_LEN";
    case BFQ_PAIRS_E_GZIP:
        if (E.merge) snprintf(b, sizeof b, "FASTQ %s: text %u is compressed (it begins with 1f 8b): inflate the text first", E.merge == 2 ? "repair" : "interleave", E.k);
        else snprintf(b, sizeof b, "interleaved FASTQ: the text is compressed (it begins with 1f 8b): inflate the text first");
        return b;
    case BFQ_PAIRS_E_ODD: snprintf(b, sizeof b, "interleaved FASTQ: %llu records, an odd number", E.n); return b;
    case BFQ_PAIRS_E_COUNTS: snprintf(b, sizeof b, "FASTQ interleave: text 1 holds %llu reads, text 2 holds %llu", E.n, E.m); return b;
    case BFQ_PAIRS_E_NAMES:
        if (E.merge) snprintf(b, sizeof b, "FASTQ interleave: pair %llu: the names differ", E.n);
        else snprintf(b, sizeof b, "interleaved FASTQ: pair %llu (records %llu and %llu): the names differ", E.n, 2 * E.n, 2 * E.n + 1);
        return b;
    case BFQ_PAIRS_E_CAP: return E.merge == 1 ? "output buffer smaller than the interleaved text" : "output buffer smaller than the text it receives";
    default: return "ok";
    }
}

// ---------------------------------------------------------------- the rule, for one lane
// The key of the header line t[s, s + n): where it starts and its length.  The loop ends at the line's length.
BFQ_HD void bfq_pairs_key(const u8 *t, u64 s, u64 n, u32 mateSuffix, u64 *ks, u64 *kl)
{
    if (!n) { *ks = s; *kl = 0; return; }
    const u64 b = s + 1, e = s + n;
    u64 p = b;
    while (p < e && t[p] != ' ' && t[p] != '\t' && t[p] != '\r') p++;
    u64 l = p - b;
    if (mateSuffix && l > 2 && t[b + l - 2] == '/' && (t[b + l - 1] == '1' || t[b + l - 1] == '2')) l -= 2;
    *ks = b; *kl = l;
}
// Are the keys of the header lines ta[sa, sa + na) and tb[sb, sb + nb) equal?  Each key is read where it lies in its text.
BFQ_HD bool bfq_pairs_same(const u8 *ta, u64 sa, u64 na, const u8 *tb, u64 sb, u64 nb, u32 mateSuffix)
{
    u64 ka, la, kb, lb;
    bfq_pairs_key(ta, sa, na, mateSuffix, &ka, &la);
    bfq_pairs_key(tb, sb, nb, mateSuffix, &kb, &lb);
    if (la != lb) return false;
    for (u64 j = 0; j < la; j++)
        if (ta[ka + j] != tb[kb + j]) return false;
    return true;
}
// Orphan mode: the output of record i whose run starts at record `start`; last: i is its run's last record.
BFQ_HD u32 bfq_pairs_role(u64 i, u64 start, bool last) { return ((i - start) & 1u) ? 2u : last ? 0u : 1u; }

// ---- repair: the hash of a key, the hint of a record, the role of a record in its group
// The key's bytes in 8-byte little-endian chunks w_j, the last one zero-padded: acc = sum_j fmix64(w_j + C * (j + 1)) mod 2^64,
// h = fmix64(acc ^ fmix64(L ^ seed)) with L the key's length.  The sum is commutative on purpose: lanes that share a record
// each take chunks and reduce.  Keys that differ only by trailing zero bytes have equal chunks and differ through L.
#define BFQ_REPAIR_GOLD 0x9E3779B97F4A7C15ull
BFQ_HD u64 bfq_repair_word(const u8 *p, u64 n)           // the first n <= 8 bytes at p, little-endian, zero-padded
{
    u64 w = 0;
    for (u64 b = 0; b < n; b++) w |= (u64)p[b] << (8 * b);
    return w;
}
BFQ_HD u64 bfq_repair_chunk(u64 w, u64 j) { return bfq_fmix64(w + BFQ_REPAIR_GOLD * (j + 1)); }
BFQ_HD u64 bfq_repair_finish(u64 acc, u64 L, u64 seed) { return bfq_fmix64(acc ^ bfq_fmix64(L ^ seed)); }
BFQ_HD u64 bfq_repair_hash(const u8 *key, u64 L, u64 seed)
{
    u64 acc = 0;
    for (u64 j = 0; 8 * j < L; j++) acc += bfq_repair_chunk(bfq_repair_word(key + 8 * j, L - 8 * j < 8 ? L - 8 * j : 8), j);
    return bfq_repair_finish(acc, L, seed);
}
BFQ_HD u64 bfq_repair_sort_key(u64 h, u32 hashBits) { return h >> (64 - hashBits); }
// The hint of a record of text `src` whose header line is t[s, s + n) and whose key (bfq_pairs_key) is t[ks, ks + kl): behind a
// key that lost its suffix stands the '/', behind any other a blank, a tab, a CR or the line's end.
BFQ_HD u32 bfq_repair_hint(const u8 *t, u64 s, u64 n, u32 src, u64 ks, u64 kl)
{
    if (src) return src;
    return ks + kl < s + n && t[ks + kl] == '/' ? (t[ks + kl + 1] == '1' ? 1u : 2u) : 0u;
}
// The role of a record with hint `hint` that has before[] records of its group in front of it, by hint, in a group of
// total[]: 0, 1 or 2 = its output.  *mate: for a pair member the index, in its list, of the group's record that is the
// pair's output-1 record (list L1 for hints 1 and 2, list L0 for hint 0) -- for an output-1 record its own.
BFQ_HD u32 bfq_repair_role(u32 hint, const u32 before[3], const u32 total[3], u32 *mate)
{
    const u32 p12 = total[1] < total[2] ? total[1] : total[2];
    *mate = 0;
    if (hint) {
        if (before[hint] >= p12) return 0;
        *mate = before[hint];
        return hint;
    }
    if ((before[0] | 1u) >= total[0]) return 0;            // the last of an odd list
    *mate = before[0] & ~1u;
    return (before[0] & 1u) ? 2u : 1u;
}

// ---------------------------------------------------------------- host side
inline void bfq_pairs_defaults(bfq_pairs_opts *o) { o->check_names = 1; o->mate_suffix = 1; o->orphans = 0; o->reserved = 0; }
inline bool bfq_pairs_resolve(const bfq_pairs_opts *in, bfq_pairs_opts *O, bfq_pairs_err *E)
{
    bfq_pairs_defaults(O);
    if (in) *O = *in;
    if (O->reserved) { E->kind = BFQ_PAIRS_E_RESERVED; return false; }
    return true;
}
inline bool bfq_pairs_gzip_ok(const u8 first[2], u64 len, u32 merge, u32 k, bfq_pairs_err *E)
{
    if (len < 2 || first[0] != 0x1F || first[1] != 0x8B) return true;
    E->kind = BFQ_PAIRS_E_GZIP; E->merge = merge; E->k = k;
    return false;
}

// The records of a text as one host thread finds them: where the header lines start (hs[N] = the text's length with its
// final LF) and how long they are.
struct bfq_pairs_index { std::vector<u64> hs; std::vector<u64> hl; u64 N = 0, tl = 0; };
inline bool bfq_pairs_parse(const u8 *t, u64 len, bfq_pairs_index *I, bfq_pairs_err *E)
{
    std::vector<u64> le;
    for (u64 p = 0; p < len; p++)
        if (t[p] == 10) le.push_back(p);
    if (len && t[len - 1] != 10) le.push_back(len);
    if (le.size() % 4) { E->kind = BFQ_PAIRS_E_LINES; return false; }
    const u64 N = le.size() / 4;
    bool badLen = false, tooLong = false;
    I->hs.assign(N + 1, 0); I->hl.assign(N + 1, 0);
    for (u64 i = 0; i < N; i++) {
        u64 s[4], e[4];
        for (int k = 0; k < 4; k++) {
            const u64 li = 4 * i + k;
            s[k] = li ? le[li - 1] + 1 : 0;
            e[k] = le[li];
            if (k && e[k] > s[k] && t[e[k] - 1] == 13) e[k]--;
        }
        I->hs[i] = s[0]; I->hl[i] = e[0] - s[0];
        const u64 l = e[1] - s[1];
        if (e[3] - s[3] != l) badLen = true;
        if (l > BFQ_MAX_READ_LEN) tooLong = true;
    }
    I->N = N;
    I->tl = len + (len && t[len - 1] != 10 ? 1 : 0);
    I->hs[N] = I->tl;
    if (badLen) { E->kind = BFQ_PAIRS_E_FASTQ; return false; }
    if (tooLong) { E->kind = BFQ_PAIRS_E_TOO_LONG; return false; }
    return true;
}
// record i of an indexed text to dst: its bytes, and the LF the text's last line lacked
inline u64 bfq_pairs_put(u8 *dst, const u8 *t, u64 len, const bfq_pairs_index &I, u64 i)
{
    const u64 s = I.hs[i], n = I.hs[i + 1] - s, have = s + n <= len ? n : len - s;
    memcpy(dst, t + s, (size_t)have);
    if (have < n) dst[have] = 10;
    return n;
}

// The host form of the split: the same steps by one thread.  out[k] of cap[k] bytes (measure: not touched).  Returns 0;
// 2 = refused (*X); 3 = a cap below its length (S->out_len: the lengths).  Nothing is written unless 0 is returned.
inline int bfq_pairs_split_host(const u8 *t, u64 len, const bfq_pairs_opts &O, u8 *const out[3], const uint64_t cap[3], bool measure, bfq_pairs_stats *S,
                                u64 nReads[3], bfq_pairs_err *X)
{
    *S = bfq_pairs_stats{};
    *X = bfq_pairs_err{};
    nReads[0] = nReads[1] = nReads[2] = 0;
    if (!bfq_pairs_gzip_ok(t, len, 0, 0, X)) return 2;
    bfq_pairs_index I;
    if (!bfq_pairs_parse(t, len, &I, X)) return 2;
    const u64 N = I.N;
    std::vector<u8> role(N);
    if (!O.orphans) {
        if (N & 1) { X->kind = BFQ_PAIRS_E_ODD; X->n = N; return 2; }
        for (u64 k = 0; k < N / 2; k++) {
            if (O.check_names && !bfq_pairs_same(t, I.hs[2 * k], I.hl[2 * k], t, I.hs[2 * k + 1], I.hl[2 * k + 1], O.mate_suffix)) {
                X->kind = BFQ_PAIRS_E_NAMES; X->n = k;
                return 2;
            }
            role[2 * k] = 1; role[2 * k + 1] = 2;
        }
    } else {
        // b[i]: a run starts at record i; the run start of i: the largest j <= i with b[j] (an inclusive max-scan of b[i] ? i : 0)
        std::vector<u64> start(N + 1);
        u64 run = 0;
        for (u64 i = 0; i < N; i++) {
            const bool b = i == 0 || !bfq_pairs_same(t, I.hs[i - 1], I.hl[i - 1], t, I.hs[i], I.hl[i], O.mate_suffix);
            if (b) run = i;
            start[i] = run;
        }
        start[N] = N;
        for (u64 i = 0; i < N; i++) role[i] = (u8)bfq_pairs_role(i, start[i], start[i + 1] == i + 1);
    }
    u64 at[3] = {0, 0, 0};
    for (u64 i = 0; i < N; i++) { at[role[i]] += I.hs[i + 1] - I.hs[i]; nReads[role[i]]++; }
    S->records = N; S->pairs = nReads[1]; S->singles = nReads[0];
    for (int k = 0; k < 3; k++) S->out_len[k] = at[k];
    if (measure) return 0;
    for (int k = 0; k < 3; k++)
        if (cap[k] < at[k]) return 3;
    at[0] = at[1] = at[2] = 0;
    for (u64 i = 0; i < N; i++) at[role[i]] += bfq_pairs_put(out[role[i]] + at[role[i]], t, len, I, i);
    return 0;
}

// The host form of the merge.  text[k] (nullptr: absent).  S->out_len[0]: the length of the interleaved text.
inline int bfq_pairs_merge_host(const u8 *const text[3], const uint64_t textLen[3], const bfq_pairs_opts &O, u8 *out, u64 cap, bool measure, bfq_pairs_stats *S,
                                u64 nReads[3], bfq_pairs_err *X)
{
    *S = bfq_pairs_stats{};
    *X = bfq_pairs_err{};
    nReads[0] = nReads[1] = nReads[2] = 0;
    u64 len[3];
    for (u32 k = 0; k < 3; k++) {
        len[k] = text[k] ? textLen[k] : 0;
        if (!bfq_pairs_gzip_ok(text[k], len[k], 1, k, X)) return 2;
    }
    bfq_pairs_index I[3];
    for (u32 k = 0; k < 3; k++)
        if (!bfq_pairs_parse(text[k], len[k], &I[k], X)) return 2;
    if (I[1].N != I[2].N) { X->kind = BFQ_PAIRS_E_COUNTS; X->n = I[1].N; X->m = I[2].N; return 2; }
    const u64 P = I[1].N;
    if (O.check_names)
        for (u64 k = 0; k < P; k++)
            if (!bfq_pairs_same(text[1], I[1].hs[k], I[1].hl[k], text[2], I[2].hs[k], I[2].hl[k], O.mate_suffix)) {
                X->kind = BFQ_PAIRS_E_NAMES; X->merge = 1; X->n = k;
                return 2;
            }
    const u64 total = I[0].tl + I[1].tl + I[2].tl;
    S->records = 2 * P + I[0].N; S->pairs = P; S->singles = I[0].N; S->out_len[0] = total;
    nReads[0] = I[0].N; nReads[1] = nReads[2] = P;
    if (measure) return 0;
    if (cap < total) return 3;
    u64 at = 0;
    for (u64 k = 0; k < P; k++) {
        at += bfq_pairs_put(out + at, text[1], len[1], I[1], k);
        at += bfq_pairs_put(out + at, text[2], len[2], I[2], k);
    }
    for (u64 i = 0; i < I[0].N; i++) at += bfq_pairs_put(out + at, text[0], len[0], I[0], i);
    return 0;
}

// ---------------------------------------------------------------- repair
inline void bfq_repair_defaults(bfq_repair_opts *o) { o->mate_suffix = 1; o->hash_bits = 40; o->seed = 0; o->reserved[0] = o->reserved[1] = 0; }
inline bool bfq_repair_resolve(const bfq_repair_opts *in, bfq_repair_opts *O, bfq_pairs_err *E)
{
    bfq_repair_defaults(O);
    if (in) *O = *in;
    E->merge = 2;
    if (O->reserved[0] || O->reserved[1]) { E->kind = BFQ_PAIRS_E_RESERVED; return false; }
    if (O->hash_bits < 1 || O->hash_bits > 40) { E->kind = BFQ_PAIRS_E_HASH_BITS; return false; }
    return true;
}
// the text a global record number lies in (the order of the numbering: 1, 2, 0) and its number there
inline u32 bfq_repair_text_of(u64 g, const u64 n[3], u64 *i)
{
    if (g < n[1]) { *i = g; return 1; }
    if (g < n[1] + n[2]) { *i = g - n[1]; return 2; }
    *i = g - n[1] - n[2];
    return 0;
}

// The host form of the repair: the steps of the kernels by one thread.  out[k] of cap[k] bytes (measure: not touched).  Returns
// 0; 2 = refused (*X); 3 = a cap below its length (S->out_len: the lengths).  Nothing is written unless 0 is returned.
inline int bfq_pairs_repair_host(const u8 *const text[3], const uint64_t textLen[3], const bfq_repair_opts &O, u8 *const out[3], const uint64_t cap[3],
                                 bool measure, bfq_repair_stats *S, u64 nReads[3], bfq_pairs_err *X)
{
    *S = bfq_repair_stats{};
    *X = bfq_pairs_err{};
    X->merge = 2;
    nReads[0] = nReads[1] = nReads[2] = 0;
    u64 len[3];
    for (u32 k = 0; k < 3; k++) {
        len[k] = text[k] ? textLen[k] : 0;
        if (!bfq_pairs_gzip_ok(text[k], len[k], 2, k, X)) return 2;
    }
    bfq_pairs_index I[3];
    for (u32 k = 0; k < 3; k++)
        if (!bfq_pairs_parse(text[k], len[k], &I[k], X)) return 2;
    const u64 n[3] = {I[0].N, I[1].N, I[2].N}, N = n[0] + n[1] + n[2];
    // step 1: key, hint and hash of every record, in global order
    struct Rec { u64 h, ks, kl, size; u32 src, hint; u64 i; };
    std::vector<Rec> R(N);
    std::vector<u64> order(N);
    for (u64 g = 0; g < N; g++) {
        Rec &r = R[g];
        r.src = bfq_repair_text_of(g, n, &r.i);
        const u8 *t = text[r.src];
        const bfq_pairs_index &J = I[r.src];
        bfq_pairs_key(t, J.hs[r.i], J.hl[r.i], O.mate_suffix, &r.ks, &r.kl);
        r.hint = bfq_repair_hint(t, J.hs[r.i], J.hl[r.i], r.src, r.ks, r.kl);
        r.h = bfq_repair_hash(t + r.ks, r.kl, O.seed);
        r.size = J.hs[r.i + 1] - J.hs[r.i];
        order[g] = g;
    }
    // step 2: the stable sort on the sort key
    std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) { return bfq_repair_sort_key(R[a].h, O.hash_bits) < bfq_repair_sort_key(R[b].h, O.hash_bits); });
    // step 3: the runs; their lengths are checked before any of them is walked
    std::vector<u64> start(N + 1);
    u64 firstBad = BFQ_PAIRS_NONE;
    for (u64 p = 0, run = 0; p < N; p++) {
        if (p == 0 || bfq_repair_sort_key(R[order[p - 1]].h, O.hash_bits) != bfq_repair_sort_key(R[order[p]].h, O.hash_bits)) run = p;
        start[p] = run;
    }
    start[N] = N;
    for (u64 p = 0; p < N; p++) {
        if (start[p + 1] != p + 1) continue;                    // p ends a run
        const u64 r = p + 1 - start[p];
        if (r > S->max_run) S->max_run = r;
        if (r > BFQ_REPAIR_RUN_MAX && order[start[p]] < firstBad) firstBad = order[start[p]];
    }
    if (firstBad != BFQ_PAIRS_NONE) {
        X->kind = BFQ_PAIRS_E_RUN;
        X->k = bfq_repair_text_of(firstBad, n, &X->n);
        *S = bfq_repair_stats{};
        return 2;
    }
    auto same = [&](const Rec &a, const Rec &b) { return a.h == b.h && a.kl == b.kl && !memcmp(text[a.src] + a.ks, text[b.src] + b.ks, (size_t)a.kl); };
    std::vector<u8> role(N);
    std::vector<u64> anchor(N);
    for (u64 p = 0; p < N; p++) {
        const Rec &me = R[order[p]];
        u64 e = start[p];
        u32 before[3] = {0, 0, 0}, total[3] = {0, 0, 0};
        bool mixed = false;
        for (; e < N && start[e] == start[p]; e++) {
            const Rec &o = R[order[e]];
            if (!same(me, o)) { mixed = true; continue; }
            total[o.hint]++;
            if (e < p) before[o.hint]++;
        }
        u32 mate = 0;
        const u32 r = bfq_repair_role(me.hint, before, total, &mate);
        role[order[p]] = (u8)r;
        if (r) {                                                // the anchor: the mate-th record of list L1 (hint 0: L0) of the group
            const u32 list = me.hint ? 1u : 0u;
            u32 seen = 0;
            for (u64 q = start[p]; q < e; q++) {
                const Rec &o = R[order[q]];
                if (o.hint != list || !same(me, o)) continue;
                if (seen++ == mate) { anchor[order[p]] = order[q]; break; }
            }
        }
        if (p == start[p] && mixed) S->mixed_runs++;
        if (before[0] + before[1] + before[2] == 0 && total[0] + total[1] + total[2] > 2) S->dup_groups++;
    }
    // step 4: ranks in global order, sizes, offsets
    std::vector<u64> rank1(N), rank0(N), off[3];
    u64 P = 0, Z = 0;
    for (u64 g = 0; g < N; g++) { rank1[g] = P; rank0[g] = Z; P += role[g] == 1; Z += role[g] == 0; }
    off[0].assign(Z + 1, 0); off[1].assign(P + 1, 0); off[2].assign(P + 1, 0);
    std::vector<u64> slot(N);
    for (u64 g = 0; g < N; g++) {
        slot[g] = role[g] ? rank1[anchor[g]] : rank0[g];
        off[role[g]][slot[g]] = R[g].size;
    }
    u64 at[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++)
        for (u64 j = 0; j < off[k].size(); j++) { const u64 s = off[k][j]; off[k][j] = at[k]; at[k] += s; }
    S->records = N; S->pairs = P; S->singles = Z;
    for (int k = 0; k < 3; k++) { S->out_len[k] = at[k]; S->n_in[k] = n[k]; }
    nReads[0] = Z; nReads[1] = nReads[2] = P;
    if (measure) return 0;
    for (int k = 0; k < 3; k++)
        if (cap[k] < at[k]) return 3;
    // step 5: every record moved once
    for (u64 g = 0; g < N; g++) bfq_pairs_put(out[role[g]] + off[role[g]][slot[g]], text[R[g].src], len[R[g].src], I[R[g].src], R[g].i);
    return 0;
}
