// bfq_dedup.h -- exact duplicate removal of FASTQ reads and pairs, host and device: the definition, the hash of a unit, the
// messages and the host form.  Plain C++, shared by the kernels (k_dedup.hip), the host side (bfq_dedup.hip) and the
// sanitizer program (tests/cxx/test_dedup.cpp).
//
// This project's definition (bfq_fastq_dedup*, include/bfqzip_hip.h):
//   The texts: text[0] holds mate 1 or the single-end file, text[1] mate 2 (nullptr: single-end).  Plain FASTQ as
//     bfq_fastq_interleave reads it, four lines per record; a record is its four lines byte for byte, and a text whose last line
//     lacks its LF gets one.  Refusals keep the words of bfq_pairs.h -- "FASTQ: number of lines is not a multiple of 4", "FASTQ:
//     len(DNA) != len(QS) in a record" (BFQ_E_ARG), "read longer than BFQ_MAX_READ_LEN" (BFQ_E_TOO_LONG) --, looked for in that
//     order, text by text; a text that begins with 1f 8b: "FASTQ dedup: text <k> is compressed (it begins with 1f 8b): inflate
//     the text first".  Paired: the k-th records of the two texts are one unit; "FASTQ dedup: text 0 holds <n> reads, text 1
//     holds <m>" where the counts differ.  The global number g of a unit is its record index.
//   Key of a unit: the bytes of the sequence line without the LF and without one trailing CR; paired: the ordered pair (key
//     of mate 1, key of mate 2), lengths included.  Bytes compare as they are.  Header, '+' line and qualities: no part of it.
//   Group: all units of the call with equal keys.  Kept: keep = 0, the smallest g of the group; keep = 1, the largest score
//     and among equals the smallest g; score = sum of max(byte - 33, 0) over the quality bytes of the unit (both mates; the
//     quality line without its LF and one trailing CR), mod 2^64.
//   Outputs: out[m] = the kept units' records of text m in increasing g, dup[m] = all others' in increasing g.  A function of
//     the texts and keep alone.
//   Hash of a unit: single-end h = H(seq) = bfq_repair_hash(seq, L, seed) (bfq_pairs.h: 8-byte chunks, a commutative sum of
//     fmix64, finished with the length and the seed); paired h = fmix64(H(seq1) ^ fmix64(H(seq2) + GOLD)): not commutative,
//     (x, y) and (y, x) hash apart.  The sort key: the top hash_bits bits of h.
//   How: the units are sorted by the sort key (stable: a run of equal sort keys is in global order), and every run is cut into
//     groups in rounds.  A run has a current head, at first its first position.  In a round every unresolved position compares
//     its unit with the head's -- full hash, lengths, bytes --, joins the head's group if they are equal, and else proposes
//     itself as the next head; the smallest proposal wins.  Round k resolves the k-th different key of every run, in the order
//     of the keys' first units; the head of a group is therefore its smallest g.  The number of rounds is the largest number of
//     different keys in a run (`rounds`); a run that is unresolved after BFQ_DEDUP_KINDS_MAX rounds is refused, "FASTQ dedup:
//     more than 1024 different sequences share a hash (the first: record <g>)": <g> is the smallest global number in such a
//     run.  The number of EQUAL units in a run is not bounded.
//   Statistics: see include/bfqzip_hip.h; mixed_runs (runs with more than one key), max_run and rounds depend on hash_bits and
//     the seed, nothing else does.
//   All refusals but the too-long read are BFQ_E_ARG.  In every form a refusal writes nothing.
// Out of scope: a read and its reverse complement as equal; near-duplicates; optical duplicates; name checks between the
// mates (bfq_fastq_interleave_measure does them); interleaved input; BGZF parts inside these calls; multiplicities in headers.
#pragma once
#include "bfq_pairs.h"

enum {
    BFQ_DEDUP_OK = 0,
    BFQ_DEDUP_E_RESERVED,    // bfq_dedup_opts.reserved != 0
    BFQ_DEDUP_E_KEEP,        // keep > 1
    BFQ_DEDUP_E_HASH_BITS,   // hash_bits outside 1..40
    BFQ_DEDUP_E_GZIP,        // a text begins with 1f 8b
    BFQ_DEDUP_E_LINES,       // lines not a multiple of 4
    BFQ_DEDUP_E_FASTQ,       // len(DNA) != len(QS)
    BFQ_DEDUP_E_TOO_LONG,    // a read above BFQ_MAX_READ_LEN
    BFQ_DEDUP_E_COUNTS,      // the mates' record counts differ
    BFQ_DEDUP_E_KINDS,       // more than BFQ_DEDUP_KINDS_MAX different keys in a run of equal sort keys
    BFQ_DEDUP_E_CAP          // an output below its text
};
#define BFQ_DEDUP_KINDS_MAX 1024u
struct bfq_dedup_err { u32 kind = 0, k = 0; u64 n = 0, m = 0; };
inline int bfq_dedup_code(const bfq_dedup_err &E) { return E.kind == BFQ_DEDUP_E_TOO_LONG ? BFQ_E_TOO_LONG : BFQ_E_ARG; }
inline std::string bfq_dedup_message(const bfq_dedup_err &E)
{
    char b[200];
    switch (E.kind) {
    case BFQ_DEDUP_E_RESERVED: return "bfq_dedup_opts.reserved: must be 0";
    case BFQ_DEDUP_E_KEEP: return "bfq_dedup_opts.keep: must be 0 or 1";
    case BFQ_DEDUP_E_HASH_BITS: return "bfq_dedup_opts.hash_bits: must be 1..40";
    case BFQ_DEDUP_E_GZIP: snprintf(b, sizeof b, "FASTQ dedup: text %u is compressed (it begins with 1f 8b): inflate the text first", E.k); return b;
    case BFQ_DEDUP_E_LINES: return "FASTQ: number of lines is not a multiple of 4";
    case BFQ_DEDUP_E_FASTQ: return "FASTQ: len(DNA) != len(QS) in a record";
    case BFQ_DEDUP_E_TOO_LONG: return "read longer than BFQ_MAX_READ_LEN";
    case BFQ_DEDUP_E_COUNTS: snprintf(b, sizeof b, "FASTQ dedup: text 0 holds %llu reads, text 1 holds %llu", E.n, E.m); return b;
    case BFQ_DEDUP_E_KINDS:
        snprintf(b, sizeof b, "FASTQ dedup: more than %u different sequences share a hash (the first: record %llu)", BFQ_DEDUP_KINDS_MAX, E.n);
        return b;
    case BFQ_DEDUP_E_CAP: return "output buffer smaller than the text it receives";
    default: return "ok";
    }
}

// ---------------------------------------------------------------- the rule, for one lane
BFQ_HD u64 bfq_dedup_pair_hash(u64 h1, u64 h2) { return bfq_fmix64(h1 ^ bfq_fmix64(h2 + BFQ_REPAIR_GOLD)); }
BFQ_HD u64 bfq_dedup_qual(u8 q) { return q > 33 ? (u64)(q - 33) : 0; }
BFQ_HD u32 bfq_dedup_level(u64 size)                               // floor(log2(size)) for size >= 1, at most 31
{
    u32 l = 0;
    while (l < 31 && (size >> (l + 1))) l++;
    return l;
}

// ---------------------------------------------------------------- host side
inline void bfq_dedup_defaults(bfq_dedup_opts *o) { o->keep = 0; o->hash_bits = 40; o->seed = 0; o->reserved[0] = o->reserved[1] = 0; }
inline bool bfq_dedup_resolve(const bfq_dedup_opts *in, bfq_dedup_opts *O, bfq_dedup_err *E)
{
    bfq_dedup_defaults(O);
    if (in) *O = *in;
    if (O->reserved[0] || O->reserved[1]) { E->kind = BFQ_DEDUP_E_RESERVED; return false; }
    if (O->keep > 1) { E->kind = BFQ_DEDUP_E_KEEP; return false; }
    if (O->hash_bits < 1 || O->hash_bits > 40) { E->kind = BFQ_DEDUP_E_HASH_BITS; return false; }
    return true;
}
inline bool bfq_dedup_gzip_ok(const u8 first[2], u64 len, u32 k, bfq_dedup_err *E)
{
    if (len < 2 || first[0] != 0x1F || first[1] != 0x8B) return true;
    E->kind = BFQ_DEDUP_E_GZIP; E->k = k;
    return false;
}

// The records of a text as one host thread finds them: where they start (rs[N] = the text's length with its final LF), and
// where the sequence and the quality line start and how long they are (CR dropped).
struct bfq_dedup_index { std::vector<u64> rs, ss, qs; std::vector<u32> sl; u64 N = 0, tl = 0; };
inline bool bfq_dedup_parse(const u8 *t, u64 len, bfq_dedup_index *I, bfq_dedup_err *E)
{
    std::vector<u64> le;
    for (u64 p = 0; p < len; p++)
        if (t[p] == 10) le.push_back(p);
    if (len && t[len - 1] != 10) le.push_back(len);
    if (le.size() % 4) { E->kind = BFQ_DEDUP_E_LINES; return false; }
    const u64 N = le.size() / 4;
    bool badLen = false, tooLong = false;
    I->rs.assign(N + 1, 0); I->ss.assign(N, 0); I->qs.assign(N, 0); I->sl.assign(N, 0);
    for (u64 i = 0; i < N; i++) {
        u64 s[4], e[4];
        for (int k = 0; k < 4; k++) {
            const u64 li = 4 * i + k;
            s[k] = li ? le[li - 1] + 1 : 0;
            e[k] = le[li];
            if (k && e[k] > s[k] && t[e[k] - 1] == 13) e[k]--;
        }
        const u64 l = e[1] - s[1];
        I->rs[i] = s[0]; I->ss[i] = s[1]; I->qs[i] = s[3];
        if (e[3] - s[3] != l) badLen = true;
        if (l > BFQ_MAX_READ_LEN) tooLong = true; else I->sl[i] = (u32)l;
    }
    I->N = N;
    I->tl = len + (len && t[len - 1] != 10 ? 1 : 0);
    I->rs[N] = I->tl;
    if (badLen) { E->kind = BFQ_DEDUP_E_FASTQ; return false; }
    if (tooLong) { E->kind = BFQ_DEDUP_E_TOO_LONG; return false; }
    return true;
}
// record i of an indexed text to dst: its bytes, and the LF the text's last line lacked
inline u64 bfq_dedup_put(u8 *dst, const u8 *t, u64 len, const bfq_dedup_index &I, u64 i)
{
    const u64 s = I.rs[i], n = I.rs[i + 1] - s, have = s + n <= len ? n : len - s;
    memcpy(dst, t + s, (size_t)have);
    if (have < n) dst[have] = 10;
    return n;
}

// The host form: the steps of the kernels by one thread.  out[m] of outCap[m] bytes; dup == nullptr: the removed records are
// counted and not written (measure: nothing is touched).  Returns 0; 2 = refused (*X); 3 = a cap below its length (S->out_len,
// S->dup_len: the lengths).  Nothing is written unless 0 is returned.
inline int bfq_dedup_host(const u8 *const text[2], const uint64_t textLen[2], const bfq_dedup_opts &O, u8 *const out[2], const uint64_t outCap[2],
                          u8 *const dup[2], const uint64_t dupCap[2], bool measure, bfq_dedup_stats *S, bfq_dedup_err *X)
{
    *S = bfq_dedup_stats{};
    *X = bfq_dedup_err{};
    const u32 nt = text[1] ? 2 : 1;
    u64 len[2] = {0, 0};
    for (u32 k = 0; k < nt; k++) {
        len[k] = text[k] ? textLen[k] : 0;
        if (!bfq_dedup_gzip_ok(text[k], len[k], k, X)) return 2;
    }
    bfq_dedup_index I[2];
    for (u32 k = 0; k < nt; k++)
        if (!bfq_dedup_parse(text[k], len[k], &I[k], X)) return 2;
    if (nt == 2 && I[0].N != I[1].N) { X->kind = BFQ_DEDUP_E_COUNTS; X->n = I[0].N; X->m = I[1].N; return 2; }
    const u64 N = I[0].N;
    // step 1: hash and score of every unit
    std::vector<u64> h(N), score(N), order(N);
    for (u64 g = 0; g < N; g++) {
        u64 hv = 0, sc = 0;
        for (u32 k = 0; k < nt; k++) {
            const u64 hk = bfq_repair_hash(text[k] + I[k].ss[g], I[k].sl[g], O.seed);
            hv = k ? bfq_dedup_pair_hash(hv, hk) : hk;
            for (u32 j = 0; j < I[k].sl[g]; j++) sc += bfq_dedup_qual(text[k][I[k].qs[g] + j]);
        }
        h[g] = hv; score[g] = sc; order[g] = g;
    }
    // step 2: the stable sort on the sort key, the runs
    std::stable_sort(order.begin(), order.end(), [&](u64 a, u64 b) { return bfq_repair_sort_key(h[a], O.hash_bits) < bfq_repair_sort_key(h[b], O.hash_bits); });
    auto same = [&](u64 a, u64 b) {
        if (h[a] != h[b]) return false;
        for (u32 k = 0; k < nt; k++)
            if (I[k].sl[a] != I[k].sl[b] || memcmp(text[k] + I[k].ss[a], text[k] + I[k].ss[b], I[k].sl[a])) return false;
        return true;
    };
    // step 3: the groups of every run.  heads: the positions that were a head, in the order of their rounds; rep[p]: the head p joined
    std::vector<u64> rep(N), heads;
    u64 firstBad = BFQ_PAIRS_NONE;
    for (u64 s = 0, e; s < N; s = e) {
        for (e = s + 1; e < N && bfq_repair_sort_key(h[order[e]], O.hash_bits) == bfq_repair_sort_key(h[order[s]], O.hash_bits); e++) {}
        heads.clear();
        bool bad = false;
        for (u64 p = s; p < e && !bad; p++) {
            size_t j = 0;
            while (j < heads.size() && !same(order[heads[j]], order[p])) j++;
            if (j == heads.size()) {
                if (heads.size() == BFQ_DEDUP_KINDS_MAX) { bad = true; break; }
                heads.push_back(p);
            }
            rep[p] = heads[j];
        }
        if (bad && order[s] < firstBad) firstBad = order[s];
        if (e - s > S->max_run) S->max_run = e - s;
        if (heads.size() > 1) S->mixed_runs++;
        if (heads.size() > S->rounds) S->rounds = heads.size();
    }
    if (firstBad != BFQ_PAIRS_NONE) { *S = bfq_dedup_stats{}; X->kind = BFQ_DEDUP_E_KINDS; X->n = firstBad; return 2; }
    // step 4: sizes and winners per group (a group is named by its head's position)
    std::vector<u64> size(N, 0), best(N, 0), win(N, BFQ_PAIRS_NONE);
    for (u64 p = 0; p < N; p++) { size[rep[p]]++; if (score[order[p]] > best[rep[p]]) best[rep[p]] = score[order[p]]; }
    for (u64 p = 0; p < N; p++)
        if (score[order[p]] == best[rep[p]] && order[p] < win[rep[p]]) win[rep[p]] = order[p];
    std::vector<u8> kept(N, 0);
    for (u64 p = 0; p < N; p++) {
        const u64 g = order[p];
        kept[g] = O.keep ? win[rep[p]] == g : rep[p] == p;
        if (rep[p] != p) continue;                                  // the heads: one per group, its smallest g
        const u64 n = size[p];
        const u32 l = bfq_dedup_level(n);
        S->level_groups[l]++; S->level_units[l] += n;
        if (n >= 2) S->dup_groups++;
        if (n > S->max_group || (n == S->max_group && g < S->max_group_first)) { S->max_group = n; S->max_group_first = g; }
    }
    // step 5: lengths, then every record moved once
    S->units = N;
    for (u64 g = 0; g < N; g++) {
        S->kept += kept[g];
        for (u32 k = 0; k < nt; k++) (kept[g] ? S->out_len : S->dup_len)[k] += I[k].rs[g + 1] - I[k].rs[g];
    }
    S->removed = N - S->kept;
    if (measure) return 0;
    for (u32 k = 0; k < nt; k++)
        if (outCap[k] < S->out_len[k] || (dup && dupCap[k] < S->dup_len[k])) return 3;
    u64 at[2] = {0, 0}, dat[2] = {0, 0};
    for (u64 g = 0; g < N; g++)
        for (u32 k = 0; k < nt; k++) {
            if (kept[g]) at[k] += bfq_dedup_put(out[k] + at[k], text[k], len[k], I[k], g);
            else if (dup) dat[k] += bfq_dedup_put(dup[k] + dat[k], text[k], len[k], I[k], g);
        }
    return 0;
}
