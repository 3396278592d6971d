// bfq_bam_patch.h -- FASTQ text back into the BAM records it came from, host and device: the definition, the checking
// walk, the patching walk, the messages and the host form.  Plain C++ on top of bfq_bam.h (the format, the chain), shared by
// the kernels (k_bam_patch.hip), the host side (bfq_bam_patch.hip) and the sanitizer program (tests/cxx/test_bam_patch.cpp).
//
// "This BAM, with the reads of these FASTQ texts in it."  Inputs: the inflated stream, bfq_bam_opts with the meaning they
// have for bfq_bam_to_fastq, up to three plain FASTQ texts text[k].
//   Which record meets which read: the i-th kept record of output k -- exactly the record bfq_bam_to_fastq with the same
//     options writes as read i of output k -- meets read i of text[k] (lines 4i + 1 and 4i + 3).  An absent text[k] leaves
//     the records of output k as they are; records excluded by exclude_flags are never touched.
//   The text: plain FASTQ (a text that begins with 1f 8b is refused by name); CR before LF is stripped from every line; a
//     last line without its LF counts.  The header line is used only with check_names.
//   Bases: case-insensitive over =ACMGRSVTWYHKDBN, each letter to its nibble; any other byte becomes 15 (N) and is counted
//     (unknown_bases).  Flag 0x10: text base i goes to record position l_seq - 1 - i as its complement (the complement of a
//     nibble is its four bits in reverse order): the inverse of bfq_bam_base(., true).  The unused low nibble of an
//     odd-length sequence keeps what the record holds.
//   Qualities: (char - 33) mod 256, reversed under 0x10.  Two keep rules make the identity patch exact:
//     1 the record's qualities are present, the text says 93 ('~') and the record holds a value above 93: the record's
//       value stays (kept_high_quals);
//     2 the record's qualities are absent (first byte 0xFF) and every quality of the read equals default_qual + 33: they
//       stay absent (kept_absent counts the records).  Otherwise all l_seq values are written as the text has them.
//   Refusals (nothing is written): a text that is compressed; a line count that is no multiple of 4; a number of reads
//     other than the number of kept records of its output; and, found by the checking walk, which reports the offending
//     record that comes first in the file: len(DNA) != len(QS); a read whose length is not l_seq; with check_names a
//     name that differs from read_name.  The text's name is the bytes behind '@' up to the first blank (space or tab), less
//     the "/1" or "/2" that mate_suffix adds on the way in; a line that does not begin with '@' has no name.
//   Counts: records (of the file), patched[k] (records that met a read of text k), skipped (all others: excluded, or of an
//     absent text), reversed (patched records with 0x10), reads_changed (patched records of which a stored value changed),
//     bases_changed and quals_changed (positions whose stored value differs from before), unknown_bases, kept_high_quals,
//     kept_absent.  They are taken per piece of the chain and summed in chain order; none depends on the piece size.
// Every record keeps its size, so the patch works in place on a copy of the stream; a wave (or the one host thread)
// writes only inside the SEQ and QUAL fields of the kept records of its own chain piece.
#pragma once
#include "bfq_bam.h"

enum {
    BFQ_BAMP_OK = 0,
    BFQ_BAMP_E_GZIP,         // a text begins with 1f 8b
    BFQ_BAMP_E_LINES,        // lines not a multiple of 4
    BFQ_BAMP_E_COUNT,        // reads of text k != kept records of output k
    BFQ_BAMP_E_FASTQ,        // len(DNA) != len(QS)
    BFQ_BAMP_E_LEN,          // bases of the read != l_seq
    BFQ_BAMP_E_NAME          // check_names: the names differ
};
// what is refused: text k, its read i, record rec of the file at byte off; n / m: the two numbers the message names
struct bfq_bamp_err { u32 kind = 0, k = 0; u64 i = 0, rec = 0, off = 0, n = 0, m = 0; };
inline std::string bfq_bamp_message(const bfq_bamp_err &E)
{
    char b[320];
    switch (E.kind) {
    case BFQ_BAMP_E_GZIP: snprintf(b, sizeof b, "BAM patch: text %u is compressed (it begins with 1f 8b): inflate the text first", E.k); break;
    case BFQ_BAMP_E_LINES: snprintf(b, sizeof b, "FASTQ: number of lines is not a multiple of 4"); break;
    case BFQ_BAMP_E_COUNT: snprintf(b, sizeof b, "BAM patch: text %u holds %llu reads, the BAM file holds %llu records for it", E.k, E.n, E.m); break;
    case BFQ_BAMP_E_FASTQ: snprintf(b, sizeof b, "FASTQ: len(DNA) != len(QS) in a record"); break;
    case BFQ_BAMP_E_LEN: snprintf(b, sizeof b, "BAM patch: text %u read %llu: %llu bases, record %llu at byte %llu holds %llu", E.k, E.i, E.n, E.rec, E.off, E.m); break;
    case BFQ_BAMP_E_NAME: snprintf(b, sizeof b, "BAM patch: text %u read %llu: the name differs from that of record %llu at byte %llu", E.k, E.i, E.rec, E.off); break;
    default: snprintf(b, sizeof b, "ok");
    }
    return b;
}

// the texts of a call: text[k] == nullptr: absent.  lineEnd[k][l]: where line l ends (its LF, or len[k] for a last line
// without one), as bfq_line_index gives it.
struct bfq_bam_texts { const u8 *text[3]; const u64 *lineEnd[3]; u64 len[3]; };
// the counts of one chain piece
struct bfq_bamp_cnt { u64 readsChanged, basesChanged, qualsChanged, unknown, keptHigh, keptAbsent, reversed, pad; };
// How the nl lanes of a walk agree: the host's one lane with itself.  (The device's wave64: k_bam_patch.hip.)
struct bfq_bamp_alone {
    static BFQ_HD bool all(bool v) { return v; }
    static BFQ_HD bool any(bool v) { return v; }
};

// line l of a text without its CR: [*s, *e)
BFQ_HD void bfq_bamp_line(const u8 *t, const u64 *lineEnd, u64 l, u64 *s, u64 *e)
{
    *s = l ? lineEnd[l - 1] + 1 : 0;
    *e = lineEnd[l];
    if (*e > *s && t[*e - 1] == 13) (*e)--;
}
// the nibble of a base of the text (rev: of its complement); *unknown: the byte is no letter of the alphabet
BFQ_HD u32 bfq_bamp_nibble(u8 ch, bool rev, u32 *unknown)
{
    u32 n = 15;
    *unknown = 0;
    switch (ch == '=' ? ch : (u8)(ch & 0xDFu)) {
    case '=': n = 0; break;
    case 'A': n = 1; break;  case 'C': n = 2; break;  case 'M': n = 3; break;  case 'G': n = 4; break;  case 'R': n = 5; break;
    case 'S': n = 6; break;  case 'V': n = 7; break;  case 'T': n = 8; break;  case 'W': n = 9; break;  case 'Y': n = 10; break;
    case 'H': n = 11; break; case 'K': n = 12; break; case 'D': n = 13; break; case 'B': n = 14; break; case 'N': n = 15; break;
    default: *unknown = 1;
    }
    return rev ? ((n & 1u) << 3) | ((n & 2u) << 1) | ((n & 4u) >> 1) | ((n & 8u) >> 3) : n;
}

// Read i of text k against the record at s[o] (checked: R), by nl lanes: 0, or why it is refused -- the same in every lane.
// *bases: the length of its sequence line.
template <class W> BFQ_HD u32 bfq_bamp_check_rec(const u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_opts &O, const bfq_bam_texts &T, u32 k, u64 i, u32 lane,
                                                 u32 nl, u64 *bases)
{
    const u8 *t = T.text[k];
    u64 s1, e1, s3, e3;
    bfq_bamp_line(t, T.lineEnd[k], 4 * i + 1, &s1, &e1);
    bfq_bamp_line(t, T.lineEnd[k], 4 * i + 3, &s3, &e3);
    *bases = e1 - s1;
    if (e3 - s3 != e1 - s1) return BFQ_BAMP_E_FASTQ;
    if (e1 - s1 != R.lseq) return BFQ_BAMP_E_LEN;
    if (!O.check_names) return BFQ_BAMP_OK;
    u64 s0, e0;
    bfq_bamp_line(t, T.lineEnd[k], 4 * i, &s0, &e0);
    const u8 *name = s + o + 36;
    const u32 nameLen = R.ln - 1, mate = O.mate_suffix ? bfq_bam_mate(R.flag) : 0;
    const u64 need = 1ull + nameLen + (mate ? 2 : 0);
    bool same = e0 - s0 >= need && t[s0] == '@' && (e0 - s0 == need || t[s0 + need] == ' ' || t[s0 + need] == '\t');
    if (same && mate) same = t[s0 + need - 2] == '/' && t[s0 + need - 1] == (u8)('0' + mate);
    if (same)
        for (u32 j = lane; j < nameLen; j += nl) same = same && t[s0 + 1 + j] == name[j] && name[j] != ' ' && name[j] != '\t';
    return W::all(same) ? BFQ_BAMP_OK : BFQ_BAMP_E_NAME;
}

// The checking walk of a chain piece, by nl lanes: BFQ_BAM_NONE, or the offset of its first record whose read is refused,
// with *E filled (rec: counted from the piece's first record; the caller adds the records in front of the piece).
template <class W> BFQ_HD u64 bfq_bam_patch_check(const u8 *s, u64 len, const bfq_bam_job &J, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T, u32 lane, u32 nl,
                                                  bfq_bamp_err *E)
{
    u64 idx[3] = {J.recBase[0], J.recBase[1], J.recBase[2]}, nrec = 0;
    for (u64 o = J.start; o < J.end; nrec++) {
        bfq_bam_rec R;
        if (bfq_bam_check(s, len, o, nref, false, &R)) break;       // (the count pass has passed every record of the chain)
        if (!(R.flag & O.exclude_flags)) {
            const u32 k = O.split ? bfq_bam_mate(R.flag) : 0;
            if (T.text[k]) {
                u64 bases = 0;
                const u32 why = bfq_bamp_check_rec<W>(s, o, R, O, T, k, idx[k], lane, nl, &bases);
                if (why) {
                    E->kind = why; E->k = k; E->i = idx[k]; E->rec = nrec; E->off = o; E->n = bases; E->m = R.lseq;
                    return o;
                }
            }
            idx[k]++;
        }
        o += 4ull + R.bs;
    }
    return BFQ_BAM_NONE;
}

// Read i of text k (checked) into the record at s[o], by nl lanes: a lane owns whole bytes of SEQ -- two bases, neighbouring
// bytes of the text -- and whole bytes of QUAL; lane b, b + nl, ... take byte b, b + nl, ... so the lanes' loads and stores
// are consecutive.  C: this lane's counts.
template <class W> BFQ_HD void bfq_bamp_patch_rec(u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_opts &O, const bfq_bam_texts &T, u32 k, u64 i, u32 lane, u32 nl,
                                                  bfq_bamp_cnt *C)
{
    const u8 *t = T.text[k];
    u64 s1, e1, s3, e3;
    bfq_bamp_line(t, T.lineEnd[k], 4 * i + 1, &s1, &e1);
    bfq_bamp_line(t, T.lineEnd[k], 4 * i + 3, &s3, &e3);
    u8 *seq = s + o + 36 + R.ln + 4ull * R.nc, *qual = seq + (R.lseq + 1) / 2;
    const u32 L = R.lseq;
    const bool rev = (R.flag & 0x10u) != 0;
    const bool absent = L && qual[0] == 0xFF;                       // (read by every lane before any lane stores a quality)
    bool changed = false;
    for (u32 b = lane; b < (L + 1) / 2; b += nl) {
        const u32 j = 2 * b, old = seq[b];
        u32 unk, hi = bfq_bamp_nibble(t[s1 + (rev ? L - 1 - j : j)], rev, &unk), lo = old & 15u;
        C->unknown += unk;
        if (j + 1 < L) {
            lo = bfq_bamp_nibble(t[s1 + (rev ? L - 2 - j : j + 1)], rev, &unk);
            C->unknown += unk;
        }
        C->basesChanged += ((old >> 4) != hi ? 1 : 0) + ((old & 15u) != lo ? 1 : 0);
        if (((hi << 4) | lo) != old) { seq[b] = (u8)((hi << 4) | lo); changed = true; }
    }
    bool keepAbsent = false;
    if (absent) {                                                   // (the same in every lane)
        bool mine = true;
        for (u32 j = lane; j < L; j += nl) mine = mine && t[s3 + j] == (u8)(O.default_qual + 33);
        keepAbsent = W::all(mine);
    }
    if (keepAbsent) C->keptAbsent += lane == 0 ? 1 : 0;
    else
        for (u32 j = lane; j < L; j += nl) {
            const u8 old = qual[j];
            u8 q = (u8)(t[s3 + (rev ? L - 1 - j : j)] - 33);
            if (!absent && q == BFQ_BAM_MAX_QUAL && old > BFQ_BAM_MAX_QUAL) { q = old; C->keptHigh++; }
            if (q != old) { qual[j] = q; C->qualsChanged++; changed = true; }
        }
    changed = W::any(changed);
    if (lane == 0) { C->readsChanged += changed ? 1 : 0; C->reversed += rev ? 1 : 0; }
}

// The patching walk of a chain piece, by nl lanes.  *C: this lane's counts of the piece (the caller sums the lanes).
template <class W> BFQ_HD void bfq_bam_patch_job(u8 *s, u64 len, const bfq_bam_job &J, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T, u32 lane, u32 nl,
                                                bfq_bamp_cnt *C)
{
    u64 idx[3] = {J.recBase[0], J.recBase[1], J.recBase[2]};
    for (u64 o = J.start; o < J.end;) {
        bfq_bam_rec R;
        if (bfq_bam_check(s, len, o, nref, false, &R)) break;       // (the count pass has passed every record of the chain)
        if (!(R.flag & O.exclude_flags)) {
            const u32 k = O.split ? bfq_bam_mate(R.flag) : 0;
            if (T.text[k]) bfq_bamp_patch_rec<W>(s, o, R, O, T, k, idx[k], lane, nl, C);
            idx[k]++;
        }
        o += 4ull + R.bs;
    }
}

// ---------------------------------------------------------------- host side
// the checks of a text as a whole, in the order both forms make them; false: *E
inline bool bfq_bamp_gzip_ok(const u8 first[2], u64 len, u32 k, bfq_bamp_err *E)
{
    if (len < 2 || first[0] != 0x1F || first[1] != 0x8B) return true;
    E->kind = BFQ_BAMP_E_GZIP; E->k = k;
    return false;
}
inline bool bfq_bamp_lines_ok(u64 nlines, u64 written, u32 k, bfq_bamp_err *E)
{
    if (nlines % 4) { E->kind = BFQ_BAMP_E_LINES; E->k = k; return false; }
    if (nlines / 4 != written) { E->kind = BFQ_BAMP_E_COUNT; E->k = k; E->n = nlines / 4; E->m = written; return false; }
    return true;
}
// the records in front of every piece of the chain
inline std::vector<u64> bfq_bamp_rec_bases(const std::vector<bfq_bam_piece> &P, const std::vector<bfq_bam_job> &jobs, u64 hdrEnd, u64 piece)
{
    std::vector<u64> base(jobs.size() + 1, 0);
    for (size_t j = 0; j < jobs.size(); j++) base[j + 1] = base[j] + P[(jobs[j].start - hdrEnd) / piece].nrec;
    return base;
}
// *PS from the chain's counts and the pieces' (in chain order)
inline void bfq_bamp_totals(const bfq_bam_stats &S, const bool present[3], u64 rawLen, const bfq_bamp_cnt *cnt, u64 nj, bfq_bam_patch_stats *PS)
{
    *PS = bfq_bam_patch_stats{};
    PS->records = S.records; PS->raw_len = rawLen; PS->pieces = S.pieces; PS->repaired = S.repaired;
    u64 met = 0;
    for (int k = 0; k < 3; k++) { PS->patched[k] = present[k] ? S.written[k] : 0; met += PS->patched[k]; }
    PS->skipped = S.records - met;
    for (u64 j = 0; j < nj; j++) {
        PS->reads_changed += cnt[j].readsChanged; PS->bases_changed += cnt[j].basesChanged; PS->quals_changed += cnt[j].qualsChanged;
        PS->unknown_bases += cnt[j].unknown; PS->kept_high_quals += cnt[j].keptHigh; PS->kept_absent += cnt[j].keptAbsent; PS->reversed += cnt[j].reversed;
    }
}

// The host form: the same steps by one thread.  s[0, len): the inflated stream; O: resolved options; text[k] (nullptr:
// absent) of textLen[k] bytes; out[0, cap): where the patched stream goes.  Returns 0; 1 = a damaged BAM (*E); 2 = a text
// refused (*X); 3 = cap < len.  Nothing is written unless 0 is returned.
inline int bfq_bam_patch_host_form(const u8 *s, u64 len, const bfq_bam_opts &O, const u8 *const text[3], const u64 textLen[3], u8 *out, u64 cap,
                                   bfq_bam_patch_stats *PS, bfq_bam_err *E, bfq_bamp_err *X)
{
    *PS = bfq_bam_patch_stats{};
    *X = bfq_bamp_err{};
    *E = bfq_bam_err{};
    for (u32 k = 0; k < 3; k++)
        if (text[k] && !bfq_bamp_gzip_ok(text[k], textLen[k], k, X)) return 2;
    u32 nref = 0;
    u64 hdrEnd = 0;
    std::vector<bfq_bam_piece> P;
    std::vector<bfq_bam_job> jobs;
    bfq_bam_stats S;
    if (!bfq_bam_host_chain(s, len, O, &nref, &hdrEnd, P, jobs, &S, E)) return 1;
    PS->raw_len = len;
    if (cap < len) return 3;
    std::vector<u64> lineEnd[3];
    bfq_bam_texts T{};
    bool present[3];
    for (u32 k = 0; k < 3; k++) {
        present[k] = text[k] != nullptr;
        if (!present[k]) continue;
        for (u64 p = 0; p < textLen[k]; p++)
            if (text[k][p] == 10) lineEnd[k].push_back(p);
        if (textLen[k] && text[k][textLen[k] - 1] != 10) lineEnd[k].push_back(textLen[k]);
        if (!bfq_bamp_lines_ok(lineEnd[k].size(), S.written[k], k, X)) return 2;
        T.text[k] = text[k]; T.lineEnd[k] = lineEnd[k].data(); T.len[k] = textLen[k];
    }
    const std::vector<u64> recBase = bfq_bamp_rec_bases(P, jobs, hdrEnd, O.piece);
    for (size_t j = 0; j < jobs.size(); j++)
        if (bfq_bam_patch_check<bfq_bamp_alone>(s, len, jobs[j], nref, O, T, 0, 1, X) != BFQ_BAM_NONE) { X->rec += recBase[j]; return 2; }
    if (len) memcpy(out, s, (size_t)len);
    std::vector<bfq_bamp_cnt> cnt(jobs.size() + 1, bfq_bamp_cnt{});
    for (size_t j = 0; j < jobs.size(); j++) bfq_bam_patch_job<bfq_bamp_alone>(out, len, jobs[j], nref, O, T, 0, 1, &cnt[j]);
    bfq_bamp_totals(S, present, len, cnt.data(), jobs.size(), PS);
    PS->raw_len = len;
    return 0;
}
