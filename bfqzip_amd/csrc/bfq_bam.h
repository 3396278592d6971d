// bfq_bam.h -- unaligned (or any) BAM to FASTQ text, host and device: the format, the record check, the record-start rule,
// the decode tables, the walkers, the chain and every bound.  Plain C++, shared by the kernels (k_bam.hip), the host side
// (bfq_bam.hip) and the sanitizer program (tests/cxx/test_bam.cpp).
//
// The inflated stream (all little-endian):  "BAM\1" | l_text:i32 text | n_ref:i32 { l_name:i32 name l_ref:i32 } x n_ref |
// records to the end.  A record is block_size:u32 and block_size bytes:
//    0 refID:i32   4 pos:i32   8 l_read_name:u8   9 mapq:u8  10 bin:u16  12 n_cigar_op:u16  14 flag:u16  16 l_seq:u32
//   20 next_refID:i32  24 next_pos:i32  28 tlen:i32  32 read_name[l_read_name] (NUL-terminated)  cigar:u32[n_cigar_op]
//   seq:u8[(l_seq + 1) / 2] (high nibble first)  qual:u8[l_seq] (0xFF first: absent)  auxiliary tags (ignored).
// Records are length-prefixed, so where record i + 1 starts is known only after record i has been read.  The stream is cut
// into pieces (piece k = [hdrEnd + k * piece, hdrEnd + (k + 1) * piece)); in every piece behind the first the lowest offset
// that passes the record-start rule (bfq_bam_candidate: a heuristic) starts a walker, which hops from record to record up
// to the first record at or behind the piece's end: its landing.  The chain (bfq_bam_chain) goes from the header's end from
// landing to landing; a piece whose walker did not START at the chain's landing is walked again from there.  Exactness
// rests on the chain alone: every record on it has passed bfq_bam_check, whatever the rule found.
//
// What a record becomes -- this project's definition, modelled on the defaults of `samtools fastq` (parity with it is not
// pinned by any test: no htslib tool exists where this was written):
//   flag & exclude_flags != 0: left out.  "@" name [ "/1" | "/2" ] \n sequence \n "+" \n qualities \n.  The suffix (mate_suffix)
//   stands where exactly one of READ1 (0x40) / READ2 (0x80) is set.  Flag 0x10: the sequence is reverse-complemented and
//   the qualities reversed.  Quality: phred + 33, above 93 written as '~' (counted); absent: default_qual + 33 throughout.
//   split: READ1-only records go to output 1, READ2-only to output 2, the rest to output 0; else all to output 0.
// A kept record is l_read_name + 2 * l_seq + 5 bytes of text, + 2 with a suffix.
#pragma once
#include "bfq_common.h"
#include "../../include/bfqzip_hip.h"
#include <stdio.h>
#include <string.h>
#include <functional>
#include <string>
#include <vector>

#define BFQ_BAM_DEF_PIECE 65536u
#define BFQ_BAM_MIN_PIECE 64u
#define BFQ_BAM_MAX_PIECE (1u << 30)
#define BFQ_BAM_MAX_BLOCK (1u << 24)              // a record above 16 MiB is refused (a 65 000-base read is below 100 KiB)
#define BFQ_BAM_MAX_REF (1u << 20)
#define BFQ_BAM_NONE (~0ull)
#define BFQ_BAM_MAX_QUAL 93u                      // '~' - 33
// text per byte of stream: l_read_name + 2 l_seq + 7 <= 4/3 (36 + l_read_name + 3/2 l_seq)
#define BFQ_BAM_TEXT_BOUND(raw) ((raw) + (raw) / 3 + 64)

// why a stream is refused (0: it is fine).  One code per rule; bfq_bam_reason() words them.
enum {
    BFQ_BAM_OK = 0,
    BFQ_BAM_E_MAGIC,         // header: not "BAM\1"
    BFQ_BAM_E_HDR_SHORT,     // header: the stream ends inside it
    BFQ_BAM_E_L_TEXT,        // header: l_text < 0
    BFQ_BAM_E_N_REF,         // header: n_ref outside [0, 2^20]
    BFQ_BAM_E_L_NAME,        // header: l_name < 1
    BFQ_BAM_E_REF_NUL,       // header: a reference name that does not end with NUL
    BFQ_BAM_E_SMALL,         // block_size < 32
    BFQ_BAM_E_BIG,           // block_size > 2^24
    BFQ_BAM_E_PAST,          // the block runs past the end of the stream (a stream that ends inside a record)
    BFQ_BAM_E_NAME0,         // l_read_name == 0
    BFQ_BAM_E_LAYOUT,        // 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq > block_size
    BFQ_BAM_E_NAME,          // the name does not end with NUL, or holds one
    BFQ_BAM_E_REF,           // refID or next_refID outside [-1, n_ref)
    BFQ_BAM_E_TOO_LONG,      // l_seq > BFQ_MAX_READ_LEN
    BFQ_BAM_E_PAIR_COUNT,    // the pairing check: outputs 1 and 2 differ in length
    BFQ_BAM_E_PAIR_NAME,     // the pairing check: the names of a pair differ
    BFQ_BAM_E_NUM,
    BFQ_BAM_NOT_CANDIDATE = 255   // bfq_bam_check(strict): a record, but not one the rule starts a walker on
};

BFQ_HD const char *bfq_bam_reason(int r)
{
    switch (r) {
    case BFQ_BAM_OK: return "ok";
    case BFQ_BAM_E_MAGIC: return "no BAM magic (42 41 4d 01 expected)";
    case BFQ_BAM_E_HDR_SHORT: return "the stream ends inside the header";
    case BFQ_BAM_E_L_TEXT: return "negative header text length";
    case BFQ_BAM_E_N_REF: return "reference count outside [0, 1048576]";
    case BFQ_BAM_E_L_NAME: return "reference name length below 1";
    case BFQ_BAM_E_REF_NUL: return "reference name without its final NUL";
    case BFQ_BAM_E_SMALL: return "block size below 32";
    case BFQ_BAM_E_BIG: return "block size above 16777216";
    case BFQ_BAM_E_PAST: return "the record runs past the end of the stream";
    case BFQ_BAM_E_NAME0: return "read name length 0";
    case BFQ_BAM_E_LAYOUT: return "name, CIGAR, sequence and qualities do not fit the block";
    case BFQ_BAM_E_NAME: return "read name without its final NUL or with a NUL inside";
    case BFQ_BAM_E_REF: return "reference index outside [-1, n_ref)";
    case BFQ_BAM_E_TOO_LONG: return "read longer than 65000 bases";
    case BFQ_BAM_E_PAIR_COUNT: return "no mate";
    case BFQ_BAM_E_PAIR_NAME: return "the names of READ1 and READ2 differ";
    default: return "unknown";
    }
}

BFQ_HD u32 bfq_bam_le16(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8); }
BFQ_HD u32 bfq_bam_le32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

// ---------------------------------------------------------------- one record
struct bfq_bam_rec { u32 bs, ln, nc, flag, lseq; };   // block_size, l_read_name, n_cigar_op, flag, l_seq
// The record that starts at s[o], o < len: 0 and *R, or why it is refused.  Reads nothing outside s[0, len).  strict adds
// what the record-start rule asks beyond well-formedness (pos, next_pos >= -1; printable name bytes).
BFQ_HD int bfq_bam_check(const u8 *s, u64 len, u64 o, u32 nref, bool strict, bfq_bam_rec *R)
{
    if (len - o < 4) return BFQ_BAM_E_PAST;
    const u32 bs = bfq_bam_le32(s + o);
    if (bs < 32) return BFQ_BAM_E_SMALL;
    if (bs > BFQ_BAM_MAX_BLOCK) return BFQ_BAM_E_BIG;
    if (bs > len - o - 4) return BFQ_BAM_E_PAST;
    const u8 *r = s + o + 4;
    const int refID = (int)bfq_bam_le32(r), pos = (int)bfq_bam_le32(r + 4), nextRef = (int)bfq_bam_le32(r + 20), nextPos = (int)bfq_bam_le32(r + 24);
    R->bs = bs; R->ln = r[8]; R->nc = bfq_bam_le16(r + 12); R->flag = bfq_bam_le16(r + 14); R->lseq = bfq_bam_le32(r + 16);
    if (R->ln == 0) return BFQ_BAM_E_NAME0;
    if (32ull + R->ln + 4ull * R->nc + ((u64)R->lseq + 1) / 2 + R->lseq > bs) return BFQ_BAM_E_LAYOUT;
    if (r[32 + R->ln - 1] != 0) return BFQ_BAM_E_NAME;
    bool plain = true;
    for (u32 i = 0; i + 1 < R->ln; i++) {
        const u8 ch = r[32 + i];
        if (ch == 0) return BFQ_BAM_E_NAME;
        plain = plain && ch >= 0x21 && ch <= 0x7e;
    }
    if (refID < -1 || refID >= (int)nref || nextRef < -1 || nextRef >= (int)nref) return BFQ_BAM_E_REF;
    if (R->lseq > BFQ_MAX_READ_LEN) return BFQ_BAM_E_TOO_LONG;
    if (strict && (!plain || pos < -1 || nextPos < -1)) return BFQ_BAM_NOT_CANDIDATE;
    return BFQ_BAM_OK;
}
// The record-start rule: the strict check passes at o, and again where that record ends unless the stream ends there.
BFQ_HD bool bfq_bam_candidate(const u8 *s, u64 len, u64 o, u32 nref)
{
    bfq_bam_rec R;
    if (bfq_bam_check(s, len, o, nref, true, &R)) return false;
    const u64 next = o + 4 + R.bs;
    return next == len || bfq_bam_check(s, len, next, nref, true, &R) == BFQ_BAM_OK;
}

BFQ_HD u32 bfq_bam_mate(u32 flag) { return (flag & 0x40u) && !(flag & 0x80u) ? 1u : (flag & 0x80u) && !(flag & 0x40u) ? 2u : 0u; }
BFQ_HD u64 bfq_bam_text_bytes(const bfq_bam_rec &R, const bfq_bam_opts &O) { return (u64)R.ln + 2ull * R.lseq + 5 + (O.mate_suffix && bfq_bam_mate(R.flag) ? 2 : 0); }
BFQ_HD u8 bfq_bam_base(u32 nib, bool rev) { return (u8)(rev ? "=TGKCYSBAWRDMHVN" : "=ACMGRSVTWYHKDBN")[nib & 15u]; }

// The text of the record at s[o] (checked: R) at dst[0, bfq_bam_text_bytes), by nl lanes of which this is lane `lane`: the
// lanes share the name, the bases and the qualities byte by byte, so that neighbouring lanes store neighbouring bytes.
BFQ_HD void bfq_bam_emit(const u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_opts &O, u8 *dst, u32 lane, u32 nl)
{
    const u8 *name = s + o + 36, *seq = name + R.ln + 4ull * R.nc, *qual = seq + (R.lseq + 1) / 2;
    const u32 mate = O.mate_suffix ? bfq_bam_mate(R.flag) : 0, nameLen = R.ln - 1, L = R.lseq;
    const bool rev = (R.flag & 0x10u) != 0;
    for (u32 i = lane; i < nameLen; i += nl) dst[1 + i] = name[i];
    u8 *p = dst + 1 + nameLen;
    if (lane == 0) {
        dst[0] = '@';
        if (mate) { p[0] = '/'; p[1] = (u8)('0' + mate); }
        p[mate ? 2 : 0] = '\n';
    }
    p += mate ? 3 : 1;
    for (u32 i = lane; i < L; i += nl) {
        const u32 j = rev ? L - 1 - i : i;
        p[i] = bfq_bam_base((u32)seq[j >> 1] >> ((j & 1u) ? 0 : 4), rev);
    }
    p += L;
    if (lane == 0) { p[0] = '\n'; p[1] = '+'; p[2] = '\n'; p[3 + L] = '\n'; }
    p += 3;
    const bool absent = L && qual[0] == 0xFF;
    for (u32 i = lane; i < L; i += nl) {
        const u32 q = absent ? O.default_qual : qual[rev ? L - 1 - i : i];
        p[i] = (u8)(33 + (q > BFQ_BAM_MAX_QUAL ? BFQ_BAM_MAX_QUAL : q));
    }
}

// ---------------------------------------------------------------- walkers
// What one walker found.  start == BFQ_BAM_NONE: the piece has no candidate and no walker.  status != 0: dead at record
// badRec (of this walker) at byte badOff.
struct bfq_bam_piece {
    u64 start, landing, badOff, clamped;
    u64 bytes[3];
    u32 kept[3];
    u32 nrec, skipped, reversed, noQual, status, badRec, pad;
};
// Hops from `start` over the records that start below `end` (<= len), checks every one and counts.  All nl lanes do the
// same hops; they share the quality bytes for the count of clamped values, of which this lane's share is returned (the
// caller sums the lanes into P->clamped).
BFQ_HD u64 bfq_bam_walk(const u8 *s, u64 len, u64 start, u64 end, u32 nref, const bfq_bam_opts &O, u32 lane, u32 nl, bfq_bam_piece *P)
{
    bfq_bam_piece W{};
    W.start = start;
    u64 o = start, clamped = 0;
    while (o < end) {
        bfq_bam_rec R;
        const int r = bfq_bam_check(s, len, o, nref, false, &R);
        if (r) { W.status = (u32)r; W.badOff = o; W.badRec = W.nrec; break; }
        W.nrec++;
        if (R.flag & O.exclude_flags) W.skipped++;
        else {
            const u32 out = O.split ? bfq_bam_mate(R.flag) : 0;
            W.kept[out]++;
            W.bytes[out] += bfq_bam_text_bytes(R, O);
            if (R.flag & 0x10u) W.reversed++;
            if (R.lseq) {
                const u8 *qual = s + o + 36 + R.ln + 4ull * R.nc + (R.lseq + 1) / 2;
                if (qual[0] == 0xFF) W.noQual++;
                else
                    for (u32 i = lane; i < R.lseq; i += nl) clamped += qual[i] > BFQ_BAM_MAX_QUAL ? 1 : 0;
            }
        }
        o += 4ull + R.bs;
    }
    W.landing = o;
    *P = W;
    return clamped;
}

// One piece of the chain: its records start in [start, end); their text begins at byteBase[] of the outputs, and they are
// records recBase[] of them.
struct bfq_bam_job { u64 start, end, byteBase[3], recBase[3]; };
struct bfq_bam_outs { u8 *text[3]; u64 *names[3]; };   // names[k]: where record i of output k starts in the stream (nullptr: not wanted)
// The second walk of a chain piece: every kept record's text, by nl lanes.
BFQ_HD void bfq_bam_place(const u8 *s, u64 len, const bfq_bam_job &J, u32 nref, const bfq_bam_opts &O, const bfq_bam_outs &out, u32 lane, u32 nl)
{
    u64 at[3] = {J.byteBase[0], J.byteBase[1], J.byteBase[2]}, idx[3] = {J.recBase[0], J.recBase[1], J.recBase[2]};
    for (u64 o = J.start; o < J.end;) {
        bfq_bam_rec R;
        if (bfq_bam_check(s, len, o, nref, false, &R)) break;       // (the count pass has passed every record of the chain)
        if (!(R.flag & O.exclude_flags)) {
            const u32 k = O.split ? bfq_bam_mate(R.flag) : 0;
            bfq_bam_emit(s, o, R, O, out.text[k] + at[k], lane, nl);
            if (out.names[k] && lane == 0) out.names[k][idx[k]] = o;
            at[k] += bfq_bam_text_bytes(R, O);
            idx[k]++;
        }
        o += 4ull + R.bs;
    }
}
// the names of the records at a and b (both on the chain) are the same
BFQ_HD bool bfq_bam_same_name(const u8 *s, u64 a, u64 b)
{
    const u32 n = s[a + 12];
    if (n != s[b + 12]) return false;
    for (u32 i = 0; i < n; i++)
        if (s[a + 36 + i] != s[b + 36 + i]) return false;
    return true;
}

// ---------------------------------------------------------------- host side: options, header, chain, messages
struct bfq_bam_err { int reason = 0; bool header = false; u64 rec = 0, off = 0, n1 = 0, n2 = 0; };
inline std::string bfq_bam_message(const bfq_bam_err &E)
{
    char b[320];
    if (E.reason == BFQ_BAM_E_PAIR_COUNT)
        snprintf(b, sizeof b, "unpaired BAM input: pair %llu: no mate (%llu READ1 records, %llu READ2 records); collate the file by name first", E.rec, E.n1, E.n2);
    else if (E.reason == BFQ_BAM_E_PAIR_NAME)
        snprintf(b, sizeof b, "unpaired BAM input: pair %llu: the names of READ1 and READ2 differ; collate the file by name first", E.rec);
    else if (E.header) snprintf(b, sizeof b, "damaged BAM input: header at byte %llu: %s", E.off, bfq_bam_reason(E.reason));
    else snprintf(b, sizeof b, "damaged BAM input: record %llu at byte %llu: %s", E.rec, E.off, bfq_bam_reason(E.reason));
    return b;
}
// the options of a call (in == nullptr: the defaults) with the default piece put in; false: an option out of range (*why)
inline bool bfq_bam_resolve(const bfq_bam_opts *in, bfq_bam_opts *O, const char **why)
{
    if (in) *O = *in;
    else { memset(O, 0, sizeof *O); O->exclude_flags = 0x900; O->mate_suffix = 1; O->default_qual = 1; }
    if (!O->piece) O->piece = BFQ_BAM_DEF_PIECE;
    *why = nullptr;
    if (O->piece < BFQ_BAM_MIN_PIECE || O->piece > BFQ_BAM_MAX_PIECE) *why = "BAM piece: 64 bytes to 1 GiB";
    else if (O->default_qual > BFQ_BAM_MAX_QUAL) *why = "BAM default quality: 0 to 93";
    else if (O->paired_check && !O->split) *why = "the BAM pairing check needs split = 1";
    return *why == nullptr;
}
inline u64 bfq_bam_pieces(u64 len, u64 hdrEnd, u64 piece) { return len > hdrEnd ? (len - hdrEnd + piece - 1) / piece : 1; }

// The header of a stream of len bytes, of which fetch(off, n, dst) copies [off, off + n) (off + n <= len): n_ref and where
// the records begin.  A window of 1 MiB is fetched at a time, so a header of any size costs len / 1 MiB fetches at most.
template <class Fetch> inline int bfq_bam_header(Fetch &&fetch, u64 len, u32 *nref, u64 *hdrEnd, u64 *badOff)
{
    std::vector<u8> win;
    u64 winAt = 0;
    auto get = [&](u64 off, u32 n) -> const u8 * {                  // n <= 8, off + n <= len
        if (win.empty() || off < winAt || off + n > winAt + win.size()) {
            const u64 take = len - off < (1u << 20) ? len - off : (1u << 20);
            win.resize((size_t)take);
            fetch(off, take, win.data());
            winAt = off;
        }
        return win.data() + (off - winAt);
    };
    *nref = 0; *hdrEnd = 0; *badOff = 0;
    if (len < 4) return BFQ_BAM_E_HDR_SHORT;
    if (memcmp(get(0, 4), "BAM\1", 4) != 0) return BFQ_BAM_E_MAGIC;
    *badOff = 4;
    if (len < 8) return BFQ_BAM_E_HDR_SHORT;
    const int ltext = (int)bfq_bam_le32(get(4, 4));
    if (ltext < 0) return BFQ_BAM_E_L_TEXT;
    u64 p = 8 + (u64)ltext;
    *badOff = 8;
    if (p > len) return BFQ_BAM_E_HDR_SHORT;
    *badOff = p;
    if (len - p < 4) return BFQ_BAM_E_HDR_SHORT;
    const int n = (int)bfq_bam_le32(get(p, 4));
    if (n < 0 || (u32)n > BFQ_BAM_MAX_REF) return BFQ_BAM_E_N_REF;
    p += 4;
    for (int i = 0; i < n; i++) {
        *badOff = p;
        if (len - p < 4) return BFQ_BAM_E_HDR_SHORT;
        const int lname = (int)bfq_bam_le32(get(p, 4));
        if (lname < 1) return BFQ_BAM_E_L_NAME;
        if (len - p - 4 < (u64)lname + 4) return BFQ_BAM_E_HDR_SHORT;
        if (*get(p + 4 + (u64)lname - 1, 1) != 0) return BFQ_BAM_E_REF_NUL;
        p += 8 + (u64)lname;
    }
    *nref = (u32)n; *hdrEnd = p; *badOff = 0;
    return BFQ_BAM_OK;
}

// The chain.  P[k]: what pass 1 found in piece k (P[0] started at hdrEnd).  rewalk(k, start) walks piece k again from
// `start` and returns its record.  Fills the chain's jobs, *S (all but n_ref and header_bytes) and, on a record that fails
// the check on the chain, *E.
template <class Rewalk> inline void bfq_bam_chain(std::vector<bfq_bam_piece> &P, u64 hdrEnd, u64 len, u64 piece, Rewalk &&rewalk,
                                                  std::vector<bfq_bam_job> &jobs, bfq_bam_stats *S, bfq_bam_err *E)
{
    const u64 np = P.size();
    S->pieces = np; S->rounds = 1;
    for (const bfq_bam_piece &w : P)
        if (w.start != BFQ_BAM_NONE) { S->walkers++; if (w.status) S->dead++; }
    u64 bytes[3] = {0, 0, 0};
    for (u64 pos = hdrEnd; pos < len;) {
        const u64 k = (pos - hdrEnd) / piece;
        if (P[k].start != pos) {                                     // a false start, or no walker: a round of its own
            P[k] = rewalk(k, pos);
            S->repaired++; S->rounds++;
        }
        const bfq_bam_piece &w = P[k];
        if (w.status) {
            E->reason = (int)w.status; E->header = false; E->rec = S->records + w.badRec; E->off = w.badOff;
            return;
        }
        bfq_bam_job J;
        J.start = pos;
        J.end = hdrEnd + (k + 1) * piece < len ? hdrEnd + (k + 1) * piece : len;
        for (int o = 0; o < 3; o++) { J.byteBase[o] = bytes[o]; J.recBase[o] = S->written[o]; bytes[o] += w.bytes[o]; S->written[o] += w.kept[o]; }
        jobs.push_back(J);
        S->records += w.nrec; S->skipped += w.skipped; S->reversed += w.reversed; S->no_qual += w.noQual; S->clamped_quals += w.clamped;
        pos = w.landing;
    }
}
// the lengths of the three texts: where the chain's last piece ends
inline void bfq_bam_totals(const std::vector<bfq_bam_piece> &P, const std::vector<bfq_bam_job> &jobs, u64 hdrEnd, u64 piece, u64 outLen[3])
{
    outLen[0] = outLen[1] = outLen[2] = 0;
    if (jobs.empty()) return;
    const bfq_bam_job &J = jobs.back();
    const bfq_bam_piece &w = P[(J.start - hdrEnd) / piece];
    for (int o = 0; o < 3; o++) outLen[o] = J.byteBase[o] + w.bytes[o];
}
// the pairing check's count rule; the names are compared by the caller
inline bool bfq_bam_pair_counts(const bfq_bam_stats &S, bfq_bam_err *E)
{
    if (S.written[1] == S.written[2]) return true;
    E->reason = BFQ_BAM_E_PAIR_COUNT; E->header = false;
    E->rec = S.written[1] < S.written[2] ? S.written[1] : S.written[2];
    E->n1 = S.written[1]; E->n2 = S.written[2];
    return false;
}

// What steps 1-3 leave on the device side: the stream in the arena (d_s, raw bytes) and the chain.  bfq_bam.hip's, declared
// here for the two host files of the BAM calls (bfq_bam.hip, bfq_bam_patch.hip):
//   bfq_bam_chain_device  steps 1-3: the stream of h_in[0, len) into the arena -- reserved there, once, with more(raw length)
//                         bytes beside the stream --, the header, the counting walk, the chain; *stats (may be null) is set
//                         before a damaged file is refused
//   bfq_bam_refuse        throws the refusal that *E words;  bfq_bam_opts_of: the resolved options of a call, or throws
//   bfq_bam_host_error_set  the calling thread's bfq_bam_host_error()
struct bfq_bam_chain_dev { u8 *d_s = nullptr; u64 raw = 0, hdrEnd = 0; u32 nref = 0; std::vector<bfq_bam_piece> P; std::vector<bfq_bam_job> jobs; bfq_bam_stats S; };
void bfq_bam_chain_device(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts &O, const std::function<size_t(u64)> &more, bfq_bam_stats *stats,
                          bfq_bam_chain_dev *C);
void bfq_bam_refuse(const bfq_bam_err &E);
bfq_bam_opts bfq_bam_opts_of(const bfq_bam_opts *in);
void bfq_bam_host_error_set(const std::string &msg);

// Steps 1-3 by one thread on the inflated stream s[0, len): the header, the candidates and the counting walk, the chain.
// O: resolved options.  Fills P, jobs, *S and -- returning false -- *E.  Shared by both directions' host forms.
inline bool bfq_bam_host_chain(const u8 *s, u64 len, const bfq_bam_opts &O, u32 *nrefOut, u64 *hdrEndOut, std::vector<bfq_bam_piece> &P,
                               std::vector<bfq_bam_job> &jobs, bfq_bam_stats *S, bfq_bam_err *E)
{
    *S = bfq_bam_stats{};
    *E = bfq_bam_err{};
    u32 nref = 0;
    u64 hdrEnd = 0, bad = 0;
    const int hr = bfq_bam_header([&](u64 off, u64 n, u8 *dst) { memcpy(dst, s + off, (size_t)n); }, len, &nref, &hdrEnd, &bad);
    if (hr) { E->reason = hr; E->header = true; E->off = bad; return false; }
    S->n_ref = nref; S->header_bytes = hdrEnd;
    *nrefOut = nref; *hdrEndOut = hdrEnd;
    const u64 piece = O.piece, np = bfq_bam_pieces(len, hdrEnd, piece);
    P.assign(np, bfq_bam_piece{});
    for (u64 k = 0; k < np; k++) {
        const u64 lo = hdrEnd + k * piece, hi = lo + piece < len ? lo + piece : len;
        u64 cand = k ? BFQ_BAM_NONE : hdrEnd;
        for (u64 o = lo; k && o < hi && cand == BFQ_BAM_NONE; o++)
            if (bfq_bam_candidate(s, len, o, nref)) cand = o;
        if (cand == BFQ_BAM_NONE) { P[k] = bfq_bam_piece{}; P[k].start = BFQ_BAM_NONE; continue; }
        P[k].clamped = bfq_bam_walk(s, len, cand, hi, nref, O, 0, 1, &P[k]);
    }
    bfq_bam_chain(P, hdrEnd, len, piece, [&](u64 k, u64 start) {
        bfq_bam_piece w;
        const u64 hi = hdrEnd + (k + 1) * piece < len ? hdrEnd + (k + 1) * piece : len;
        const u64 cl = bfq_bam_walk(s, len, start, hi, nref, O, 0, 1, &w);
        w.clamped = cl;
        return w;
    }, jobs, S, E);
    return E->reason == 0;
}

// The host form: the same steps by one thread on the inflated stream s[0, len).  O: resolved options.  out[k] / cap[k]: the
// three texts (measure: not touched).  Returns 0, 1 = refused (*E), 2 = a capacity below the measured length (outLen: the
// lengths needed; nothing written).
inline int bfq_bam_host(const u8 *s, u64 len, const bfq_bam_opts &O, u8 *const out[3], const u64 cap[3], bool measure, u64 outLen[3], u64 nReads[3],
                        bfq_bam_stats *S, bfq_bam_err *E)
{
    outLen[0] = outLen[1] = outLen[2] = nReads[0] = nReads[1] = nReads[2] = 0;
    u32 nref = 0;
    u64 hdrEnd = 0;
    std::vector<bfq_bam_piece> P;
    std::vector<bfq_bam_job> jobs;
    if (!bfq_bam_host_chain(s, len, O, &nref, &hdrEnd, P, jobs, S, E)) return 1;
    const u64 piece = O.piece;
    bfq_bam_totals(P, jobs, hdrEnd, piece, outLen);
    for (int o = 0; o < 3; o++) nReads[o] = S->written[o];
    if (measure) return 0;
    for (int o = 0; o < 3; o++)
        if (outLen[o] > cap[o]) return 2;
    std::vector<u64> names[3];
    bfq_bam_outs W{};
    for (int o = 0; o < 3; o++) {
        W.text[o] = out[o];
        if (O.paired_check && o) { names[o].resize((size_t)S->written[o] + 1); W.names[o] = names[o].data(); }
    }
    if (O.paired_check && !bfq_bam_pair_counts(*S, E)) return 1;
    for (const bfq_bam_job &J : jobs) bfq_bam_place(s, len, J, nref, O, W, 0, 1);
    if (O.paired_check)
        for (u64 i = 0; i < S->written[1]; i++)
            if (!bfq_bam_same_name(s, names[1][i], names[2][i])) { E->reason = BFQ_BAM_E_PAIR_NAME; E->rec = i; return 1; }
    return 0;
}
