// bfq_bam.h -- unaligned (or any) BAM to FASTQ text, host and device: the format, the record check, the record-start rule,
// the decode tables, the walkers, the chain and every bound.  Plain C++, shared by the kernels (k_bam.hip), the host side
// (bfq_bam.hip) and the sanitizer program (tests/cxx/test_bam.cpp).
//
// The inflated stream (all little-endian):  "BAM\1" | l_text:i32 text | n_ref:i32 { l_name:i32 name l_ref:i32 } x n_ref |
// records to the end.  A record is block_size:u32 and block_size bytes:
//    0 refID:i32   4 pos:i32   8 l_read_name:u8   9 mapq:u8  10 bin:u16  12 n_cigar_op:u16  14 flag:u16  16 l_seq:u32
//   20 next_refID:i32  24 next_pos:i32  28 tlen:i32  32 read_name[l_read_name] (NUL-terminated)  cigar:u32[n_cigar_op]
//   seq:u8[(l_seq + 1) / 2] (high nibble first)  qual:u8[l_seq] (0xFF first: absent)  auxiliary tags (ignored unless asked for).
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
// A kept record is l_read_name + 2 * l_seq + 5 bytes of text, + 2 with a suffix, + what its tags take.
//
// Aux tags into the header line (bfq_bam_tag_opts; off unless asked for) -- this project's definition, modelled on `samtools
// fastq -T`; parity with htslib is not pinned.  The tag area is what follows the qualities up to the block's end: tag:u8[2]
// type:u8 value, with value A: 1 byte; c C: 1; s S: 2; i I f: 4; Z H: bytes and a NUL; B: subtype:u8 (cCsSiIf) count:u32 and
// count elements.  Behind the name and its suffix every SELECTED tag is written as \tXX:T:value, in the record's order (one
// pass over the area; the way back needs that order):  A -> XX:A:c;  c C s S i I -> XX:i:<decimal>;  Z -> XX:Z:<bytes>;
// H -> XX:H:<bytes>.  Selected: every tag (n_tags 0), or those of a list of at most 32 keys, each [A-Za-z][A-Za-z0-9].
//   Not carried: a selected tag of type f or B; one whose Z / H value or A character holds a byte outside [0x20, 0x7e]; one
//   whose key is not [A-Za-z][A-Za-z0-9] (with a list no such key is selected).  It is left out and counted (tags_dropped);
//   with strict the call is refused: "BAM tags: record <i> at byte <off>: tag <XX> of type <T> cannot be carried" (T: the
//   stored type; a key byte outside [!-~] is worded '?').
//   With tags on the tag area of every KEPT record must parse -- at least three bytes per tag, a known type, every value
//   inside the block, a NUL for every Z / H --, else "damaged BAM input: record <i> at byte <off>: malformed tag area"; in
//   one record this comes before the strict refusal.  Excluded records are not looked at; with tags off nothing is checked.
//   Both refusals are a walker's death like every other: the chain names the first such record of the file.
// Text per byte of stream with tags: A 7 of 4; c 10 of 4 ("\tXX:i:-128"), C 9 of 4; s 12 of 5, S 11 of 5; i 17 of 7, I 16 of
// 7; Z / H 6 + n of 4 + n: at most 5/2, as the rest of a record is at most 4/3 (BFQ_BAM_TEXT_BOUND_TAGS).
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
#define BFQ_BAM_TEXT_BOUND_TAGS(raw) (2 * (raw) + (raw) / 2 + 64)   // with tags (above): 5/2

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
    BFQ_BAM_E_TAGS,          // tags asked for: the tag area of a kept record does not parse
    BFQ_BAM_E_CARRY,         // tags asked for, strict: a selected tag that cannot be carried
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
    case BFQ_BAM_E_TAGS: return "malformed tag area";
    case BFQ_BAM_E_CARRY: return "a tag that cannot be carried";
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

// ---------------------------------------------------------------- aux tags
// the selection of a call (on == 0: tags off), what a walker counts, and how the nl lanes of a record agree: the host's one
// lane with itself (the device's wave64: k_bam.hip)
struct bfq_bam_tagsel { u32 on, n, strict, pad; u8 tag[32][2]; };
struct bfq_bam_tagcnt { u64 written, dropped, bytes; };
struct bfq_bam_alone {
    static BFQ_HD u32 first(bool v) { return v ? 0u : 1u; }         // the lowest lane whose v holds; nl: none
    static BFQ_HD bool any(bool v) { return v; }
};
BFQ_HD bool bfq_bam_key_ok(u32 a, u32 b) { return ((a | 32u) - 'a' < 26u) && (((b | 32u) - 'a' < 26u) || (b - '0' < 10u)); }
BFQ_HD bool bfq_bam_selected(const bfq_bam_tagsel &G, u32 a, u32 b)
{
    if (!G.n) return true;
    for (u32 j = 0; j < G.n; j++)
        if (G.tag[j][0] == a && G.tag[j][1] == b) return true;
    return false;
}
// One tag: its key and stored type; carried: it can be written; val: where its value begins; vlen: the bytes of a Z / H value
// in front of the NUL; text: the bytes of "\tXX:T:value"; num: an integer's value; next: where the next tag begins.
struct bfq_bam_tag { u32 k0, k1, type, carried, vlen, text; u64 val, next; long long num; };
// The tag at s[p] of a tag area that ends at `end` (p < end <= the stream's length), by nl lanes that all take the same
// path: false: malformed.  Only the bytes of a Z / H value are shared -- lane i looks at bytes i, i + nl, ..., and the NUL is
// the lowest lane that sees one (one vote per nl bytes) --; everything else is the same few loads in every lane.
template <class W> BFQ_HD bool bfq_bam_tag_at(const u8 *s, u64 p, u64 end, u32 lane, u32 nl, bfq_bam_tag *T)
{
    if (end - p < 3) return false;
    const u32 ty = s[p + 2];
    const u64 v = p + 3;
    const bool key = bfq_bam_key_ok(s[p], s[p + 1]);
    T->k0 = s[p]; T->k1 = s[p + 1]; T->type = ty; T->val = v; T->vlen = 0; T->num = 0; T->text = 0; T->carried = 0;
    if (ty == 'Z' || ty == 'H') {
        bool bad = false;
        for (u64 base = 0;; base += nl) {
            const u64 q = v + base + lane;
            const bool in = q < end;
            const u32 ch = in ? s[q] : 0u;
            const u32 f = W::first(!in || ch == 0);
            const bool b = W::any(lane < f && (ch < 0x20u || ch > 0x7eu));
            bad = bad || b;
            if (f < nl) { T->vlen = (u32)(base + f); break; }
        }
        if (v + T->vlen >= end) return false;                       // no NUL inside the block
        T->carried = key && !bad; T->text = 6u + T->vlen; T->next = v + T->vlen + 1;
        return true;
    }
    if (ty == 'B') {
        if (end - v < 5) return false;
        const u32 sub = s[v], es = sub == 'c' || sub == 'C' ? 1u : sub == 's' || sub == 'S' ? 2u : sub == 'i' || sub == 'I' || sub == 'f' ? 4u : 0u;
        const u64 bytes = (u64)bfq_bam_le32(s + v + 1) * es;
        if (!es || bytes > end - v - 5) return false;
        T->next = v + 5 + bytes;
        return true;
    }
    const u32 w = ty == 'A' || ty == 'c' || ty == 'C' ? 1u : ty == 's' || ty == 'S' ? 2u : ty == 'i' || ty == 'I' || ty == 'f' ? 4u : 0u;
    if (!w || end - v < w) return false;
    T->next = v + w;
    if (ty == 'f') return true;
    if (ty == 'A') { T->carried = key && s[v] >= 0x20 && s[v] <= 0x7e; T->text = 7; return true; }
    const u32 x = w == 1 ? s[v] : w == 2 ? bfq_bam_le16(s + v) : bfq_bam_le32(s + v);
    const long long n = ty == 'c' ? (long long)(signed char)x : ty == 's' ? (long long)(short)x : ty == 'i' ? (long long)(int)x : (long long)x;
    u32 d = 1;
    for (u64 a = (u64)(n < 0 ? -n : n); a >= 10; a /= 10) d++;
    T->num = n; T->carried = key; T->text = 6u + d + (n < 0 ? 1u : 0u);
    return true;
}
BFQ_HD u64 bfq_bam_tag_area(u64 o, const bfq_bam_rec &R) { return o + 36 + R.ln + 4ull * R.nc + ((u64)R.lseq + 1) / 2 + R.lseq; }
// The tag area of the record at s[o] (checked: R), by nl lanes: 0 and what its selected tags take added to *C, or
// BFQ_BAM_E_TAGS, or -- strict -- BFQ_BAM_E_CARRY with *bad = key | type << 16 of the record's first such tag.
template <class W> BFQ_HD u32 bfq_bam_tags_count(const u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_tagsel &G, u32 lane, u32 nl, bfq_bam_tagcnt *C, u32 *bad)
{
    const u64 end = o + 4ull + R.bs;
    bfq_bam_tagcnt c{};
    u32 first = 0;
    for (u64 p = bfq_bam_tag_area(o, R); p < end;) {
        bfq_bam_tag T;
        if (!bfq_bam_tag_at<W>(s, p, end, lane, nl, &T)) return BFQ_BAM_E_TAGS;
        if (bfq_bam_selected(G, T.k0, T.k1)) {
            if (T.carried) { c.written++; c.bytes += T.text; }
            else { if (!c.dropped) first = T.k0 | (T.k1 << 8) | (T.type << 16); c.dropped++; }
        }
        p = T.next;
    }
    if (G.strict && c.dropped) { *bad = first; return BFQ_BAM_E_CARRY; }
    C->written += c.written; C->dropped += c.dropped; C->bytes += c.bytes;
    return BFQ_BAM_OK;
}
// The selected tags of the record at s[o] (passed by bfq_bam_tags_count) as text at dst, by nl lanes; returns the bytes.  The
// lanes share the bytes of a Z / H value; the six bytes in front of a value and the <= 11 of an integer are lane 0's.
template <class W> BFQ_HD u64 bfq_bam_tags_emit(const u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_tagsel &G, u8 *dst, u32 lane, u32 nl)
{
    const u64 end = o + 4ull + R.bs;
    u64 at = 0;
    for (u64 p = bfq_bam_tag_area(o, R); p < end;) {
        bfq_bam_tag T;
        if (!bfq_bam_tag_at<W>(s, p, end, lane, nl, &T)) break;     // (the counting walk has passed every kept record)
        if (T.carried && bfq_bam_selected(G, T.k0, T.k1)) {
            u8 *d = dst + at;
            const bool str = T.type == 'Z' || T.type == 'H';
            if (str)
                for (u32 i = lane; i < T.vlen; i += nl) d[6 + i] = s[T.val + i];
            if (lane == 0) {
                d[0] = '\t'; d[1] = (u8)T.k0; d[2] = (u8)T.k1; d[3] = ':'; d[4] = (u8)(str || T.type == 'A' ? T.type : 'i'); d[5] = ':';
                if (T.type == 'A') d[6] = s[T.val];
                else if (!str) {
                    const u32 neg = T.num < 0 ? 1u : 0u;
                    u64 a = (u64)(neg ? -T.num : T.num);
                    for (u32 j = T.text - 6; j-- > neg; a /= 10) d[6 + j] = (u8)('0' + a % 10);
                    if (neg) d[6] = '-';
                }
            }
            at += T.text;
        }
        p = T.next;
    }
    return at;
}

// The text of the record at s[o] (checked: R) at dst[0, the bytes returned), by nl lanes of which this is lane `lane`: the
// lanes share the name, the bases and the qualities byte by byte, so that neighbouring lanes store neighbouring bytes.
// Without TAGS the bytes are bfq_bam_text_bytes; with them the tags' text stands between the suffix and the line's end.
template <bool TAGS = false, class W = bfq_bam_alone>
BFQ_HD u64 bfq_bam_emit(const u8 *s, u64 o, const bfq_bam_rec &R, const bfq_bam_opts &O, u8 *dst, u32 lane, u32 nl, const bfq_bam_tagsel *G = nullptr)
{
    const u8 *name = s + o + 36, *seq = name + R.ln + 4ull * R.nc, *qual = seq + (R.lseq + 1) / 2;
    const u32 mate = O.mate_suffix ? bfq_bam_mate(R.flag) : 0, nameLen = R.ln - 1, L = R.lseq;
    const bool rev = (R.flag & 0x10u) != 0;
    for (u32 i = lane; i < nameLen; i += nl) dst[1 + i] = name[i];
    u8 *p = dst + 1 + nameLen;
    u64 tagText = 0;
    if constexpr (TAGS) tagText = bfq_bam_tags_emit<W>(s, o, R, *G, p + (mate ? 2 : 0), lane, nl);
    if (lane == 0) {
        dst[0] = '@';
        if (mate) { p[0] = '/'; p[1] = (u8)('0' + mate); }
        p[(mate ? 2 : 0) + tagText] = '\n';
    }
    p += (mate ? 3 : 1) + tagText;
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
    return bfq_bam_text_bytes(R, O) + tagText;
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
// caller sums the lanes into P->clamped).  TAGS: the tag area of every kept record is parsed (bfq_bam_tags_count), its text
// counted in bytes[] and in *TC (every lane holds the same *TC); a walker that dies there leaves key and type in pad.
template <bool TAGS = false, class A = bfq_bam_alone>
BFQ_HD u64 bfq_bam_walk(const u8 *s, u64 len, u64 start, u64 end, u32 nref, const bfq_bam_opts &O, u32 lane, u32 nl, bfq_bam_piece *P,
                        const bfq_bam_tagsel *G = nullptr, bfq_bam_tagcnt *TC = nullptr)
{
    bfq_bam_piece W{};
    bfq_bam_tagcnt tc{};
    W.start = start;
    u64 o = start, clamped = 0;
    while (o < end) {
        bfq_bam_rec R;
        const int r = bfq_bam_check(s, len, o, nref, false, &R);
        if (r) { W.status = (u32)r; W.badOff = o; W.badRec = W.nrec; break; }
        u64 tagText = 0;
        if constexpr (TAGS) if (!(R.flag & O.exclude_flags)) {
            const u64 before = tc.bytes;
            u32 bad = 0;
            const u32 tr = bfq_bam_tags_count<A>(s, o, R, *G, lane, nl, &tc, &bad);
            if (tr) { W.status = tr; W.badOff = o; W.badRec = W.nrec; W.pad = bad; break; }
            tagText = tc.bytes - before;
        }
        W.nrec++;
        if (R.flag & O.exclude_flags) W.skipped++;
        else {
            const u32 out = O.split ? bfq_bam_mate(R.flag) : 0;
            W.kept[out]++;
            W.bytes[out] += bfq_bam_text_bytes(R, O) + tagText;
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
    if constexpr (TAGS) *TC = tc;
    return clamped;
}

// One piece of the chain: its records start in [start, end); their text begins at byteBase[] of the outputs, and they are
// records recBase[] of them.
struct bfq_bam_job { u64 start, end, byteBase[3], recBase[3]; };
struct bfq_bam_outs { u8 *text[3]; u64 *names[3]; };   // names[k]: where record i of output k starts in the stream (nullptr: not wanted)
// The second walk of a chain piece: every kept record's text, by nl lanes.
template <bool TAGS = false, class A = bfq_bam_alone>
BFQ_HD void bfq_bam_place(const u8 *s, u64 len, const bfq_bam_job &J, u32 nref, const bfq_bam_opts &O, const bfq_bam_outs &out, u32 lane, u32 nl,
                          const bfq_bam_tagsel *G = nullptr)
{
    u64 at[3] = {J.byteBase[0], J.byteBase[1], J.byteBase[2]}, idx[3] = {J.recBase[0], J.recBase[1], J.recBase[2]};
    for (u64 o = J.start; o < J.end;) {
        bfq_bam_rec R;
        if (bfq_bam_check(s, len, o, nref, false, &R)) break;       // (the count pass has passed every record of the chain)
        if (!(R.flag & O.exclude_flags)) {
            const u32 k = O.split ? bfq_bam_mate(R.flag) : 0;
            const u64 n = bfq_bam_emit<TAGS, A>(s, o, R, O, out.text[k] + at[k], lane, nl, G);
            if (out.names[k] && lane == 0) out.names[k][idx[k]] = o;
            at[k] += n;
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
struct bfq_bam_err { int reason = 0; bool header = false; u64 rec = 0, off = 0, n1 = 0, n2 = 0; u32 tag = 0; };   // tag: key | type << 16 (BFQ_BAM_E_CARRY)
inline std::string bfq_bam_message(const bfq_bam_err &E)
{
    char b[320];
    if (E.reason == BFQ_BAM_E_PAIR_COUNT)
        snprintf(b, sizeof b, "unpaired BAM input: pair %llu: no mate (%llu READ1 records, %llu READ2 records); collate the file by name first", E.rec, E.n1, E.n2);
    else if (E.reason == BFQ_BAM_E_PAIR_NAME)
        snprintf(b, sizeof b, "unpaired BAM input: pair %llu: the names of READ1 and READ2 differ; collate the file by name first", E.rec);
    else if (E.reason == BFQ_BAM_E_CARRY) {
        const auto ch = [](u32 c) { return (char)(c >= 0x21 && c <= 0x7e ? c : '?'); };
        snprintf(b, sizeof b, "BAM tags: record %llu at byte %llu: tag %c%c of type %c cannot be carried", E.rec, E.off, ch(E.tag & 255u), ch((E.tag >> 8) & 255u),
                 ch((E.tag >> 16) & 255u));
    } else if (E.header) snprintf(b, sizeof b, "damaged BAM input: header at byte %llu: %s", E.off, bfq_bam_reason(E.reason));
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
// the tag selection of a call: off unless in->reserved holds BFQ_BAM_OPTS_TAGS; false: refused (*why).  *stats: where the
// caller wants the tag counts (may come back null)
inline bool bfq_bam_tags_resolve(const bfq_bam_opts *in, bfq_bam_tagsel *G, bfq_bam_tag_stats **stats, const char **why)
{
    memset(G, 0, sizeof *G);
    *stats = nullptr; *why = nullptr;
    if (!in || in->reserved != BFQ_BAM_OPTS_TAGS) return true;
    const bfq_bam_tag_opts *X = (const bfq_bam_tag_opts *)in;
    if (X->n_tags > 32) { *why = "BAM tags: more than 32 tags"; return false; }
    for (u32 j = 0; j < X->n_tags; j++) {
        if (!bfq_bam_key_ok(X->tag[j][0], X->tag[j][1])) { *why = "BAM tags: a tag that is not [A-Za-z][A-Za-z0-9]"; return false; }
        G->tag[j][0] = X->tag[j][0]; G->tag[j][1] = X->tag[j][1];
    }
    G->on = 1; G->n = X->n_tags; G->strict = X->strict ? 1u : 0u;
    *stats = X->stats;
    return true;
}
// the tag counts of the chain's pieces
inline bfq_bam_tag_stats bfq_bam_tag_totals(const std::vector<bfq_bam_tagcnt> &T, const std::vector<bfq_bam_job> &jobs, u64 hdrEnd, u64 piece)
{
    bfq_bam_tag_stats S{};
    for (const bfq_bam_job &J : jobs) {
        const bfq_bam_tagcnt &t = T[(J.start - hdrEnd) / piece];
        S.tags_written += t.written; S.tags_dropped += t.dropped; S.tag_bytes += t.bytes;
    }
    return S;
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
            E->reason = (int)w.status; E->header = false; E->rec = S->records + w.badRec; E->off = w.badOff; E->tag = w.pad;
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
struct bfq_bam_chain_dev { u8 *d_s = nullptr; u64 raw = 0, hdrEnd = 0; u32 nref = 0; std::vector<bfq_bam_piece> P; std::vector<bfq_bam_job> jobs; bfq_bam_stats S; bfq_bam_tag_stats T{}; };
void bfq_bam_chain_device(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts &O, const std::function<size_t(u64)> &more, bfq_bam_stats *stats,
                          bfq_bam_chain_dev *C, const bfq_bam_tagsel *G = nullptr);   // G (tags on): the tag counts in C->T
void bfq_bam_refuse(const bfq_bam_err &E);
bfq_bam_opts bfq_bam_opts_of(const bfq_bam_opts *in);
void bfq_bam_host_error_set(const std::string &msg);

// Steps 1-3 by one thread on the inflated stream s[0, len): the header, the candidates and the counting walk, the chain.
// O: resolved options.  Fills P, jobs, *S and -- returning false -- *E.  Shared by both directions' host forms.
inline bool bfq_bam_host_chain(const u8 *s, u64 len, const bfq_bam_opts &O, u32 *nrefOut, u64 *hdrEndOut, std::vector<bfq_bam_piece> &P,
                               std::vector<bfq_bam_job> &jobs, bfq_bam_stats *S, bfq_bam_err *E, const bfq_bam_tagsel *G = nullptr, bfq_bam_tag_stats *TS = nullptr)
{
    const bool tags = G && G->on;
    std::vector<bfq_bam_tagcnt> T;
    const auto walk = [&](u64 from, u64 hi, bfq_bam_piece *w, bfq_bam_tagcnt *t) {
        return tags ? bfq_bam_walk<true>(s, len, from, hi, *nrefOut, O, 0, 1, w, G, t) : bfq_bam_walk(s, len, from, hi, *nrefOut, O, 0, 1, w);
    };
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
    T.assign(np, bfq_bam_tagcnt{});
    for (u64 k = 0; k < np; k++) {
        const u64 lo = hdrEnd + k * piece, hi = lo + piece < len ? lo + piece : len;
        u64 cand = k ? BFQ_BAM_NONE : hdrEnd;
        for (u64 o = lo; k && o < hi && cand == BFQ_BAM_NONE; o++)
            if (bfq_bam_candidate(s, len, o, nref)) cand = o;
        if (cand == BFQ_BAM_NONE) { P[k] = bfq_bam_piece{}; P[k].start = BFQ_BAM_NONE; continue; }
        P[k].clamped = walk(cand, hi, &P[k], &T[k]);
    }
    bfq_bam_chain(P, hdrEnd, len, piece, [&](u64 k, u64 start) {
        bfq_bam_piece w;
        const u64 hi = hdrEnd + (k + 1) * piece < len ? hdrEnd + (k + 1) * piece : len;
        const u64 cl = walk(start, hi, &w, &T[k]);
        w.clamped = cl;
        return w;
    }, jobs, S, E);
    if (tags && TS && !E->reason) *TS = bfq_bam_tag_totals(T, jobs, hdrEnd, piece);
    return E->reason == 0;
}

// The host form: the same steps by one thread on the inflated stream s[0, len).  O: resolved options.  out[k] / cap[k]: the
// three texts (measure: not touched).  Returns 0, 1 = refused (*E), 2 = a capacity below the measured length (outLen: the
// lengths needed; nothing written).
inline int bfq_bam_host(const u8 *s, u64 len, const bfq_bam_opts &O, u8 *const out[3], const u64 cap[3], bool measure, u64 outLen[3], u64 nReads[3],
                        bfq_bam_stats *S, bfq_bam_err *E, const bfq_bam_tagsel *G = nullptr, bfq_bam_tag_stats *TS = nullptr)
{
    outLen[0] = outLen[1] = outLen[2] = nReads[0] = nReads[1] = nReads[2] = 0;
    u32 nref = 0;
    u64 hdrEnd = 0;
    std::vector<bfq_bam_piece> P;
    std::vector<bfq_bam_job> jobs;
    if (!bfq_bam_host_chain(s, len, O, &nref, &hdrEnd, P, jobs, S, E, G, TS)) return 1;
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
    for (const bfq_bam_job &J : jobs) {
        if (G && G->on) bfq_bam_place<true>(s, len, J, nref, O, W, 0, 1, G);
        else bfq_bam_place(s, len, J, nref, O, W, 0, 1);
    }
    if (O.paired_check)
        for (u64 i = 0; i < S->written[1]; i++)
            if (!bfq_bam_same_name(s, names[1][i], names[2][i])) { E->reason = BFQ_BAM_E_PAIR_NAME; E->rec = i; return 1; }
    return 0;
}
