// bfq_ubam.h -- FASTQ texts as an unaligned BAM, host and device: the definition, the sizing pass, the writing pass, the
// messages and the host form.  Plain C++ on top of bfq_bam_patch.h (the texts of a call, their lines) and bfq_bam.h (the
// format), shared by the kernels (k_ubam.hip), the host side (bfq_ubam.hip) and the sanitizer program (tests/cxx/test_ubam.cpp).
//
// "These FASTQ texts as an unaligned BAM."  This project's definition, modelled on the defaults of `samtools import`; parity
// with an htslib tool is not pinned by any test.
//   Inputs: text[k], k = 0, 1, 2, with the meaning of the outputs of bfq_bam_to_fastq*.  Unpaired: text[0] alone, every
//     record flag 4.  Paired: text[1] and text[2] together: record 2i is read i of text[1], flag 77, record 2i + 1 read i of
//     text[2], flag 141; an optional text[0] comes behind all pairs, flag 4.  Exactly one of text[1] / text[2], or differing
//     read counts: BFQ_E_ARG, "FASTQ to BAM: text 1 holds <n> reads, text 2 holds <m>" (an absent text holds 0).
//   The text: plain FASTQ (one that begins with 1f 8b is refused: "inflate the text first"); CR before LF is stripped from
//     every line; a last line without its LF counts.  "FASTQ: number of lines is not a multiple of 4" and "FASTQ:
//     len(DNA) != len(QS) in a record" keep their words.  The header line begins with '@', the third line with '+' (what
//     follows the '+' is dropped).
//   Name: the bytes behind '@' up to the first blank, tab or line end; the rest of the header line is dropped and counted
//     (comments_dropped).  More than 254 bytes, or a byte outside [!-?A-~] (33..126 without '@'), is refused -- the length
//     before any suffix is removed; at most '@' and 255 bytes of the header line are looked at.  With mate_suffix a trailing
//     "/1" of a text[1] name and a trailing "/2" of a text[2] name are removed -- only the matching suffix, and only where
//     at least one byte remains.  An empty name ("@" alone: what a run without kept headers writes) becomes the read's
//     1-based index in decimal: both mates share theirs, the reads of text[0] continue the count behind the pairs (named).
//     paired_check: the names of read i of text[1] and text[2] are compared after the suffix removal (a mate whose header
//     line is refused differs); the first differing pair is named, at its record of text[1].
//   Fixed fields (the 32 bytes behind block_size): refID -1, pos -1, l_read_name, mapq 0, bin 4680, n_cigar_op 0, flag,
//     l_seq, next_refID -1, next_pos -1, tlen 0.
//   SEQ: case-insensitive over =ACMGRSVTWYHKDBN to the nibbles 0..15, any other byte 15 (N; unknown_bases); the spare
//     nibble of an odd length is 0; l_seq may be 0; l_seq > BFQ_MAX_READ_LEN is BFQ_E_TOO_LONG.
//   QUAL: char - 33; a byte below 33 or above 126 is refused.  Qualities are always written: absent qualities cannot come
//     back from a text, so BAM -> text -> BAM is an identity only for records that held qualities <= 93 and no tags.
//   Tags: none, or with rg_id "RG:Z:<rg_id>" on every record (rg_id: 1..255 bytes of [ -~]).
//   Tags out of the header line (bfq_ubam_tag_opts; off unless asked for), modelled on `samtools import -T`; parity with
//     htslib is not pinned.  Behind the name the header line -- all of it, CR before LF stripped -- is cut at tabs.  Where a
//     space ended the name, the bytes up to the first tab are a comment and dropped.  A field [A-Za-z][A-Za-z0-9]:[AiZH]:value
//     becomes a tag of the record, in line order, between QUAL and the RG tag of rg_id, when no list is given (n_tags 0) or
//     its key is in the list (at most 32 keys, each [A-Za-z][A-Za-z0-9]):
//       A  exactly one byte of [ -~]                                      stored A, 4 bytes
//       i  an optional '-' and 1..10 digits, within [-2^31, 2^32 - 1]     stored at htslib's smallest width: 0..255 C, ..65535
//          S, else I; -128.. c, -32768.. s, else i ("-0" is 0): 4, 5 or 7 bytes
//       Z  bytes of [ -~] (may be none)                                   stored Z, 4 + n bytes
//       H  an even number of hex digits (may be none)                     stored H, 4 + n bytes
//     Every other field is dropped and counted (fields_dropped), never refused: types f and B, an integer out of range or
//     above 10 digits, "+5", an empty i, a malformed key, an empty field, a key not in the list, a Z value with a byte outside
//     [ -~] (a NUL in it would end the value early) or above 2^20 bytes, what would take a record's tags above 2^23 bytes;
//     and, with rg_id set, an RG field: the constant RG tag comes last, as without tags.  comments_dropped then counts the
//     reads of which some byte behind the name did not become a tag: a comment, or a dropped field.
//     No field is longer stored than written ("\tXX:A:c" 7 of text, 4 stored; "\tXX:i:0" 7 and 4, 256 9 and 5, 65536 11 and
//     7, -1 8 and 4, -129 10 and 5, -32769 12 and 7; Z / H 6 + n and 4 + n): the stream's bound of bfq_ubam.hip holds.
//     Identity: BAM -> text (every tag, bfq_bam.h) -> BAM (tags on, header_text the original's) gives the inflated stream
//     byte for byte for uBAM records of flags 4 / 77 / 141 with qualities <= 93 (as without tags) whose tags are of types A /
//     Z / H or integers stored at their smallest width and whose values are printable.  Text -> BAM -> text is one for
//     header lines without a comment whose fields are all well-formed (an integer without leading zeros or "-0").
//   Header: "BAM\1", l_text, the text, n_ref 0.  header_text given: written as it is (the caller's to make valid); NULL:
//     "@HD\tVN:1.6\tSO:unsorted\n" and, with rg_id, "@RG\tID:<rg_id>\n".
//   Sizes: a record is 36 + (l_name + 1) + ceil(l_seq / 2) + l_seq bytes, + 4 + strlen(rg_id): the stream's length is
//     exact once the sizing pass has run, before anything is written.
//   Refusals: what is checked per read is checked in this order -- '@', the name's length, its bytes, the mate's name, '+',
//     the two lengths, l_seq, the qualities -- and of all offending reads the one whose record would come first in the file
//     is named: the host form meets it first, the device takes the minimum of (record index, reason) with one atomicMin.
// The sizing pass (bfq_ubam_size_read) is one lane per read; an exclusive prefix sum over the sizes in file order places the
// records; the writing pass (bfq_ubam_write_rec) is nl lanes per record, which share its bytes.
#pragma once
#include "bfq_bam_patch.h"

#define BFQ_UBAM_MAX_NAME 254u
#define BFQ_UBAM_MAX_FIELD (1u << 20)              // bytes of a Z / H value
#define BFQ_UBAM_MAX_TAGS (1u << 23)               // bytes of a record's tags out of its header line
#define BFQ_UBAM_PIECE 65280ull                     // bytes of stream per BGZF member (bfq_deflate.h's BFQ_DEFL_PIECE)

enum {
    BFQ_UBAM_OK = 0,
    BFQ_UBAM_E_HDR,          // the header line does not begin with '@'
    BFQ_UBAM_E_NAME_LONG,    // name above 254 bytes
    BFQ_UBAM_E_NAME_BYTE,    // a byte outside [!-?A-~]
    BFQ_UBAM_E_PAIR_NAME,    // paired_check: the mate's name differs
    BFQ_UBAM_E_PLUS,         // the third line does not begin with '+'
    BFQ_UBAM_E_FASTQ,        // len(DNA) != len(QS)
    BFQ_UBAM_E_TOO_LONG,     // l_seq > BFQ_MAX_READ_LEN
    BFQ_UBAM_E_QUAL,         // a quality byte outside [33, 126]
    BFQ_UBAM_E_GZIP,         // a text begins with 1f 8b
    BFQ_UBAM_E_LINES,        // lines not a multiple of 4
    BFQ_UBAM_E_PAIRS,        // reads of text 1 != reads of text 2
    BFQ_UBAM_E_RG,           // rg_id
    BFQ_UBAM_E_LEVEL,        // level
    BFQ_UBAM_E_HEADER        // header_text of 2^31 bytes or more, or NULL with a length
};
// what is refused: text k, its read i; n / m: the two numbers the message names
struct bfq_ubam_err { u32 kind = 0, k = 0; u64 i = 0, n = 0, m = 0; };
inline int bfq_ubam_code(const bfq_ubam_err &E) { return E.kind == BFQ_UBAM_E_TOO_LONG ? BFQ_E_TOO_LONG : BFQ_E_ARG; }
inline std::string bfq_ubam_message(const bfq_ubam_err &E)
{
    char b[320];
    const char *why = nullptr;
    switch (E.kind) {
    case BFQ_UBAM_E_HDR: why = "the header line does not begin with '@'"; break;
    case BFQ_UBAM_E_NAME_LONG: why = "name longer than 254 bytes"; break;
    case BFQ_UBAM_E_NAME_BYTE: why = "a byte outside [!-?A-~] in the name"; break;
    case BFQ_UBAM_E_PAIR_NAME: why = "the name differs from that of its mate in text 2"; break;
    case BFQ_UBAM_E_PLUS: why = "the third line does not begin with '+'"; break;
    case BFQ_UBAM_E_TOO_LONG: why = "read longer than 65000 bases"; break;
    case BFQ_UBAM_E_QUAL: why = "a quality byte outside [33, 126]"; break;
    case BFQ_UBAM_E_FASTQ: return "FASTQ: len(DNA) != len(QS) in a record";
    case BFQ_UBAM_E_LINES: return "FASTQ: number of lines is not a multiple of 4";
    case BFQ_UBAM_E_GZIP: snprintf(b, sizeof b, "FASTQ to BAM: text %u is compressed (it begins with 1f 8b): inflate the text first", E.k); return b;
    case BFQ_UBAM_E_PAIRS: snprintf(b, sizeof b, "FASTQ to BAM: text 1 holds %llu reads, text 2 holds %llu", E.n, E.m); return b;
    case BFQ_UBAM_E_RG: return "FASTQ to BAM: rg_id: empty, longer than 255 bytes, or a byte outside [ -~]";
    case BFQ_UBAM_E_LEVEL: return "level: 0 (every member stored) or 1 (the compressor)";
    case BFQ_UBAM_E_HEADER: return "FASTQ to BAM: header_text of 2^31 bytes or more, or NULL with a length";
    default: return "ok";
    }
    snprintf(b, sizeof b, "FASTQ to BAM: text %u read %llu: %s", E.k, E.i, why);
    return b;
}
static_assert(BFQ_MAX_READ_LEN == 65000, "the message's number");

// What both passes are given: the texts and their line index, the read counts, the tag every record ends with (tag[0,
// tagLen): "RGZ<rg_id>\0", or none), the options.
struct bfq_ubam_job { bfq_bam_texts T; u64 npairs, n0; const u8 *tag; u32 tagLen, mateSuffix, pairedCheck, pad; };
// the lanes' counts of the writing pass / of the sizing pass
struct bfq_ubam_cnt { u64 named, comments, unknown, pad; };
// How the nl lanes of a record agree: the host's one lane with itself.  (The device's wave64: k_ubam.hip.)
struct bfq_ubam_alone {
    static BFQ_HD u32 first(bool v) { return v ? 0u : 1u; }        // the lowest lane whose v holds; nl: none
    static BFQ_HD bool any(bool v) { return v; }
};
// the tag selection of a call (on == 0: tags off; dropRG: rg_id is set) and what the sizing pass counts
struct bfq_ubam_tagsel { u32 on, n, dropRG, pad; u8 tag[32][2]; };
struct bfq_ubam_tcnt { u64 written, dropped, bytes, pad; };

// unaligned 8- and 4-byte accesses (the device takes them as they are; the host through memcpy)
BFQ_HD u64 bfq_ubam_ld64(const u8 *p) { u64 v; __builtin_memcpy(&v, p, 8); return v; }
BFQ_HD void bfq_ubam_st64(u8 *p, u64 v) { __builtin_memcpy(p, &v, 8); }
BFQ_HD void bfq_ubam_st32(u8 *p, u32 v) { __builtin_memcpy(p, &v, 4); }

// record r of the file: read *i of text *k
BFQ_HD void bfq_ubam_where(const bfq_ubam_job &J, u64 r, u32 *k, u64 *i)
{
    if (r < 2 * J.npairs) { *k = 1u + (u32)(r & 1u); *i = r >> 1; }
    else { *k = 0; *i = r - 2 * J.npairs; }
}
BFQ_HD u32 bfq_ubam_flag(u32 k) { return k == 0 ? 4u : k == 1 ? 77u : 141u; }
BFQ_HD u32 bfq_ubam_digits(u64 v) { u32 d = 1; while (v >= 10) { v /= 10; d++; } return d; }
BFQ_HD u64 bfq_ubam_index(const bfq_ubam_job &J, u32 k, u64 i) { return (k ? i : J.npairs + i) + 1; }   // the number an empty name becomes

// The nibble of a base: 4 bits per letter of the alphabet in two words, a bit per letter that has one.
constexpr u64 bfq_ubam_nib_tab(int half)
{
    const char *s = "=ACMGRSVTWYHKDBN";
    u64 t = ~0ull;                                                  // 15 everywhere
    for (int n = 1; n < 16; n++) {
        const int idx = s[n] - 'A' + 1;
        if (idx / 16 == half) t = (t & ~(15ull << (4 * (idx % 16)))) | ((u64)n << (4 * (idx % 16)));
    }
    return t;
}
constexpr u32 bfq_ubam_known_mask()
{
    const char *s = "=ACMGRSVTWYHKDBN";
    u32 m = 0;
    for (int n = 1; n < 16; n++) m |= 1u << (s[n] - 'A' + 1);
    return m;
}
BFQ_HD u32 bfq_ubam_nibble(u32 ch, u32 *unknown)
{
    constexpr u64 lo = bfq_ubam_nib_tab(0), hi = bfq_ubam_nib_tab(1);
    constexpr u32 known = bfq_ubam_known_mask();
    const u32 up = ch & 0xDFu, idx = up & 31u;
    const bool letter = up - 'A' < 26u && ((known >> idx) & 1u);
    const u32 n = (u32)((idx < 16 ? lo >> (4 * idx) : hi >> (4 * (idx - 16))) & 15u);
    *unknown = letter || ch == '=' ? 0u : 1u;
    return letter ? n : ch == '=' ? 0u : 15u;
}

// The name of a header line t[s0, e0) of text k, by one lane: 0, or why it is refused.  *ns: where it starts; *nl: its
// length, the suffix removed (0: an empty name); *comment: the line goes on behind it.
BFQ_HD u32 bfq_ubam_name(const u8 *t, u64 s0, u64 e0, u32 k, u32 mateSuffix, u64 *ns, u32 *nl, u32 *comment)
{
    if (e0 == s0 || t[s0] != '@') return BFQ_UBAM_E_HDR;
    const u64 b = s0 + 1, lim = e0 - b > BFQ_UBAM_MAX_NAME + 1 ? b + BFQ_UBAM_MAX_NAME + 1 : e0;
    u64 p = b;
    while (p < lim && t[p] != ' ' && t[p] != '\t') p++;
    u32 n = (u32)(p - b);
    if (n > BFQ_UBAM_MAX_NAME) return BFQ_UBAM_E_NAME_LONG;
    *comment = p < e0 ? 1u : 0u;
    if (mateSuffix && k && n > 2 && t[b + n - 2] == '/' && t[b + n - 1] == (u8)('0' + k)) n -= 2;
    for (u32 j = 0; j < n; j++) {
        const u8 ch = t[b + j];
        if (ch < 33 || ch > 126 || ch == '@') return BFQ_UBAM_E_NAME_BYTE;
    }
    *ns = b; *nl = n;
    return BFQ_UBAM_OK;
}

// ---------------------------------------------------------------- tags out of the header line
// where the field that starts at t[fs] ends: the first tab at or behind fs, or e0.  The nl lanes look at a byte each.
template <class W> BFQ_HD u64 bfq_ubam_field_end(const u8 *t, u64 fs, u64 e0, u32 lane, u32 nl)
{
    for (u64 base = fs;; base += nl) {
        const u64 q = base + lane;
        const u32 f = W::first(q >= e0 || t[q] == '\t');
        if (f < nl) return base + f;
    }
}
// One field: type 0: dropped; else the tag's key, its stored type, its bytes in the record (stored), where its value
// stands in the text (val, vlen) and an integer's value (num, two's complement).
struct bfq_ubam_fld { u32 k0, k1, type, stored, vlen, num; u64 val; };
// The field t[fs, fe), by nl lanes that all take the same path: they share the bytes of a Z / H value; everything else is
// the same few loads in every lane.
template <class W> BFQ_HD void bfq_ubam_field(const u8 *t, u64 fs, u64 fe, const bfq_ubam_tagsel &G, u32 lane, u32 nl, bfq_ubam_fld *F)
{
    F->type = 0; F->stored = 0; F->vlen = 0; F->num = 0; F->val = fs;
    if (fe - fs < 5) return;
    const u32 k0 = t[fs], k1 = t[fs + 1], ty = t[fs + 3];
    if (!bfq_bam_key_ok(k0, k1) || t[fs + 2] != ':' || t[fs + 4] != ':') return;
    if (G.dropRG && k0 == 'R' && k1 == 'G') return;
    if (G.n) {
        bool in = false;
        for (u32 j = 0; j < G.n; j++) in = in || (G.tag[j][0] == k0 && G.tag[j][1] == k1);
        if (!in) return;
    }
    const u64 v = fs + 5, vl = fe - v;
    F->k0 = k0; F->k1 = k1; F->val = v;
    if (ty == 'A') {
        if (vl != 1 || t[v] < 0x20 || t[v] > 0x7e) return;
        F->type = 'A'; F->stored = 4;
    } else if (ty == 'i') {
        const u32 neg = vl && t[v] == '-' ? 1u : 0u;
        if (vl < 1 + neg || vl > 10 + neg) return;
        u64 a = 0;
        for (u64 j = neg; j < vl; j++) {
            const u32 d = (u32)t[v + j] - '0';
            if (d > 9) return;
            a = a * 10 + d;
        }
        if (a > (neg ? 2147483648ull : 4294967295ull)) return;
        u32 w;
        if (!neg || !a) { F->type = a <= 255 ? 'C' : a <= 65535 ? 'S' : 'I'; w = a <= 255 ? 1 : a <= 65535 ? 2 : 4; F->num = (u32)a; }
        else { F->type = a <= 128 ? 'c' : a <= 32768 ? 's' : 'i'; w = a <= 128 ? 1 : a <= 32768 ? 2 : 4; F->num = 0u - (u32)a; }
        F->stored = 3 + w;
    } else if (ty == 'Z' || ty == 'H') {
        if (vl > BFQ_UBAM_MAX_FIELD || (ty == 'H' && (vl & 1))) return;
        bool bad = false;
        for (u64 j = lane; j < vl; j += nl) {
            const u32 ch = t[v + j];
            bad = bad || (ty == 'Z' ? ch < 0x20u || ch > 0x7eu : !(ch - '0' < 10u || (ch | 32u) - 'a' < 6u));
        }
        if (W::any(bad)) return;
        F->type = ty; F->vlen = (u32)vl; F->stored = 4 + (u32)vl;
    }
}
// The fields of the header line t[., e0) behind the name, which ends at p, by nl lanes.  each(F, at): called for every
// field that becomes a tag, at byte `at` of the record's tags.  Returns the tags' bytes; *dropped: the fields that did not
// become one; *junk: some byte behind the name did not become a tag.
template <class W, class Each> BFQ_HD u32 bfq_ubam_fields(const u8 *t, u64 p, u64 e0, const bfq_ubam_tagsel &G, u32 lane, u32 nl, u32 *dropped, u32 *junk, Each &&each)
{
    u32 bytes = 0;
    *dropped = 0; *junk = 0;
    if (p < e0 && t[p] == ' ') { *junk = 1; p = bfq_ubam_field_end<W>(t, p, e0, lane, nl); }
    while (p < e0) {                                                // t[p] is a tab
        const u64 fs = p + 1, fe = bfq_ubam_field_end<W>(t, fs, e0, lane, nl);
        bfq_ubam_fld F;
        bfq_ubam_field<W>(t, fs, fe, G, lane, nl, &F);
        if (F.type && bytes + F.stored <= BFQ_UBAM_MAX_TAGS) { each(F, bytes); bytes += F.stored; }
        else { (*dropped)++; *junk = 1; }
        p = fe;
    }
    return bytes;
}

// The sizing pass of read i of text k, by one lane: 0 and *size (the record's bytes, block_size included), or why the read
// is refused.  C: this lane's counts (named, comments).  Reads the header line's first 256 bytes, the mate's with
// pairedCheck, the first byte of the third line and the quality line; writes nothing.  TAGS: it walks the whole header
// line, validates every field and adds the tags' stored bytes to the size (T: this lane's tag counts).
template <bool TAGS = false>
BFQ_HD u32 bfq_ubam_size_read(const bfq_ubam_job &J, u32 k, u64 i, u32 *size, bfq_ubam_cnt *C, const bfq_ubam_tagsel *G = nullptr, bfq_ubam_tcnt *T = nullptr)
{
    const u8 *t = J.T.text[k];
    const u64 *le = J.T.lineEnd[k];
    u64 s0, e0, s1, e1, s2, e2, s3, e3, ns = 0;
    u32 nl = 0, comment = 0;
    bfq_bamp_line(t, le, 4 * i, &s0, &e0);
    u32 why = bfq_ubam_name(t, s0, e0, k, J.mateSuffix, &ns, &nl, &comment);
    if (why) return why;
    if (J.pairedCheck && k == 1) {
        const u8 *t2 = J.T.text[2];
        u64 m0, f0, ms = 0;
        u32 ml = 0, mc = 0;
        bfq_bamp_line(t2, J.T.lineEnd[2], 4 * i, &m0, &f0);
        bool same = bfq_ubam_name(t2, m0, f0, 2, J.mateSuffix, &ms, &ml, &mc) == BFQ_UBAM_OK && ml == nl;
        for (u32 j = 0; same && j < nl; j++) same = t[ns + j] == t2[ms + j];
        if (!same) return BFQ_UBAM_E_PAIR_NAME;
    }
    bfq_bamp_line(t, le, 4 * i + 2, &s2, &e2);
    if (e2 == s2 || t[s2] != '+') return BFQ_UBAM_E_PLUS;
    bfq_bamp_line(t, le, 4 * i + 1, &s1, &e1);
    bfq_bamp_line(t, le, 4 * i + 3, &s3, &e3);
    const u64 L = e1 - s1;
    if (e3 - s3 != L) return BFQ_UBAM_E_FASTQ;
    if (L > BFQ_MAX_READ_LEN) return BFQ_UBAM_E_TOO_LONG;
    u64 p = s3;
    u32 bad = 0;
    for (; p + 8 <= e3; p += 8) {                                   // eight at a time: a byte is bad when byte - 33 > 93
        u64 w = bfq_ubam_ld64(t + p);
        for (int j = 0; j < 8; j++, w >>= 8) bad |= ((u32)(w & 0xFFu) - 33u > 93u) ? 1u : 0u;
    }
    for (; p < e3; p++) bad |= ((u32)t[p] - 33u > 93u) ? 1u : 0u;
    if (bad) return BFQ_UBAM_E_QUAL;
    if (!nl) { nl = bfq_ubam_digits(bfq_ubam_index(J, k, i)); C->named++; }
    u32 tagBytes = 0;
    if constexpr (TAGS) {
        u64 p = s0 + 1;
        while (p < e0 && t[p] != ' ' && t[p] != '\t') p++;          // (the name's end: within 255 bytes, or the read was refused)
        u32 dropped = 0, written = 0;
        tagBytes = bfq_ubam_fields<bfq_ubam_alone>(t, p, e0, *G, 0, 1, &dropped, &comment, [&](const bfq_ubam_fld &, u32) { written++; });
        T->written += written; T->dropped += dropped; T->bytes += tagBytes;
    }
    C->comments += comment;
    *size = (u32)(36u + nl + 1u + (u32)((L + 1) / 2) + (u32)L + tagBytes + J.tagLen);
    return BFQ_UBAM_OK;
}

// Word j (0..8) of a record's first 36 bytes.
BFQ_HD u32 bfq_ubam_fixed(u32 j, u32 size, u32 nameLen, u32 flag, u32 lseq)
{
    return j == 0 ? size - 4u : j == 3 ? (nameLen + 1u) | (4680u << 16) : j == 4 ? flag << 16 : j == 5 ? lseq : j == 8 ? 0u : 0xFFFFFFFFu;
}

// The writing pass of read i of text k (passed by the sizing pass) at out[o, o + size), by nl lanes of which this is lane
// `lane`.  The first nine lanes store the fixed fields, a word each; the lanes share the name's bytes; a lane owns whole
// bytes of SEQ -- two bases, neighbouring bytes of the text -- and whole bytes of QUAL, four and eight at a time where the
// destination is aligned (the text is read unaligned), byte by byte in front of and behind that; the tag's bytes last.  No
// two lanes write one byte, no lane walks a read, and every byte of the record is written.  *unknown: this lane's count.
// TAGS: the fields of the header line that the sizing pass took stand between QUAL and that tag: the lanes share a Z / H
// value's bytes; a tag's three leading bytes, its NUL and the <= 4 bytes of an integer are lane 0's.
template <class W, bool TAGS = false>
BFQ_HD void bfq_ubam_write_rec(u8 *out, u64 o, u32 size, const bfq_ubam_job &J, u32 k, u64 i, u32 lane, u32 nl, u64 *unknown, const bfq_ubam_tagsel *G = nullptr)
{
    const u8 *t = J.T.text[k];
    const u64 *le = J.T.lineEnd[k];
    u64 s0, e0, s1, e1, s3, e3;
    bfq_bamp_line(t, le, 4 * i, &s0, &e0);
    bfq_bamp_line(t, le, 4 * i + 1, &s1, &e1);
    bfq_bamp_line(t, le, 4 * i + 3, &s3, &e3);
    const u32 L = (u32)(e1 - s1);
    // the name's end: the lanes look at a byte each
    const u64 b = s0 + 1;
    u32 n = 0;
    for (u32 base = 0;; base += nl) {
        const u64 p = b + base + lane;
        const bool stop = p >= e0 || t[p] == ' ' || t[p] == '\t';
        const u32 f = W::first(stop);
        if (f < nl) { n = base + f; break; }
    }
    const u64 nameEnd = b + n;
    if (J.mateSuffix && k && n > 2 && t[b + n - 2] == '/' && t[b + n - 1] == (u8)('0' + k)) n -= 2;
    const u64 number = bfq_ubam_index(J, k, i);
    const u32 nameLen = n ? n : bfq_ubam_digits(number);
    u8 *r = out + o;
    for (u32 j = lane; j < 9; j += nl) bfq_ubam_st32(r + 4 * j, bfq_ubam_fixed(j, size, nameLen, bfq_ubam_flag(k), L));
    u8 *name = r + 36;
    if (n) {
        for (u32 j = lane; j <= n; j += nl) name[j] = j < n ? t[b + j] : (u8)0;
    } else {
        for (u32 j = lane; j <= nameLen; j += nl) {
            u64 v = number;
            for (u32 d = j + 1; d < nameLen; d++) v /= 10;
            name[j] = j < nameLen ? (u8)('0' + v % 10) : (u8)0;
        }
    }
    // SEQ
    u8 *seq = name + nameLen + 1;
    const u32 nb = (L + 1) / 2, full = L / 2;                       // bytes of SEQ; those of two bases
    u32 head = (u32)((0 - (uintptr_t)seq) & 3u);
    if (head > full) head = full;
    const u32 nw = (full - head) / 4, tail = head + 4 * nw;
    u32 unk = 0, u1, u2;
    for (u32 j = lane; j < head; j += nl) {
        const u32 hi = bfq_ubam_nibble(t[s1 + 2 * j], &u1), lo = bfq_ubam_nibble(t[s1 + 2 * j + 1], &u2);
        seq[j] = (u8)((hi << 4) | lo); unk += u1 + u2;
    }
    for (u32 w = lane; w < nw; w += nl) {
        u64 x = bfq_ubam_ld64(t + s1 + 2 * (u64)(head + 4 * w));
        u32 v = 0;
        for (int j = 0; j < 4; j++, x >>= 16) {
            const u32 hi = bfq_ubam_nibble((u32)(x & 0xFFu), &u1), lo = bfq_ubam_nibble((u32)((x >> 8) & 0xFFu), &u2);
            v |= ((hi << 4) | lo) << (8 * j); unk += u1 + u2;
        }
        bfq_ubam_st32(seq + head + 4 * w, v);
    }
    for (u32 j = tail + lane; j < nb; j += nl) {
        const u32 hi = bfq_ubam_nibble(t[s1 + 2 * j], &u1);
        u32 lo = 0;
        u2 = 0;
        if (2 * j + 1 < L) lo = bfq_ubam_nibble(t[s1 + 2 * j + 1], &u2);
        seq[j] = (u8)((hi << 4) | lo); unk += u1 + u2;
    }
    *unknown += unk;
    // QUAL
    u8 *qual = seq + nb;
    u32 qh = (u32)((0 - (uintptr_t)qual) & 7u);
    if (qh > L) qh = L;
    const u32 qw = (L - qh) / 8, qt = qh + 8 * qw;
    for (u32 j = lane; j < qh; j += nl) qual[j] = (u8)(t[s3 + j] - 33);
    for (u32 w = lane; w < qw; w += nl) bfq_ubam_st64(qual + qh + 8 * w, bfq_ubam_ld64(t + s3 + qh + 8 * (u64)w) - 0x2121212121212121ull);   // (every byte >= 33: no borrow)
    for (u32 j = qt + lane; j < L; j += nl) qual[j] = (u8)(t[s3 + j] - 33);
    u8 *tag = qual + L;
    if constexpr (TAGS) {
        u32 dropped, junk;
        u8 *const first = tag;
        tag += bfq_ubam_fields<W>(t, nameEnd, e0, *G, lane, nl, &dropped, &junk, [&](const bfq_ubam_fld &F, u32 at) {
            u8 *d = first + at;
            const bool str = F.type == 'Z' || F.type == 'H';
            if (str)
                for (u32 j = lane; j < F.vlen; j += nl) d[3 + j] = t[F.val + j];
            if (lane == 0) {
                d[0] = (u8)F.k0; d[1] = (u8)F.k1; d[2] = (u8)F.type;
                if (str) d[3 + F.vlen] = 0;
                else if (F.type == 'A') d[3] = t[F.val];
                else
                    for (u32 j = 0; j + 3 < F.stored; j++) d[3 + j] = (u8)(F.num >> (8 * j));
            }
        });
    }
    for (u32 j = lane; j < J.tagLen; j += nl) tag[j] = J.tag[j];
}

// ---------------------------------------------------------------- host side
// The options of a call as both forms take them: the defaults for a null pointer, *E for what is refused.
inline void bfq_ubam_defaults(bfq_ubam_opts *o) { *o = bfq_ubam_opts{}; o->mate_suffix = 1; o->level = 1; }
inline bool bfq_ubam_resolve(const bfq_ubam_opts *in, bfq_ubam_opts *O, bfq_ubam_err *E)
{
    bfq_ubam_defaults(O);
    if (in) *O = *in;
    if (O->rg_id) {
        const size_t n = strlen(O->rg_id);
        bool ok = n >= 1 && n <= 255;
        for (size_t j = 0; ok && j < n; j++) ok = (u8)O->rg_id[j] >= 32 && (u8)O->rg_id[j] <= 126;
        if (!ok) { E->kind = BFQ_UBAM_E_RG; return false; }
    }
    if (O->level > 1) { E->kind = BFQ_UBAM_E_LEVEL; return false; }
    if (O->header_len >= (1ull << 31) || (!O->header_text && O->header_len)) { E->kind = BFQ_UBAM_E_HEADER; return false; }
    return true;
}
// the tag selection of a call: off unless in->reserved holds BFQ_UBAM_OPTS_TAGS; false: refused (*why)
inline bool bfq_ubam_tags_resolve(const bfq_ubam_opts *in, bfq_ubam_tagsel *G, bfq_ubam_tag_stats **stats, const char **why)
{
    memset(G, 0, sizeof *G);
    *stats = nullptr; *why = nullptr;
    if (!in || in->reserved != BFQ_UBAM_OPTS_TAGS) return true;
    const bfq_ubam_tag_opts *X = (const bfq_ubam_tag_opts *)in;
    if (X->n_tags > 32) { *why = "FASTQ to BAM: tags: more than 32 tags"; return false; }
    for (u32 j = 0; j < X->n_tags; j++) {
        if (!bfq_bam_key_ok(X->tag[j][0], X->tag[j][1])) { *why = "FASTQ to BAM: tags: a tag that is not [A-Za-z][A-Za-z0-9]"; return false; }
        G->tag[j][0] = X->tag[j][0]; G->tag[j][1] = X->tag[j][1];
    }
    G->on = 1; G->n = X->n_tags; G->dropRG = in->rg_id ? 1u : 0u;
    *stats = X->stats;
    return true;
}
// the stream's header and the tag of every record
inline std::vector<u8> bfq_ubam_header(const bfq_ubam_opts &O)
{
    std::string text;
    if (O.header_text) text.assign((const char *)O.header_text, (size_t)O.header_len);
    else {
        text = "@HD\tVN:1.6\tSO:unsorted\n";
        if (O.rg_id) text += std::string("@RG\tID:") + O.rg_id + "\n";
    }
    std::vector<u8> h = {'B', 'A', 'M', 1};
    const u32 lt = (u32)text.size();
    for (int j = 0; j < 4; j++) h.push_back((u8)(lt >> (8 * j)));
    h.insert(h.end(), text.begin(), text.end());
    for (int j = 0; j < 4; j++) h.push_back(0);                    // n_ref
    return h;
}
inline std::vector<u8> bfq_ubam_tag(const bfq_ubam_opts &O)
{
    std::vector<u8> g;
    if (!O.rg_id) return g;
    g = {'R', 'G', 'Z'};
    g.insert(g.end(), O.rg_id, O.rg_id + strlen(O.rg_id) + 1);
    return g;
}
// the checks of the texts as a whole, in the order both forms make them; false: *E
inline bool bfq_ubam_gzip_ok(const u8 first[2], u64 len, u32 k, bfq_ubam_err *E)
{
    if (len < 2 || first[0] != 0x1F || first[1] != 0x8B) return true;
    E->kind = BFQ_UBAM_E_GZIP; E->k = k;
    return false;
}
inline bool bfq_ubam_counts_ok(const u64 lines[3], const bool present[3], u64 reads[3], bfq_ubam_err *E)
{
    for (u32 k = 0; k < 3; k++) {
        if (lines[k] % 4) { E->kind = BFQ_UBAM_E_LINES; E->k = k; return false; }
        reads[k] = lines[k] / 4;
    }
    if (reads[1] != reads[2] || present[1] != present[2]) { E->kind = BFQ_UBAM_E_PAIRS; E->n = reads[1]; E->m = reads[2]; return false; }
    return true;
}
// what a refusal found by the sizing pass says: record r of the file, reason why
inline void bfq_ubam_read_err(const bfq_ubam_job &J, u64 r, u32 why, bfq_ubam_err *E)
{
    E->kind = why;
    bfq_ubam_where(J, r, &E->k, &E->i);
}
inline void bfq_ubam_totals(const bfq_ubam_job &J, u64 rawLen, const bfq_ubam_cnt &C, bfq_ubam_stats *S)
{
    *S = bfq_ubam_stats{};
    S->records = 2 * J.npairs + J.n0;
    S->written[0] = J.n0; S->written[1] = S->written[2] = J.npairs;
    S->named = C.named; S->comments_dropped = C.comments; S->unknown_bases = C.unknown;
    S->raw_len = rawLen; S->members = (rawLen + BFQ_UBAM_PIECE - 1) / BFQ_UBAM_PIECE + 1;
}

// The host form: the same steps by one thread.  text[k] (nullptr: absent) of textLen[k] bytes; O: resolved options;
// out[0, cap): where the stream goes (measure: not touched).  Returns 0; 2 = refused (*X); 3 = cap below the length
// (S->raw_len: the length).  Nothing is written unless 0 is returned.
inline int bfq_ubam_host_form(const u8 *const text[3], const u64 textLen[3], const bfq_ubam_opts &O, u8 *out, u64 cap, bool measure, bfq_ubam_stats *S,
                              bfq_ubam_err *X, const bfq_ubam_tagsel *G = nullptr, bfq_ubam_tag_stats *TS = nullptr)
{
    const bool tags = G && G->on;
    bfq_ubam_tcnt TC{};
    *S = bfq_ubam_stats{};
    *X = bfq_ubam_err{};
    bool present[3];
    for (u32 k = 0; k < 3; k++) {
        present[k] = text[k] != nullptr;
        if (present[k] && !bfq_ubam_gzip_ok(text[k], textLen[k], k, X)) return 2;
    }
    std::vector<u64> lineEnd[3];
    u64 lines[3] = {0, 0, 0}, reads[3] = {0, 0, 0};
    bfq_ubam_job J{};
    for (u32 k = 0; k < 3; k++) {
        if (!present[k]) continue;
        for (u64 p = 0; p < textLen[k]; p++)
            if (text[k][p] == 10) lineEnd[k].push_back(p);
        if (textLen[k] && text[k][textLen[k] - 1] != 10) lineEnd[k].push_back(textLen[k]);
        lines[k] = lineEnd[k].size();
        J.T.text[k] = text[k]; J.T.lineEnd[k] = lineEnd[k].data(); J.T.len[k] = textLen[k];
    }
    if (!bfq_ubam_counts_ok(lines, present, reads, X)) return 2;
    const std::vector<u8> hdr = bfq_ubam_header(O), tag = bfq_ubam_tag(O);
    J.npairs = reads[1]; J.n0 = reads[0];
    J.tag = tag.data(); J.tagLen = (u32)tag.size(); J.mateSuffix = O.mate_suffix; J.pairedCheck = O.paired_check;
    const u64 nrec = 2 * J.npairs + J.n0;
    std::vector<u64> off(nrec + 1);
    bfq_ubam_cnt C{};
    u64 at = hdr.size();
    for (u64 r = 0; r < nrec; r++) {
        u32 k, size = 0;
        u64 i;
        bfq_ubam_where(J, r, &k, &i);
        const u32 why = tags ? bfq_ubam_size_read<true>(J, k, i, &size, &C, G, &TC) : bfq_ubam_size_read(J, k, i, &size, &C);
        if (why) { bfq_ubam_read_err(J, r, why, X); return 2; }
        off[r] = at;
        at += size;
    }
    off[nrec] = at;
    bfq_ubam_totals(J, at, C, S);
    if (tags && TS) { TS->tags_written = TC.written; TS->fields_dropped = TC.dropped; TS->tag_bytes = TC.bytes; }
    if (measure) return 0;
    if (cap < at) return 3;
    memcpy(out, hdr.data(), hdr.size());
    for (u64 r = 0; r < nrec; r++) {
        u32 k;
        u64 i;
        bfq_ubam_where(J, r, &k, &i);
        if (tags) bfq_ubam_write_rec<bfq_ubam_alone, true>(out, off[r], (u32)(off[r + 1] - off[r]), J, k, i, 0, 1, &C.unknown, G);
        else bfq_ubam_write_rec<bfq_ubam_alone>(out, off[r], (u32)(off[r + 1] - off[r]), J, k, i, 0, 1, &C.unknown);
    }
    S->unknown_bases = C.unknown;
    return 0;
}
