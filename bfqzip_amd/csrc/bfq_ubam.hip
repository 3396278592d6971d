// bfq_ubam.hip -- unaligned BAM output (include/bfqzip_hip.h, bfq_fastq_to_bam*): the host side of turning FASTQ texts
// into BAM records.  The definition and both passes are bfq_ubam.h's; the kernels are k_ubam.hip's.  One call:
//   1  every present text uploaded into the context's text buffer -- or taken where it lies on the device --, its lines
//      counted there, the arena reserved from the counts, the texts indexed (bfq_line_index)
//   2  the sizing pass, one lane per read, and an exclusive prefix sum over the sizes in file order: the stream's exact length;
//      a refusal is the lowest (record, reason) the pass reported
//   3  the header uploaded, the writing pass
//   4  bfq_fastq_to_bam / _fd / bfq_fastq_restore_bam_fd: the stream deflated where it lies (bfq_deflate_core): it never
//      crosses to the host uncompressed
//   arena   8 bytes per text line (and 12 per 4 KiB of text while they are indexed), 12 bytes per record, the stream -- before
//           the sizing pass bounded by the texts' bytes + 53 + the tag per read (with tags out of the header line too: no
//           field is longer stored than written, bfq_ubam.h goes through the types) --, the deflate batch; all reserved at once.
//           Uploaded texts lie in the context's text buffer, beside the arena, like the text of every FASTQ entry point.
// bfq_fastq_to_bam_host is the host form of bfq_ubam.h, for tests and as the statement of the algorithm: no entry point
// here falls back to it.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include "bfq_internal.h"
#include "bfq_deflate.h"
#include "bfq_ubam.h"

static_assert(sizeof(bfq_ubam_stats) == 72 && sizeof(bfq_ubam_opts) == 40 && BFQ_UBAM_PIECE == BFQ_DEFL_PIECE, "the C-ABI's structures; the member size");

void bfq_ubam_launch_size(bfq_ctx *c, const bfq_ubam_job &J, u64 nrec, u32 *d_sizes, u64 *d_firstBad, bfq_ubam_cnt *d_cnt, const bfq_ubam_tagsel &G,
                          bfq_ubam_tcnt *d_tcnt);                                                                                           // k_ubam.hip
void bfq_ubam_launch_write(bfq_ctx *c, const bfq_ubam_job &J, u64 nrec, const u64 *d_off, u8 *d_out, u64 rawLen, bfq_ubam_cnt *d_cnt, const bfq_ubam_tagsel &G);

#define UBAM_NONE (~0ull)

static void ubam_refuse(const bfq_ubam_err &X) { throw BfqError{bfq_ubam_code(X), bfq_ubam_message(X)}; }
static bfq_ubam_opts ubam_opts(const bfq_ubam_opts *in)
{
    bfq_ubam_opts O;
    bfq_ubam_err X;
    if (!bfq_ubam_resolve(in, &O, &X)) ubam_refuse(X);
    return O;
}

// the tag selection of a call (off without the extension); *stats: where its counts go (zeroed here: a refused call leaves them 0)
static bfq_ubam_tagsel ubam_tags(const bfq_ubam_opts *in, bfq_ubam_tag_stats **stats)
{
    bfq_ubam_tagsel G;
    const char *why = nullptr;
    if (!bfq_ubam_tags_resolve(in, &G, stats, &why)) throw BfqError{BFQ_E_ARG, why};
    if (*stats) **stats = bfq_ubam_tag_stats{};
    return G;
}

extern "C" void bfq_ubam_default_opts(bfq_ubam_opts *o) { if (o) bfq_ubam_defaults(o); }

static thread_local std::string g_ubamHostErr;
extern "C" const char *bfq_ubam_host_error(void) { return g_ubamHostErr.c_str(); }

extern "C" int bfq_fastq_to_bam_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *out_raw, uint64_t cap,
                                     uint64_t *raw_len, bfq_ubam_stats *stats)
{
    if (raw_len) *raw_len = 0;
    if (stats) *stats = bfq_ubam_stats{};
    return host_guarded(g_ubamHostErr, [&] {
        if (!text || !text_len || !raw_len || (!out_raw && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_ubam_opts O = ubam_opts(opts);
        bfq_ubam_tag_stats *tagStats = nullptr, TS{};
        const bfq_ubam_tagsel G = ubam_tags(opts, &tagStats);
        const u64 tl[3] = {text[0] ? text_len[0] : 0, text[1] ? text_len[1] : 0, text[2] ? text_len[2] : 0};
        bfq_ubam_stats S;
        bfq_ubam_err X;
        const int r = bfq_ubam_host_form(text, tl, O, out_raw, cap, false, &S, &X, &G, &TS);
        if (r == 2) ubam_refuse(X);
        if (tagStats) *tagStats = TS;
        *raw_len = S.raw_len;
        if (r == 3) throw BfqError{BFQ_E_ARG, "output buffer too small for the stream"};
        if (stats) *stats = S;
    });
}

// what steps 1-3 leave: the stream in the arena and the counts
struct UbamStream { u8 *d_s = nullptr; u64 raw = 0; bfq_ubam_stats S{}; bfq_ubam_tag_stats T{}; };

// arena bytes of a text's line index here, generously: `bytes` is the length of all texts of the call, not of this one (the
// restore path knows only a bound), and 8 KiB of slack go with each text for the small buffers between the indexes
static size_t ubam_index_bytes(u64 bytes, u64 lines) { return bfq_line_index_bytes(bytes, lines) + 8192; }
// arena bytes of steps 1-3 (behind the counting of the lines) for texts of `bytes` bytes and at most `lines` lines in all,
// whose line indexes take `index` bytes; + extra(bound of the stream).  (The scan over the sizes: twice over, and 4 KiB.)
static size_t ubam_need(u64 bytes, u64 lines, size_t index, size_t hdrLen, size_t tagLen, bool stream, u64 *rawBound)
{
    const u64 nrec = lines / 4 + 3;
    *rawBound = hdrLen + bytes + nrec * (53 + tagLen) + 64;
    return index + 12 * (size_t)(nrec + 2) + 2 * bfq_scan_bytes(nrec) + 4096 + (stream ? (size_t)*rawBound : 0) + tagLen + (64u << 10);
}

// Steps 2-3 on texts that stand on the device at 16-byte aligned addresses (T[k].d; nullptr: absent), in an arena that holds
// ubam_need() bytes above its top.  sized(raw) runs once the stream's length is known and before anything is written: it
// throws for a short capacity.
static void ubam_records(bfq_ctx *c, const TextPlaced T[3], const bfq_ubam_opts &O, const bfq_ubam_tagsel &G, bool measure, const std::function<void(u64)> &sized,
                         UbamStream *out)
{
    bfq_ubam_err R;
    bfq_ubam_job J{};
    u64 lines[3] = {0, 0, 0}, reads[3] = {0, 0, 0};
    const bool present[3] = {T[0].d != nullptr, T[1].d != nullptr, T[2].d != nullptr};
    for (u32 k = 0; k < 3; k++) {
        if (!present[k]) continue;
        J.T.text[k] = T[k].d; J.T.len[k] = T[k].len;
        J.T.lineEnd[k] = bfq_line_index(c, T[k].d, T[k].len, &lines[k]);
    }
    if (!bfq_ubam_counts_ok(lines, present, reads, &R)) { c->profCollect(); ubam_refuse(R); }
    const std::vector<u8> hdr = bfq_ubam_header(O), tag = bfq_ubam_tag(O);
    J.npairs = reads[1]; J.n0 = reads[0];
    J.tagLen = (u32)tag.size(); J.mateSuffix = O.mate_suffix; J.pairedCheck = O.paired_check;
    const u64 nrec = 2 * J.npairs + J.n0;
    u8 *d_tag = c->alloc<u8>(tag.size() + 16);
    if (!tag.empty()) bfq_upload(c, d_tag, tag.data(), tag.size());
    J.tag = d_tag;
    u32 *d_sizes = c->alloc<u32>(nrec + 1);
    u64 *d_off = c->alloc<u64>(nrec + 2);
    u64 *d_bad = c->alloc<u64>(1);
    bfq_ubam_cnt *d_cnt = c->alloc<bfq_ubam_cnt>(2);                // (the tag counts behind the counts: both are 32 bytes)
    bfq_ubam_tcnt *d_tcnt = (bfq_ubam_tcnt *)(d_cnt + 1);
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    HIP_CHECK(hipMemsetAsync(d_cnt, 0, 2 * sizeof(bfq_ubam_cnt), c->stream));
    bfq_ubam_launch_size(c, J, nrec, d_sizes, d_bad, d_cnt, G, d_tcnt);
    bfq_exscan_u32(c, d_sizes, d_off, nrec, d_off + nrec);
    u64 firstBad = UBAM_NONE, total = 0;
    bfq_ubam_cnt C{};
    bfq_ubam_tcnt TC{};
    if (G.on) HIP_CHECK(hipMemcpyAsync(&TC, d_tcnt, sizeof TC, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&firstBad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&total, d_off + nrec, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&C, d_cnt, sizeof C, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (firstBad != UBAM_NONE) {
        c->profCollect();
        bfq_ubam_read_err(J, firstBad >> 8, (u32)(firstBad & 0xFFu), &R);
        ubam_refuse(R);
    }
    const u64 raw = hdr.size() + total;
    bfq_ubam_totals(J, raw, C, &out->S);
    out->T.tags_written = TC.written; out->T.fields_dropped = TC.dropped; out->T.tag_bytes = TC.bytes;
    out->raw = raw;
    sized(raw);
    if (measure) { c->profCollect(); return; }
    u8 *d_s = c->alloc<u8>(raw + 64);
    bfq_upload(c, d_s, hdr.data(), hdr.size());
    bfq_ubam_launch_write(c, J, nrec, d_off, d_s + hdr.size(), raw, d_cnt, G);
    HIP_CHECK(hipMemcpyAsync(&C, d_cnt, sizeof C, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                                      // (hdr and tag live till here)
    c->profCollect();
    out->S.unknown_bases = C.unknown;
    out->d_s = d_s;
}

// Steps 1-3.  extra(bound): arena bytes the caller needs behind them for a stream of at most that length.
static void ubam_core(bfq_ctx *c, const TextIn X[3], const bfq_ubam_opts &O, const bfq_ubam_tagsel &G, bool measure, const std::function<size_t(u64)> &extra,
                      const std::function<void(u64)> &sized, UbamStream *out)
{
    bfq_ubam_err R;
    BfqTextSeen seen[3];
    bfq_texts_look(c, X, 3, seen, false);
    for (u32 k = 0; k < 3; k++)
        if (seen[k].present && !bfq_ubam_gzip_ok(seen[k].first, seen[k].len, k, &R)) ubam_refuse(R);
    // Every text's lines, which size its index and the records' arrays, are counted on the device before the arena is reserved.
    TextPlaced T[3];
    bfq_texts_place(c, X, bfq_texts_plan(seen, 3, false), 3, T);
    u64 bytes = 0, lines = 0;
    size_t index = 0;
    for (u32 k = 0; k < 3; k++) { bytes += T[k].len; lines += T[k].lines; }
    for (u32 k = 0; k < 3; k++)
        if (T[k].d) index += ubam_index_bytes(bytes, T[k].lines);
    const std::vector<u8> hdr = bfq_ubam_header(O), tag = bfq_ubam_tag(O);
    u64 bound = 0;
    const size_t need = ubam_need(bytes, lines, index, hdr.size(), tag.size(), !measure, &bound);
    bfq_phase("alloc");
    c->reserve(need + (measure ? 0 : extra(bound)) + (1u << 20));
    bfq_phase("gpu");
    ubam_records(c, T, O, G, measure, sized, out);
}

extern "C" int bfq_fastq_to_bam_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint64_t *raw_len,
                                        uint64_t n_reads[3], bfq_ubam_stats *stats)
{
    if (raw_len) *raw_len = 0;
    if (n_reads) n_reads[0] = n_reads[1] = n_reads[2] = 0;
    if (stats) *stats = bfq_ubam_stats{};
    return guarded(c, [&] {
        if (!h_text || !text_len || !raw_len) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_ubam_opts O = ubam_opts(opts);
        bfq_ubam_tag_stats *tagStats = nullptr;
        const bfq_ubam_tagsel G = ubam_tags(opts, &tagStats);
        TextIn X[3];
        bfq_texts_of(h_text, text_len, false, X);
        UbamStream U;
        ubam_core(c, X, O, G, true, [](u64) { return (size_t)0; }, [](u64) {}, &U);
        if (tagStats) *tagStats = U.T;
        *raw_len = U.raw;
        if (n_reads) for (int k = 0; k < 3; k++) n_reads[k] = U.S.written[k];
        if (stats) *stats = U.S;
    });
}

extern "C" int bfq_fastq_to_bam_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *d_out_raw,
                                       uint64_t cap, uint64_t *raw_len, bfq_ubam_stats *stats)
{
    if (raw_len) *raw_len = 0;
    if (stats) *stats = bfq_ubam_stats{};
    return guarded(c, [&] {
        if (!d_text || !text_len || !raw_len || (!d_out_raw && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_ubam_opts O = ubam_opts(opts);
        bfq_ubam_tag_stats *tagStats = nullptr;
        const bfq_ubam_tagsel G = ubam_tags(opts, &tagStats);
        TextIn X[3];
        bfq_texts_of(d_text, text_len, true, X);
        UbamStream U;
        ubam_core(c, X, O, G, false, [](u64) { return (size_t)0; }, [&](u64 raw) {
            if (cap >= raw) return;
            *raw_len = raw;
            c->profCollect();
            throw BfqError{BFQ_E_ARG, "output buffer too small for the stream"};
        }, &U);
        // (the stream is made in the arena and copied out last: a refusal has then written nothing into the caller's buffer)
        if (U.raw) HIP_CHECK(hipMemcpyAsync(d_out_raw, U.d_s, (size_t)U.raw, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        *raw_len = U.raw;
        if (stats) *stats = U.S;
        if (tagStats) *tagStats = U.T;
    });
}

// host texts in, the compressed file out to dst (memory of cap bytes, or a file)
static void ubam_compressed(bfq_ctx *c, const TextIn X[3], const bfq_ubam_opts *opts, HostRef dst, u64 cap, uint64_t *out_len, bfq_ubam_stats *stats)
{
    const bfq_ubam_opts O = ubam_opts(opts);
    bfq_ubam_tag_stats *tagStats = nullptr;
    const bfq_ubam_tagsel G = ubam_tags(opts, &tagStats);
    UbamStream U;
    ubam_core(c, X, O, G, false, [&](u64 bound) { return bfq_deflate_need(c, bound, false, 0) + 4096; }, [&](u64 raw) {
        if (cap >= bfq_defl_bound(raw)) return;
        *out_len = bfq_defl_bound(raw);
        c->profCollect();
        throw BfqError{BFQ_E_ARG, "output buffer below bfq_bgzf_deflate_bound(raw length)"};
    }, &U);
    *out_len = bfq_deflate_core(c, U.d_s, HostRef{}, U.raw, (int)O.level, dst, true, 0);
    if (stats) *stats = U.S;
    if (tagStats) *tagStats = U.T;
}

extern "C" int bfq_fastq_to_bam(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *h_out, uint64_t cap,
                                uint64_t *out_len, bfq_ubam_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_ubam_stats{};
    return guarded(c, [&] {
        if (!h_text || !text_len || !out_len || (!h_out && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        TextIn X[3];
        bfq_texts_of(h_text, text_len, false, X);
        ubam_compressed(c, X, opts, HostRef::mem(h_out), cap, out_len, stats);
    });
}

extern "C" int bfq_fastq_to_bam_fd(bfq_ctx *c, const int text_fd[3], const bfq_ubam_opts *opts, int out_fd, uint64_t *out_len, bfq_ubam_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_ubam_stats{};
    // the files are mapped, and uploaded from the mappings
    MappedInput text[3];
    return guarded(c, [&] {
        if (!out_len || !text_fd) throw BfqError{BFQ_E_ARG, "null argument"};
        if (out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        TextIn X[3];
        bfq_texts_map(text_fd, text, X);
        try {
            ubam_compressed(c, X, opts, HostRef::file(out_fd, 0), ~0ull, out_len, stats);
            bfq_fd_size(out_fd, *out_len, "cannot size the output file: ", true);
        } catch (...) {
            if (ftruncate(out_fd, 0) != 0) {}
            *out_len = 0;
            if (stats) *stats = bfq_ubam_stats{};
            throw;
        }
    });
}

// For bfq_fastq_restore_bam_fd (bfq_restore.hip), whose arena holds the restored text: the arena bytes the records and the
// deflate batch take above a text of at most `bound` bytes -- a restored read is at least 6 bytes of text in 4 lines --, and
// the text at d_text (in that arena) as an unpaired uBAM to dst.  Returns the file's length.
size_t bfq_ubam_held_need(bfq_ctx *c, u64 bound, const bfq_ubam_opts *opts)
{
    const bfq_ubam_opts O = ubam_opts(opts);
    bfq_ubam_tag_stats *tagStats = nullptr;
    ubam_tags(opts, &tagStats);                                     // (a tag list that is refused: here, before the restore begins)
    u64 rawBound = 0;
    const u64 lines = 4 * (bound / 6 + 1);
    const size_t need = ubam_need(bound, lines, ubam_index_bytes(bound, lines), bfq_ubam_header(O).size(), bfq_ubam_tag(O).size(), true, &rawBound);
    return need + bfq_deflate_need(c, rawBound, false, 0) + 4096;
}
u64 bfq_ubam_held(bfq_ctx *c, const u8 *d_text, u64 len, const bfq_ubam_opts *opts, HostRef dst, bfq_ubam_stats *stats)
{
    const bfq_ubam_opts O = ubam_opts(opts);
    TextPlaced T[3];
    T[0].d = d_text; T[0].len = len;
    bfq_ubam_tag_stats *tagStats = nullptr;
    const bfq_ubam_tagsel G = ubam_tags(opts, &tagStats);
    UbamStream U;
    ubam_records(c, T, O, G, false, [](u64) {}, &U);
    const u64 zl = bfq_deflate_core(c, U.d_s, HostRef{}, U.raw, (int)O.level, dst, true, 0);
    if (stats) *stats = U.S;
    if (tagStats) *tagStats = U.T;
    return zl;
}
