// bfq_bam_patch.hip -- BAM output (include/bfqzip_hip.h, bfq_bam_patch*): the host side of writing FASTQ texts back into
// the records of a BAM file.  The definition and both walks are bfq_bam_patch.h's; the kernels are k_bam_patch.hip's.  One call:
//   1  the stream into the arena, the header, the counting walk and the chain: bfq_bam_chain_device, as on the way in
//   2  every present text uploaded into the context's text buffer -- or taken where it lies on the device --, its lines
//      counted there before the arena is reserved, and indexed (bfq_line_index) once the stream stands
//   3  the checking walk; on a refusal the offending piece is walked once more for the words of the message
//   4  the patching walk, in place on the stream; the pieces' counts down
//   5  bfq_bam_patch / _fd: the stream deflated where it lies (bfq_deflate_core): it never crosses to the host uncompressed
//   arena   the compressed bytes and the stream, 8 bytes per text line (and 12 per 4 KiB of text while they are indexed),
//           232 bytes per piece, the deflate batch; all reserved at once, since growing the arena would lose the stream.
//           Uploaded texts lie in the context's text buffer, beside the arena, like the text of every FASTQ entry point.
// bfq_bam_patch_host is the host form of bfq_bam_patch.h, for tests and as the statement of the algorithm: no entry point
// here falls back to it.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include "bfq_internal.h"
#include "bfq_deflate.h"
#include "bfq_bam_patch.h"

static_assert(sizeof(bfq_bam_patch_stats) == 120 && sizeof(bfq_bamp_cnt) == 64 && sizeof(bfq_bam_opts) == 32, "the C-ABI's structures; 232 bytes per piece");

void bfq_bam_launch_patch_check(bfq_ctx *c, const u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T,
                                u64 only, u64 *d_firstBad, bfq_bamp_err *d_err);                                   // k_bam_patch.hip
void bfq_bam_launch_patch(bfq_ctx *c, u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T, bfq_bamp_cnt *d_cnt);

static void patch_refuse(const bfq_bamp_err &X) { throw BfqError{BFQ_E_ARG, bfq_bamp_message(X)}; }
static void patch_check_level(int level)
{
    if (level != 0 && level != 1) throw BfqError{BFQ_E_ARG, "level: 0 (every member stored) or 1 (the compressor)"};
}

extern "C" int bfq_bam_patch_host(const uint8_t *raw, uint64_t raw_len, const bfq_bam_opts *opts, const uint8_t *const text[3], const uint64_t text_len[3],
                                  uint8_t *out_raw, uint64_t cap, bfq_bam_patch_stats *stats)
{
    if (stats) *stats = bfq_bam_patch_stats{};
    std::string err;
    const int rc = host_guarded(err, [&] {
        if ((!raw && raw_len) || !text || !text_len || (!out_raw && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_bam_opts O = bfq_bam_opts_of(opts);
        static const u8 none = 0;
        bfq_bam_patch_stats PS;
        bfq_bam_err E;
        bfq_bamp_err X;
        const u64 tl[3] = {text_len[0], text_len[1], text_len[2]};
        const int r = bfq_bam_patch_host_form(raw_len ? raw : &none, raw_len, O, text, tl, out_raw, cap, &PS, &E, &X);
        if (r == 1) bfq_bam_refuse(E);
        if (r == 2) patch_refuse(X);
        if (r == 3) {
            if (stats) stats->raw_len = raw_len;
            throw BfqError{BFQ_E_ARG, "output buffer too small for the stream"};
        }
        if (stats) *stats = PS;
    });
    bfq_bam_host_error_set(err);                                    // (the BAM string: bfq_bam_host_error() reports both directions)
    return rc;
}

// Steps 1-4.  extra(raw): arena bytes the caller needs behind them.  *C: the patched stream (d_s, raw).  sized(raw) runs
// once the stream's length is known and before anything is checked against the texts: it throws for a short capacity.
static void patch_core(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts *opts, const TextIn X[3], const std::function<size_t(u64)> &extra,
                       const std::function<void(u64)> &sized, bfq_bam_chain_dev *C, bfq_bam_patch_stats *stats)
{
    const bfq_bam_opts O = bfq_bam_opts_of(opts);
    bfq_bamp_err R;
    BfqTextSeen seen[3];
    bfq_texts_look(c, X, 3, seen, false);
    for (u32 k = 0; k < 3; k++)
        if (seen[k].present && !bfq_bamp_gzip_ok(seen[k].first, seen[k].len, k, &R)) patch_refuse(R);
    // Every text's lines, which size its index, are counted on the device before the arena is reserved.
    TextPlaced t[3];
    bfq_texts_place(c, X, bfq_texts_plan(seen, 3, false), 3, t);
    bool present[3];
    size_t textNeed = 0;
    for (u32 k = 0; k < 3; k++) {
        present[k] = seen[k].present;
        if (present[k]) textNeed += bfq_line_index_bytes(t[k].len, t[k].lines) + 4096;
    }
    const std::function<size_t(u64)> more = [&](u64 raw) {
        const size_t np = (size_t)(raw / O.piece + 2);
        return np * (sizeof(bfq_bam_piece) + sizeof(bfq_bam_job) + sizeof(bfq_bamp_cnt) + 8) + textNeed + extra(raw) + 8192;
    };
    bfq_bam_chain_device(c, h_in, len, O, more, nullptr, C);
    sized(C->raw);
    bfq_bam_texts T{};
    for (u32 k = 0; k < 3; k++) {
        if (!present[k]) continue;
        u64 nl = 0;
        T.text[k] = t[k].d; T.len[k] = t[k].len;
        T.lineEnd[k] = bfq_line_index(c, t[k].d, t[k].len, &nl);
        if (!bfq_bamp_lines_ok(nl, C->S.written[k], k, &R)) { c->profCollect(); patch_refuse(R); }
    }
    const u64 nj = C->jobs.size();
    bfq_bam_job *d_jobs = c->alloc<bfq_bam_job>(nj + 1);
    bfq_bamp_cnt *d_cnt = c->alloc<bfq_bamp_cnt>(nj + 1);
    u64 *d_bad = c->alloc<u64>(1);
    bfq_bamp_err *d_err = c->alloc<bfq_bamp_err>(1);
    bfq_upload(c, d_jobs, C->jobs.data(), sizeof(bfq_bam_job) * nj);
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    bfq_bam_launch_patch_check(c, C->d_s, C->raw, d_jobs, nj, C->nref, O, T, BFQ_BAM_NONE, d_bad, d_err);
    u64 firstBad = BFQ_BAM_NONE;
    HIP_CHECK(hipMemcpyAsync(&firstBad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (firstBad != BFQ_BAM_NONE) {                                 // the piece that holds it, once more, for the message's words
        u64 j = 0;
        while (j + 1 < nj && C->jobs[j + 1].start <= firstBad) j++;
        bfq_bam_launch_patch_check(c, C->d_s, C->raw, d_jobs, nj, C->nref, O, T, j, d_bad, d_err);
        HIP_CHECK(hipMemcpyAsync(&R, d_err, sizeof R, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        c->profCollect();
        R.rec += bfq_bamp_rec_bases(C->P, C->jobs, C->hdrEnd, O.piece)[j];
        patch_refuse(R);
    }
    bfq_bam_launch_patch(c, C->d_s, C->raw, d_jobs, nj, C->nref, O, T, d_cnt);
    std::vector<bfq_bamp_cnt> cnt(nj + 1);
    if (nj) HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(bfq_bamp_cnt) * nj, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    c->profCollect();
    if (stats) bfq_bamp_totals(C->S, present, C->raw, cnt.data(), nj, stats);
}

extern "C" int bfq_bam_patch_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, const uint8_t *const d_text[3],
                                    const uint64_t text_len[3], uint8_t *d_out_raw, uint64_t cap, uint64_t *raw_len, bfq_bam_patch_stats *stats)
{
    if (raw_len) *raw_len = 0;
    if (stats) *stats = bfq_bam_patch_stats{};
    return guarded(c, [&] {
        if (!d_text || !text_len || !raw_len || (!d_out_raw && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        TextIn X[3];
        bfq_texts_of(d_text, text_len, true, X);
        bfq_bam_chain_dev C;
        bfq_bam_patch_stats PS{};
        patch_core(c, h_in, len, opts, X, [](u64) { return (size_t)0; }, [&](u64 raw) {
            if (cap >= raw) return;
            *raw_len = raw;
            c->profCollect();
            throw BfqError{BFQ_E_ARG, "output buffer too small for the stream"};
        }, &C, &PS);
        // (the stream is patched in the arena and copied out last: a refusal has then written nothing into the caller's buffer)
        if (C.raw) HIP_CHECK(hipMemcpyAsync(d_out_raw, C.d_s, (size_t)C.raw, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        *raw_len = C.raw;
        if (stats) *stats = PS;
    });
}

// host texts in, the compressed file out to dst (memory of cap bytes, or a file)
static void patch_compressed(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts *opts, const TextIn X[3], int level, HostRef dst, u64 cap, uint64_t *out_len,
                             bfq_bam_patch_stats *stats)
{
    patch_check_level(level);
    bfq_bam_chain_dev C;
    bfq_bam_patch_stats PS{};
    patch_core(c, h_in, len, opts, X, [&](u64 raw) { return bfq_deflate_need(c, raw, false, 0) + 4096; }, [&](u64 raw) {
        if (cap >= bfq_defl_bound(raw)) return;
        *out_len = bfq_defl_bound(raw);
        c->profCollect();
        throw BfqError{BFQ_E_ARG, "output buffer below bfq_bgzf_deflate_bound(raw length)"};
    }, &C, &PS);
    *out_len = bfq_deflate_core(c, C.d_s, HostRef{}, C.raw, level, dst, true, 0);
    if (stats) *stats = PS;
}

extern "C" int bfq_bam_patch(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, const uint8_t *const h_text[3], const uint64_t text_len[3],
                             int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len, bfq_bam_patch_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_bam_patch_stats{};
    return guarded(c, [&] {
        if (!h_text || !text_len || !out_len || (!h_out && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        TextIn X[3];
        bfq_texts_of(h_text, text_len, false, X);
        patch_compressed(c, h_in, len, opts, X, level, HostRef::mem(h_out), cap, out_len, stats);
    });
}

extern "C" int bfq_bam_patch_fd(bfq_ctx *c, int bam_fd, uint64_t len, const bfq_bam_opts *opts, const int text_fd[3], int level, int out_fd, uint64_t *out_len,
                                bfq_bam_patch_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_bam_patch_stats{};
    // the files are mapped, and uploaded from the mappings (the BGZF directory is read from headers and trailers all over the file)
    MappedInput bam, text[3];
    return guarded(c, [&] {
        if (!out_len || !text_fd) throw BfqError{BFQ_E_ARG, "null argument"};
        if (bam_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        if (!bam.open(bam_fd, (size_t)len)) throw BfqError{BFQ_E_IO, std::string("cannot map the input file: ") + strerror(errno)};
        TextIn X[3];
        bfq_texts_map(text_fd, text, X);
        try {
            patch_compressed(c, bam.data(), len, opts, X, level, HostRef::file(out_fd, 0), ~0ull, out_len, stats);
            bfq_fd_size(out_fd, *out_len, "cannot size the output file: ", true);
        } catch (...) {
            if (ftruncate(out_fd, 0) != 0) {}
            *out_len = 0;
            throw;
        }
    });
}
