// bfq_reorder.hip -- FASTQ text in, the same records in another order out (include/bfqzip_hip.h, bfq_fastq_reorder*): the
// pre-pass of `BFQzip_parallel.py --reorder {1,2}` (:59-75,389-437) as one call.  The kernels are k_reorder.hip's; this
// file moves the bytes and sizes the memory:
//   text buffer  the input (two mates: one after the other), uploaded through the staging workers
//   arena        line index, record index, sort records, permutation, new offsets, and the output text, which leaves
//                through bfq_download (host buffers) or the background writers (files)
// The output's length is the input's (+ 1 where the final newline was missing), so capacities are checked before anything
// is uploaded and the output files are mapped to their final size at once.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_reorder.h"

#define RO_MAX_MATES 2

struct RoSrc { HostRef ref; u64 len; };
// where a mate's text goes once it is known to be good; put() is called at most once per mate
struct RoSink {
    u64 cap[RO_MAX_MATES] = {~0ull, ~0ull};
    std::function<void(int, const u8 *, u64)> put;
};

static bool ro_ends_with_newline(const RoSrc &t)
{
    if (!t.len) return true;
    if (t.ref.ptr) return ((const u8 *)t.ref.ptr)[t.len - 1] == (u8)'\n';
    u8 b = 0;
    if (pread(t.ref.fd, &b, 1, (off_t)(t.ref.off + t.len - 1)) != 1) throw BfqError{BFQ_E_IO, "cannot read the input file"};
    return b == (u8)'\n';
}

static void ro_nomem(bfq_ctx *c, size_t need)
{
    char b[240];
    snprintf(b, sizeof b, "reordering needs %.2f GiB of device memory (input + output text + index), above the cap of %.2f GiB "
                          "(bfq_params.ws_cap_mib / BFQ_WS_CAP)", need / 1073741824.0, c->wsLimit() / 1073741824.0);
    throw BfqError{BFQ_E_NOMEM, b};
}

static void ro_check_opts(const bfq_reorder_opts *o, int nparts, int *k)
{
    if (!o) throw BfqError{BFQ_E_ARG, "null argument"};
    if (nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, "bfq_fastq_reorder: 1 or 2 parts (a file, or two files of mates)"};
    if (o->mode != 1 && o->mode != 2) throw BfqError{BFQ_E_ARG, "bfq_reorder_opts.mode: 1 (random) or 2 (locus)"};
    *k = o->k ? o->k : BFQ_RO_KDEF;
    if (*k < BFQ_RO_KMIN || *k > BFQ_RO_KMAX) throw BfqError{BFQ_E_ARG, "bfq_reorder_opts.k: 8..32 (0: 21)"};
}

// lengths of the outputs: known from the inputs alone
static void ro_lengths(const RoSrc *src, int np, u64 *tl)
{
    for (int p = 0; p < np; p++) {
        if (src[p].len && src[p].ref.null()) throw BfqError{BFQ_E_ARG, "null FASTQ text"};
        tl[p] = src[p].len + (ro_ends_with_newline(src[p]) ? 0 : 1);
    }
}

static void reorder_core(bfq_ctx *c, const RoSrc *src, int np, const bfq_reorder_opts *opts, const RoSink &sink, const u64 *tl,
                         uint64_t *h_perm, uint64_t *n_reads)
{
    int k = 0;
    ro_check_opts(opts, np, &k);
    u64 toff[RO_MAX_MATES + 1] = {0, 0, 0}, sum = 0;
    for (int p = 0; p < np; p++) {
        if (tl[p] > sink.cap[p]) throw BfqError{BFQ_E_ARG, "output buffer smaller than the FASTQ text (the input's length, + 1 without a final newline)"};
        toff[p] = sum;
        sum += (tl[p] + 64 + 255) & ~255ull;                    // every text 256-byte aligned and padded (16-byte loads)
    }
    toff[np] = sum;
    if (c->wsLimit() && 2 * sum > c->wsLimit()) ro_nomem(c, 2 * sum);
    bfq_phase("alloc");
    u8 *d_in = c->textBuf(sum + 64);
    bfq_phase("read_h2d");
    for (int p = 0; p < np; p++) {
        bfq_upload(c, d_in + toff[p], src[p].ref, src[p].len);
        if (tl[p] > src[p].len) HIP_CHECK(hipMemsetAsync(d_in + toff[p] + src[p].len, '\n', 1, c->stream));
    }
    bfq_phase("alloc");
    const u64 maxLen = *std::max_element(tl, tl + np);
    c->reserve(16 * (maxLen / 4096 + 16) + (64u << 20));
    bfq_phase("gpu");
    u64 nlines = 0;
    for (int p = 0; p < np; p++) nlines = std::max(nlines, bfq_fastq_count_lines(c, d_in + toff[p], tl[p]));
    const u64 Nb = nlines / 4 + 1;
    // per mate: the output, line ends, chunk counts of the line index, records + read offsets + lengths, sizes + new offsets;
    // once: two sets of sort records, the permutation, the radix passes' digit tables, the scans' partial sums
    const u64 nbRadix = std::min(Nb / BFQ_RS_TILE, std::max(Nb / BFQ_RS_BLOCK_ELEMS, (u64)8192)) + 2;   // radix blocks of any n <= Nb (bfq_radix_block_elems)
    const size_t perMate = (size_t)(maxLen + 4096) + 8 * (size_t)(nlines + 64) + 16 * (size_t)(maxLen / 4096 + 16) + (32 + 8 + 4 + 16) * (size_t)(Nb + 64);
    const size_t need = np * perMate + (24 + 8) * (size_t)(Nb + 64) + 12 * 256 * (size_t)nbRadix + (size_t)(Nb >> 7) + (8u << 20);
    if (c->wsLimit() && sum + need > c->wsLimit()) ro_nomem(c, sum + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    c->zeroCounters();
    RoText mate[RO_MAX_MATES];
    u64 N = 0;
    for (int p = 0; p < np; p++) {
        DevFastq fq;
        bfq_fastq_index(c, d_in + toff[p], tl[p], &fq);
        mate[p] = RoText{d_in + toff[p], (const FqRec *)fq.rec, tl[p]};
        if (p && fq.N != N) {
            char b[200];
            snprintf(b, sizeof b, "the mates differ in their number of records: %llu in the first file, %llu in the second",
                     (unsigned long long)N, (unsigned long long)fq.N);
            throw BfqError{BFQ_E_ARG, b};
        }
        N = fq.N;
    }
    if (N >> 56) throw BfqError{BFQ_E_ARG, "more than 2^56 reads"};
    SortRec a{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)}, b{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)};
    bfq_reorder_keys(c, mate, np, N, opts->mode, k, opts->seed, a);
    const SortRec sorted = bfq_radix_sort(c, a, b, N, (BFQ_RO_KEY_BITS + 7) / 8);
    u64 *perm = c->alloc<u64>(N + 1), *sizes[RO_MAX_MATES] = {nullptr, nullptr}, *newOff[RO_MAX_MATES] = {nullptr, nullptr};
    for (int p = 0; p < np; p++) { sizes[p] = c->alloc<u64>(N + 1); newOff[p] = c->alloc<u64>(N + 2); }
    bfq_reorder_perm(c, sorted, mate, np, N, perm, sizes);
    for (int p = 0; p < np; p++) {
        bfq_exscan_u64(c, sizes[p], newOff[p], N, newOff[p] + N);
        u8 *d_out = c->alloc<u8>(tl[p] + 64);
        bfq_reorder_gather(c, mate[p], perm, newOff[p], N, d_out);
        sink.put(p, d_out, tl[p]);
    }
    if (h_perm && N) bfq_download(c, h_perm, perm, 8 * N);
    c->sync();
    c->profCollect();
    if (n_reads) *n_reads = N;
}

extern "C" int bfq_fastq_reorder(bfq_ctx *c, const bfq_text_part *parts, int nparts, const bfq_reorder_opts *opts, uint8_t *const *h_out,
                                 const uint64_t *cap, uint64_t *out_len, uint64_t *h_perm, uint64_t *n_reads)
{
    if (out_len) for (int p = 0; p < nparts && p < RO_MAX_MATES; p++) out_len[p] = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (!parts || !h_out || !cap || nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, "bfq_fastq_reorder: 1 or 2 parts, their outputs and capacities"};
        RoSrc src[RO_MAX_MATES];
        RoSink sink;
        u64 tl[RO_MAX_MATES] = {0, 0};
        for (int p = 0; p < nparts; p++) {
            if (!h_out[p] && cap[p]) throw BfqError{BFQ_E_ARG, "null argument"};
            src[p] = RoSrc{HostRef::mem(parts[p].data), parts[p].len};
            sink.cap[p] = cap[p];
        }
        ro_lengths(src, nparts, tl);
        sink.put = [&](int p, const u8 *d_text, u64 len) {
            bfq_phase("d2h_write");
            bfq_download(c, h_out[p], d_text, len);
            bfq_phase("gpu");
        };
        reorder_core(c, src, nparts, opts, sink, tl, h_perm, n_reads);
        if (out_len) for (int p = 0; p < nparts; p++) out_len[p] = tl[p];
    });
}

extern "C" int bfq_fastq_reorder_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, const bfq_reorder_opts *opts,
                                    const int *out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    if (out_len) for (int p = 0; p < nparts && p < RO_MAX_MATES; p++) out_len[p] = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (!in_fd || !in_len || !out_fd || nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, "bfq_fastq_reorder_fd: 1 or 2 input and output files"};
        for (int p = 0; p < nparts; p++)
            if (in_fd[p] < 0 || out_fd[p] < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        OutFile of[RO_MAX_MATES];
        int opened = 0;
        try {
            RoSrc src[RO_MAX_MATES];
            u64 tl[RO_MAX_MATES] = {0, 0};
            for (int p = 0; p < nparts; p++) src[p] = RoSrc{HostRef::file(in_fd[p]), in_len[p]};
            ro_lengths(src, nparts, tl);
            int k = 0;
            ro_check_opts(opts, nparts, &k);
            // mapped to their final length and pre-faulted beside the upload
            for (int p = 0; p < nparts; p++) { of[p].open(out_fd[p], tl[p] + 4096, tl[p]); opened = p + 1; }
            c->call.writeHint = (size_t)(tl[0] + tl[1]);
            RoSink sink;
            sink.put = [&](int p, const u8 *d_text, u64 len) { bfq_write_async(c, of[p].at(0), d_text, len); };
            reorder_core(c, src, nparts, opts, sink, tl, nullptr, n_reads);
            bfq_phase("d2h_write");
            bfq_write_wait(c);
            opened = 0;
            bool ok = true;
            for (int p = 0; p < nparts; p++) ok = of[p].close(tl[p]) && ok;
            if (!ok) throw BfqError{BFQ_E_IO, "cannot size the output files"};
            if (out_len) for (int p = 0; p < nparts; p++) out_len[p] = tl[p];
        } catch (...) {
            if (opened) { try { bfq_write_wait(c); } catch (...) {} }
            for (int p = 0; p < nparts; p++) {
                if (p >= opened && !of[p].m && of[p].fd < 0) { of[p].fd = out_fd[p]; of[p].m = bfq_outmap_take(out_fd[p], 0); }   // (a mapping the caller registered goes with the file's contents)
                of[p].close(0);
            }
            throw;
        }
    });
}
