// bfq_reorder.hip -- FASTQ text in, the same records in another order out (include/bfqzip_hip.h, bfq_fastq_reorder*): the
// pre-pass of `BFQzip_parallel.py --reorder {1,2}` (:59-75,389-437) as one call.  The kernels are k_reorder.hip's; this
// file moves the bytes and sizes the memory:
//   text buffer  the input (two mates: one after the other), uploaded through the staging workers
//   arena        line index, record index, sort records, permutation, new offsets, and the output text, which leaves
//                through bfq_download (host buffers) or the background writers (files)
// The output's length is the input's (+ 1 where the final newline was missing), so capacities are checked before anything
// is uploaded and the output files are mapped to their final size at once.
//
// reorder_core() serves both directions; what differs is where the order comes from (RoOrder):
//   forward (bfq_fastq_reorder*)  keys, the radix sort, k_ro_perm; bfq_fastq_reorder_keep* also pack the permutation on the
//                                 device (k_perm_pack) and hand it out as the BFQPERM1 container of bfq_perm.h
//   back (bfq_fastq_unreorder*)   the container is uploaded, unpacked, validated and inverted (k_perm_unpack / k_perm_invert /
//                                 k_perm_check); the inverse is the permutation the gather reads through
#include <string.h>
#include <stdio.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_reorder.h"
#include "bfq_perm.h"

#define RO_MAX_MATES 2

// where a mate's text goes once it is known to be good; put() is called at most once per mate
struct RoSink {
    u64 cap[RO_MAX_MATES] = {~0ull, ~0ull};
    std::function<void(int, const u8 *, u64)> put;
};

// Where the order of a call comes from.  make(): the device array `order` (output record j = input record order[j]) and the
// record sizes in that order, for every mate; it throws before anything has been written.  done(): after the gathers have been
// queued (the forward calls hand the permutation out there).
struct RoOrder {
    const char *what = "bfq_fastq_reorder";
    size_t extraPerRead = 0;                 // arena bytes per read beyond the forward call's (the packed permutation)
    std::function<const u64 *(const RoText *mate, int np, u64 N, u64 *const *sizes)> make;
    std::function<void(const u64 *order, u64 N)> done;
};

static void ro_nomem(bfq_ctx *c, size_t need) { bfq_nomem_cap(c, "reordering", "input + output text + index", need); }

static void ro_check_parts(int nparts, const char *what)
{
    if (nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, std::string(what) + ": 1 or 2 parts (a file, or two files of mates)"};
}
static void ro_check_opts(const bfq_reorder_opts *o, int nparts, int *k)
{
    if (!o) throw BfqError{BFQ_E_ARG, "null argument"};
    ro_check_parts(nparts, "bfq_fastq_reorder");
    if (o->mode != 1 && o->mode != 2) throw BfqError{BFQ_E_ARG, "bfq_reorder_opts.mode: 1 (random) or 2 (locus)"};
    *k = o->k ? o->k : BFQ_RO_KDEF;
    if (*k < BFQ_RO_KMIN || *k > BFQ_RO_KMAX) throw BfqError{BFQ_E_ARG, "bfq_reorder_opts.k: 8..32 (0: 21)"};
}

// The inputs looked at, part by part, and where they go on the device.  The plan's lengths are the outputs': known from the
// inputs alone.  A part of no bytes is a text whatever its pointer.
static BfqTextPlan ro_plan(bfq_ctx *c, TextIn *src, int np)
{
    static const u8 none = 0;
    BfqTextSeen seen[RO_MAX_MATES];
    for (int p = 0; p < np; p++) {
        if (src[p].len && !src[p].present()) throw BfqError{BFQ_E_ARG, "null FASTQ text"};
        if (!src[p].present()) src[p].ref = HostRef::mem(&none);
        bfq_texts_look(c, &src[p], 1, &seen[p], false);
        if (bfq_seen_gzip(seen[p]))
            throw BfqError{BFQ_E_ARG, "a bgzip-compressed (BGZF) input is not reordered as it is: inflate first (bfq_bgzf_inflate, bfq_bgzf -d)"};
        bfq_texts_look(c, &src[p], 1, &seen[p], true);
    }
    return bfq_texts_plan(seen, np, true);
}

static void reorder_core(bfq_ctx *c, const TextIn *src, int np, const RoOrder &order, const RoSink &sink, const BfqTextPlan &plan,
                         uint64_t *n_reads)
{
    ro_check_parts(np, order.what);
    for (int p = 0; p < np; p++)
        if (plan.t[p].len > sink.cap[p]) throw BfqError{BFQ_E_ARG, "output buffer smaller than the FASTQ text (the input's length, + 1 without a final newline)"};
    const size_t sum = plan.bufNeed;
    if (c->wsLimit() && 2 * sum > c->wsLimit()) ro_nomem(c, 2 * sum);
    bfq_phase("alloc");
    TextPlaced in[RO_MAX_MATES];
    bfq_texts_place(c, src, plan, np, in);
    u64 maxLen = 0, nlines = 0;
    for (int p = 0; p < np; p++) { maxLen = std::max(maxLen, in[p].len); nlines = std::max(nlines, in[p].lines); }
    const u64 Nb = nlines / 4 + 1;
    // per mate: the output, line ends, chunk counts of the line index, records + read offsets + lengths, sizes + new offsets;
    // once: two sets of sort records, the permutation, the radix passes' digit tables, the scans' partial sums; the packed
    // permutation of the keeping calls (8 bytes per read at most).  The way back has the container, the unpacked permutation
    // and its inverse where the forward calls have their sort records.
    const u64 nbRadix = std::min(Nb / BFQ_RS_TILE, std::max(Nb / BFQ_RS_BLOCK_ELEMS, (u64)8192)) + 2;   // radix blocks of any n <= Nb (bfq_radix_block_elems)
    // (slack, as reserved so far: 16 bytes per chunk of text where the line kernels take 12, and 4 KiB)
    const size_t perMate = (size_t)(maxLen + 4096) + bfq_fastq_index_bytes(maxLen, nlines) + (8 + 8) * (size_t)(Nb + 64) + 4 * (size_t)(maxLen / BFQ_NL_CHUNK) + 4096;
    const size_t need = np * perMate + (24 + 8 + order.extraPerRead) * (size_t)(Nb + 64) + 12 * 256 * (size_t)nbRadix + (size_t)(Nb >> 7) + (8u << 20);
    if (c->wsLimit() && sum + need > c->wsLimit()) ro_nomem(c, sum + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    c->zeroCounters();
    RoText mate[RO_MAX_MATES];
    u64 N = 0;
    for (int p = 0; p < np; p++) {
        DevFastq fq;
        bfq_fastq_index(c, in[p].d, in[p].len, &fq);
        mate[p] = RoText{in[p].d, (const FqRec *)fq.rec, in[p].len};
        if (p && fq.N != N) {
            char b[200];
            snprintf(b, sizeof b, "the mates differ in their number of records: %llu in the first file, %llu in the second",
                     (unsigned long long)N, (unsigned long long)fq.N);
            throw BfqError{BFQ_E_ARG, b};
        }
        N = fq.N;
    }
    if (N >> 56) throw BfqError{BFQ_E_ARG, "more than 2^56 reads"};
    u64 *sizes[RO_MAX_MATES] = {nullptr, nullptr}, *newOff[RO_MAX_MATES] = {nullptr, nullptr};
    for (int p = 0; p < np; p++) { sizes[p] = c->alloc<u64>(N + 1); newOff[p] = c->alloc<u64>(N + 2); }
    const u64 *perm = order.make(mate, np, N, sizes);
    for (int p = 0; p < np; p++) {
        bfq_exscan_u64(c, sizes[p], newOff[p], N, newOff[p] + N);
        u8 *d_out = c->alloc<u8>(in[p].len + 64);
        bfq_reorder_gather(c, mate[p], perm, newOff[p], N, d_out);
        sink.put(p, d_out, in[p].len);
    }
    if (order.done) order.done(perm, N);
    c->sync();
    c->profCollect();
    if (n_reads) *n_reads = N;
}

// the forward order: keys, sort, permutation.  packed != nullptr: the call keeps the permutation -- capPermz is checked before
// anything is written, and *packed receives the payload of the container (device, bfq_perm_words() words) once the gathers
// are queued.
static RoOrder ro_sorted_order(bfq_ctx *c, const bfq_reorder_opts *opts, int np, uint64_t *h_perm, const u64 **packed = nullptr,
                               u64 capPermz = 0)
{
    int k = 0;
    ro_check_opts(opts, np, &k);
    RoOrder o;
    o.extraPerRead = packed ? 8 : 0;
    o.make = [=](const RoText *mate, int nm, u64 N, u64 *const *sizes) -> const u64 * {
        if (packed && capPermz < bfq_perm_bound_of(N)) {
            char b[200];
            snprintf(b, sizeof b, "permutation buffer smaller than the BFQPERM1 container of %llu reads (bfq_perm_bound: %llu bytes)",
                     (unsigned long long)N, (unsigned long long)bfq_perm_bound_of(N));
            throw BfqError{BFQ_E_ARG, b};
        }
        SortRec a{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)}, b{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)};
        bfq_reorder_keys(c, mate, nm, N, opts->mode, k, opts->seed, a);
        const SortRec sorted = bfq_radix_sort(c, a, b, N, (BFQ_RO_KEY_BITS + 7) / 8);
        u64 *perm = c->alloc<u64>(N + 1);
        bfq_reorder_perm(c, sorted, mate, nm, N, perm, sizes);
        return perm;
    };
    o.done = [=](const u64 *perm, u64 N) {
        if (h_perm && N) bfq_download(c, h_perm, perm, 8 * N);
        if (packed) {
            u64 *words = c->alloc<u64>(bfq_perm_words(N, bfq_perm_width(N)) + 1);
            bfq_perm_pack(c, perm, N, words);
            *packed = words;
        }
    };
    return o;
}

// the order of the way back: the inverse of the container's permutation
static RoOrder ro_inverse_order(bfq_ctx *c, const u8 *h_permz, u64 permzLen)
{
    u64 PN = 0;
    if (!bfq_perm_header(h_permz, permzLen, &PN, nullptr, nullptr))
        throw BfqError{BFQ_E_ARG, "perm: not a BFQPERM1 container (magic, entry width, length or padding)"};
    RoOrder o;
    o.what = "bfq_fastq_unreorder";
    o.make = [=](const RoText *mate, int nm, u64 N, u64 *const *sizes) -> const u64 * {
        if (PN != N) {
            char b[200];
            snprintf(b, sizeof b, "perm: a permutation of %llu reads for a text of %llu records", (unsigned long long)PN, (unsigned long long)N);
            throw BfqError{BFQ_E_ARG, b};
        }
        const u64 nw = bfq_perm_words(N, bfq_perm_width(N));
        u64 *words = c->alloc<u64>(nw + 1), *perm = c->alloc<u64>(N + 1), *inv = c->alloc<u64>(N + 1);
        if (nw) bfq_upload(c, words, h_permz + BFQ_PERM_HDR, 8 * nw);
        const u64 bad = bfq_perm_unpack_invert(c, words, N, perm, inv);
        if (bad != BFQ_PERM_NOPOS) {
            char b[200];
            snprintf(b, sizeof b, "perm: not a permutation: entry %llu is out of range or repeats an earlier one", (unsigned long long)bad);
            throw BfqError{BFQ_E_ARG, b};
        }
        bfq_reorder_sizes(c, inv, mate, nm, N, sizes);
        return inv;
    };
    return o;
}

// host buffers in, host buffers out: the body of bfq_fastq_reorder / _keep / bfq_fastq_unreorder.  order() is called once the
// arguments have been looked at; finish(N) after the texts have arrived.
static int ro_run_mem(bfq_ctx *c, const char *what, const bfq_text_part *parts, int nparts, uint8_t *const *h_out, const uint64_t *cap,
                      uint64_t *out_len, uint64_t *n_reads, const std::function<RoOrder()> &order, const std::function<void(u64)> &finish)
{
    if (out_len) for (int p = 0; p < nparts && p < RO_MAX_MATES; p++) out_len[p] = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (!parts || !h_out || !cap || nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, std::string(what) + ": 1 or 2 parts, their outputs and capacities"};
        TextIn src[RO_MAX_MATES];
        RoSink sink;
        for (int p = 0; p < nparts; p++) {
            if (!h_out[p] && cap[p]) throw BfqError{BFQ_E_ARG, "null argument"};
            src[p].ref = HostRef::mem(parts[p].data); src[p].len = parts[p].len;
            sink.cap[p] = cap[p];
        }
        const BfqTextPlan plan = ro_plan(c, src, nparts);
        sink.put = [&](int p, const u8 *d_text, u64 len) { bfq_download_phase(c, h_out[p], d_text, len); };
        uint64_t N = 0;
        reorder_core(c, src, nparts, order(), sink, plan, &N);
        if (finish) finish(N);
        if (n_reads) *n_reads = N;
        if (out_len) for (int p = 0; p < nparts; p++) out_len[p] = plan.t[p].len;
    });
}

// open files in, open files out: the body of bfq_fastq_reorder_fd / _keep_fd / bfq_fastq_unreorder_fd.  queue(N) may add
// background writes of its own after the texts', to extra_fd (< 0: none), and returns that file's length: it is a third
// member of the outputs, never mapped, and left empty with them.
static int ro_run_fd(bfq_ctx *c, const char *what, const int *in_fd, const uint64_t *in_len, int nparts, const int *out_fd, uint64_t *out_len,
                     uint64_t *n_reads, const std::function<RoOrder()> &order, int extra_fd = -1, const std::function<u64(u64)> &queue = nullptr)
{
    if (out_len) for (int p = 0; p < nparts && p < RO_MAX_MATES; p++) out_len[p] = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (!in_fd || !in_len || !out_fd || nparts < 1 || nparts > RO_MAX_MATES) throw BfqError{BFQ_E_ARG, std::string(what) + ": 1 or 2 input and output files"};
        for (int p = 0; p < nparts; p++)
            if (in_fd[p] < 0 || out_fd[p] < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        const int fds[RO_MAX_MATES + 1] = {out_fd[0], nparts > 1 ? out_fd[1] : -1, extra_fd};
        OutFiles F(fds, RO_MAX_MATES + 1, [c] { bfq_write_wait(c); });
        TextIn src[RO_MAX_MATES];
        for (int p = 0; p < nparts; p++) { src[p].ref = HostRef::file(in_fd[p]); src[p].len = in_len[p]; }
        const BfqTextPlan plan = ro_plan(c, src, nparts);
        u64 fin[RO_MAX_MATES + 1] = {plan.t[0].len, plan.t[1].len, 0};
        const RoOrder ord = order();
        // mapped to their final length and pre-faulted beside the upload
        for (int p = 0; p < nparts; p++) F.open(p, fin[p] + 4096, fin[p]);
        c->call.writeHint = (size_t)(fin[0] + fin[1]);
        RoSink sink;
        sink.put = [&](int p, const u8 *d_text, u64 len) { bfq_write_async(c, F.at(p, 0), d_text, len); };
        uint64_t N = 0;
        reorder_core(c, src, nparts, ord, sink, plan, &N);
        if (queue) fin[RO_MAX_MATES] = queue(N);
        bfq_phase("d2h_write");
        F.commit(fin);
        if (n_reads) *n_reads = N;
        if (out_len) for (int p = 0; p < nparts; p++) out_len[p] = fin[p];
    });
}

extern "C" int bfq_fastq_reorder(bfq_ctx *c, const bfq_text_part *parts, int nparts, const bfq_reorder_opts *opts, uint8_t *const *h_out,
                                 const uint64_t *cap, uint64_t *out_len, uint64_t *h_perm, uint64_t *n_reads)
{
    return ro_run_mem(c, "bfq_fastq_reorder", parts, nparts, h_out, cap, out_len, n_reads,
                      [&] { return ro_sorted_order(c, opts, nparts, h_perm); }, nullptr);
}

extern "C" int bfq_fastq_reorder_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, const bfq_reorder_opts *opts,
                                    const int *out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    return ro_run_fd(c, "bfq_fastq_reorder_fd", in_fd, in_len, nparts, out_fd, out_len, n_reads,
                     [&] { return ro_sorted_order(c, opts, nparts, nullptr); });
}

// ---- the permutation kept: the same calls, and the BFQPERM1 container of what they did --------------------------------------
// the header names the options as they took effect: k = 0 is written as the default it stands for
static void ro_put_header(u8 *out, u64 N, const bfq_reorder_opts *opts)
{
    bfq_reorder_opts eff = *opts;
    if (!eff.k) eff.k = BFQ_RO_KDEF;
    bfq_perm_put_header(out, N, &eff);
}
extern "C" int bfq_fastq_reorder_keep(bfq_ctx *c, const bfq_text_part *parts, int nparts, const bfq_reorder_opts *opts, uint8_t *const *h_out,
                                      const uint64_t *cap, uint64_t *out_len, uint8_t *h_permz, uint64_t cap_permz, uint64_t *permz_len,
                                      uint64_t *n_reads)
{
    if (permz_len) *permz_len = 0;
    const u64 *packed = nullptr;
    return ro_run_mem(c, "bfq_fastq_reorder_keep", parts, nparts, h_out, cap, out_len, n_reads,
                      [&] {
                          if (!h_permz) throw BfqError{BFQ_E_ARG, "null argument"};
                          return ro_sorted_order(c, opts, nparts, nullptr, &packed, cap_permz);
                      },
                      [&](u64 N) {
                          const u64 nw = bfq_perm_words(N, bfq_perm_width(N));
                          ro_put_header(h_permz, N, opts);
                          if (nw) { bfq_download(c, h_permz + BFQ_PERM_HDR, packed, 8 * nw); c->sync(); }
                          if (permz_len) *permz_len = BFQ_PERM_HDR + 8 * nw;
                      });
}

extern "C" int bfq_fastq_reorder_keep_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, const bfq_reorder_opts *opts,
                                         const int *out_fd, int perm_fd, uint64_t *out_len, uint64_t *permz_len, uint64_t *n_reads)
{
    if (permz_len) *permz_len = 0;
    const u64 *packed = nullptr;
    u64 total = 0;
    const int rc = ro_run_fd(c, "bfq_fastq_reorder_keep_fd", in_fd, in_len, nparts, out_fd, out_len, n_reads,
                             [&] {
                                 if (perm_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
                                 return ro_sorted_order(c, opts, nparts, nullptr, &packed, ~0ull);
                             },
                             perm_fd, [&](u64 N) {
                                 const u64 nw = bfq_perm_words(N, bfq_perm_width(N));
                                 u8 hdr[BFQ_PERM_HDR];
                                 ro_put_header(hdr, N, opts);
                                 total = BFQ_PERM_HDR + 8 * nw;
                                 bfq_fd_size(perm_fd, total, "cannot size the permutation file");
                                 if (pwrite(perm_fd, hdr, BFQ_PERM_HDR, 0) != BFQ_PERM_HDR) throw BfqError{BFQ_E_IO, "cannot write the permutation file"};
                                 if (nw) bfq_write_async(c, HostRef::file(perm_fd, BFQ_PERM_HDR), packed, 8 * nw);
                                 return total;
                             });
    if (rc == BFQ_OK && permz_len) *permz_len = total;
    return rc;
}

// ---- the way back on a text: output record perm[j] = input record j ------------------------------------------------------------
extern "C" int bfq_fastq_unreorder(bfq_ctx *c, const bfq_text_part *parts, int nparts, const uint8_t *h_permz, uint64_t permz_len,
                                   uint8_t *const *h_out, const uint64_t *cap, uint64_t *out_len, uint64_t *n_reads)
{
    return ro_run_mem(c, "bfq_fastq_unreorder", parts, nparts, h_out, cap, out_len, n_reads,
                      [&] { return ro_inverse_order(c, h_permz, permz_len); }, nullptr);
}

// an input file as read-only memory
struct RoMap {
    void *p = nullptr; size_t len = 0;
    const u8 *open(int fd, u64 n)
    {
        if (fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        if (!n) return nullptr;
        struct stat st;
        if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && (u64)st.st_size < n) throw BfqError{BFQ_E_ARG, "perm: the file is shorter than permz_len"};
        void *m = mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) throw BfqError{BFQ_E_IO, "cannot map the permutation file"};
        p = m; len = (size_t)n;
        return (const u8 *)m;
    }
    ~RoMap() { if (p) munmap(p, len); }
};

extern "C" int bfq_fastq_unreorder_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, int perm_fd, uint64_t permz_len,
                                      const int *out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    RoMap pm;
    return ro_run_fd(c, "bfq_fastq_unreorder_fd", in_fd, in_len, nparts, out_fd, out_len, n_reads,
                     [&] { return ro_inverse_order(c, pm.open(perm_fd, permz_len), permz_len); });
}
