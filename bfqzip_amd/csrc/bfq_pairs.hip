// bfq_pairs.hip -- interleaved paired FASTQ (include/bfqzip_hip.h, bfq_fastq_deinterleave* / bfq_fastq_interleave*): the host
// side of splitting one text with alternating mates and of merging two texts of mates.  The definition and the host forms
// are bfq_pairs.h's; the kernels are k_pairs.hip's.  One call:
//   1  every text looked at (1f 8b, its last byte), uploaded into the context's text buffer -- or taken where it lies on the
//      device --, its lines counted there, the arena reserved from the counts, the texts indexed (bfq_fastq_index: the line
//      index and record parser of every FASTQ entry point, and its refusals)
//   2  the checks -- the record counts, the keys of the pairs -- and the sizes: exact output lengths, and the capacities
//      checked against them.  Up to here nothing of the caller's has been touched
//   3  the move, one copy of every record: into the caller's device buffers, or into the arena and from there through
//      bfq_download (host buffers) or the background writers (files: committed or left empty, OutFiles, bfq_outfiles.h)
//   arena   per text 8 bytes per line (and 12 per 4 KiB while they are indexed) and 44 per record; 16 bytes per pair (orphan
//           mode: 57 per record; repair: 83 per record) of sizes and offsets; the outputs unless they are the caller's device
//           buffers
// The repair (bfq_fastq_repair*) stages its three texts the same way; its step 2 is hash, sort, group and place (k_pairs.hip).
// The *_host forms run bfq_pairs.h by one thread, for tests and as the statement of the algorithm: no entry point here falls
// back to them.
#include <string.h>
#include <stdio.h>
#include <sys/stat.h>
#include <algorithm>
#include <functional>
#include "bfq_internal.h"
#include "bfq_pairs.h"

static_assert(sizeof(bfq_pairs_opts) == 16 && sizeof(bfq_pairs_stats) == 48 && sizeof(bfq_repair_opts) == 24 && sizeof(bfq_repair_stats) == 96, "the C-ABI's structures");

static void pr_refuse(const bfq_pairs_err &X) { throw BfqError{bfq_pairs_code(X), bfq_pairs_message(X)}; }
static bfq_pairs_opts pr_opts(const bfq_pairs_opts *in)
{
    bfq_pairs_opts O;
    bfq_pairs_err X;
    if (!bfq_pairs_resolve(in, &O, &X)) pr_refuse(X);
    return O;
}

extern "C" void bfq_pairs_default_opts(bfq_pairs_opts *o) { if (o) bfq_pairs_defaults(o); }

static thread_local std::string g_pairsHostErr;
extern "C" const char *bfq_pairs_host_error(void) { return g_pairsHostErr.c_str(); }

extern "C" int bfq_fastq_deinterleave_host(const uint8_t *text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                                           uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    if (out_len) out_len[0] = out_len[1] = out_len[2] = 0;
    if (n_reads) n_reads[0] = n_reads[1] = n_reads[2] = 0;
    if (stats) *stats = bfq_pairs_stats{};
    return host_guarded(g_pairsHostErr, [&] {
        if (!out_len || (!text && len)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_pairs_opts O = pr_opts(opts);
        const bool measure = !h_out && !cap;
        if (!measure && (!h_out || !cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        if (!measure)
            for (int k = 0; k < 3; k++)
                if (!h_out[k] && cap[k]) throw BfqError{BFQ_E_ARG, "null argument"};
        bfq_pairs_stats S;
        bfq_pairs_err X;
        u64 nr[3];
        const int r = bfq_pairs_split_host(text, len, O, h_out, cap, measure, &S, nr, &X);
        if (r == 2) pr_refuse(X);
        for (int k = 0; k < 3; k++) out_len[k] = S.out_len[k];
        if (r == 3) { X.kind = BFQ_PAIRS_E_CAP; pr_refuse(X); }
        if (n_reads) for (int k = 0; k < 3; k++) n_reads[k] = nr[k];
        if (stats) *stats = S;
    });
}

extern "C" int bfq_fastq_interleave_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *out, uint64_t cap,
                                         uint64_t *out_len, bfq_pairs_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_pairs_stats{};
    return host_guarded(g_pairsHostErr, [&] {
        if (!text || !text_len || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_pairs_opts O = pr_opts(opts);
        const bool measure = !out && !cap;
        bfq_pairs_stats S;
        bfq_pairs_err X;
        u64 nr[3];
        const int r = bfq_pairs_merge_host(text, text_len, O, out, cap, measure, &S, nr, &X);
        if (r == 2) pr_refuse(X);
        *out_len = S.out_len[0];
        if (r == 3) { X.kind = BFQ_PAIRS_E_CAP; X.merge = 1; pr_refuse(X); }
        if (stats) *stats = S;
    });
}

// ---------------------------------------------------------------- the texts of a call
// Step 1 for the texts src[0, 3): t[k] = text k on the device with its index (an absent or empty text: no records).  gzip(first,
// len, k) refuses a text that begins with 1f 8b in the caller's words; what: the caller's work, for the refusal above the
// workspace cap.  perRec / arenaOut: what steps 2 and 3 take from the arena beside the index, in bytes per record, and whether
// the outputs lie there.  (bfq_dedup.hip stages its texts here too.)
void bfq_pairs_stage(bfq_ctx *c, const TextIn src[3], const std::function<void(const u8 *, u64, u32)> &gzip, const char *what, size_t perRec, bool arenaOut,
                     PrText t[3])
{
    auto nomem = [&](size_t need) { bfq_nomem_cap(c, what, "text + outputs + index", need); };
    TextIn in[3];                                                   // (an empty text is handed on as absent: it gets no slot)
    for (u32 k = 0; k < 3; k++)
        if (src[k].present() && src[k].len) in[k] = src[k];
    BfqTextSeen seen[3];
    bfq_texts_look(c, in, 3, seen, false);
    for (u32 k = 0; k < 3; k++)
        if (seen[k].present) gzip(seen[k].first, seen[k].len, k);
    bfq_texts_look(c, in, 3, seen, true);
    const BfqTextPlan plan = bfq_texts_plan(seen, 3, true);
    const u64 bytes = plan.t[0].len + plan.t[1].len + plan.t[2].len;
    const size_t outBytes = arenaOut ? (size_t)bytes + 3 * 4096 : 0;
    if (c->wsLimit() && plan.bufNeed + outBytes > c->wsLimit()) nomem(plan.bufNeed + outBytes);
    bfq_phase("alloc");
    TextPlaced p[3];
    bfq_texts_place(c, in, plan, 3, p);
    // per text its index, and slack: 12 KiB for alignment gaps and the small buffers (flags, counters) between the arrays, and
    // the scan over its records' lengths twice more; then what steps 2 and 3 take per record, with room for four scans at a time
    u64 nb = 0;
    size_t need = outBytes + (4u << 20);
    for (u32 k = 0; k < 3; k++) {
        t[k] = PrText{p[k].d, nullptr, p[k].len, 0};
        if (!p[k].d) continue;
        const u64 n = p[k].lines / 4 + 2;
        nb += n;
        need += bfq_fastq_index_bytes(p[k].len, p[k].lines) + 12288 + 2 * bfq_scan_bytes(n);
    }
    need += perRec * (size_t)(nb + 64) + 4 * bfq_scan_bytes(nb) + 4096;
    if (c->wsLimit() && plan.bufNeed + need > c->wsLimit()) nomem(plan.bufNeed + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    c->zeroCounters();
    for (u32 k = 0; k < 3; k++) {
        if (!t[k].buf) continue;
        DevFastq fq;
        bfq_fastq_index(c, t[k].buf, t[k].len, &fq);
        t[k].rec = (const FqRec *)fq.rec; t[k].N = fq.N;
    }
}

// ... for the split (merge = 0), the merge (1) and the repair (2): the refusal names the text
static void pr_stage(bfq_ctx *c, const TextIn src[3], u32 merge, size_t perRec, bool arenaOut, PrText t[3])
{
    bfq_pairs_stage(c, src, [merge](const u8 *first, u64 len, u32 k) {
        bfq_pairs_err X;
        if (!bfq_pairs_gzip_ok(first, len, merge, k, &X)) pr_refuse(X);
    }, "splitting or merging the mates", perRec, arenaOut, t);
}

// what becomes of the outputs: sized(len) runs once the lengths are exact and before anything is written (it throws for a
// short capacity, and opens files); d_dst[k]: the caller's device buffer, nullptr: the arena and then put()
struct PrSink {
    std::function<void(const u64 *)> sized;
    u8 *d_dst[3] = {nullptr, nullptr, nullptr};
    bool device = false;
    std::function<void(int, const u8 *, u64)> put;
};

static u64 pr_first_bad(bfq_ctx *c, const PrText &a, const PrText *b, u64 P, u32 suffix)
{
    u64 *d_bad = c->alloc<u64>(1);
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    bfq_pairs_compare(c, a, b, P, suffix, d_bad);
    u64 bad = BFQ_PAIRS_NONE;
    HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    return bad;
}

static void split_core(bfq_ctx *c, const TextIn &in, const bfq_pairs_opts &O, bool measure, const PrSink &sink, u64 nReads[3], bfq_pairs_stats *S)
{
    const TextIn src[3] = {in, TextIn{}, TextIn{}};
    PrText t3[3];
    pr_stage(c, src, 0, O.orphans ? 57 : 8, !measure && !sink.device, t3);
    const PrText &t = t3[0];
    const u64 N = t.N;
    bfq_pairs_err X;
    u64 lens[3] = {0, 0, 0};
    const u64 *off[3] = {nullptr, nullptr, nullptr};
    const u8 *role = nullptr;
    if (!O.orphans) {
        if (N & 1) { c->profCollect(); X.kind = BFQ_PAIRS_E_ODD; X.n = N; pr_refuse(X); }
        const u64 P = N / 2;
        if (O.check_names) {
            const u64 bad = pr_first_bad(c, t, nullptr, P, O.mate_suffix);
            if (bad != BFQ_PAIRS_NONE) { c->profCollect(); X.kind = BFQ_PAIRS_E_NAMES; X.n = bad; pr_refuse(X); }
        }
        u64 *sz = c->alloc<u64>(P + 1), *off1 = c->alloc<u64>(P + 2);
        bfq_pairs_pair_sizes(c, t, P, sz);
        bfq_exscan_u64(c, sz, off1, P, off1 + P);
        HIP_CHECK(hipMemcpyAsync(&lens[1], off1 + P, 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        lens[2] = t.len - lens[1];
        nReads[0] = 0; nReads[1] = nReads[2] = P;
        off[1] = off1;
    } else {
        u64 *start = c->alloc<u64>(N + 1), *sz[3], *o[3], *d_cnt = c->alloc<u64>(2), cnt[2] = {0, 0};
        u8 *r = c->alloc<u8>(N + 1);
        for (int k = 0; k < 3; k++) { sz[k] = c->alloc<u64>(N + 1); o[k] = c->alloc<u64>(N + 2); }
        HIP_CHECK(hipMemsetAsync(d_cnt, 0, 16, c->stream));
        bfq_pairs_run_starts(c, t, O.mate_suffix, start);
        bfq_pairs_roles(c, t, start, r, sz, d_cnt);
        for (int k = 0; k < 3; k++) {
            bfq_exscan_u64(c, sz[k], o[k], N, o[k] + N);
            HIP_CHECK(hipMemcpyAsync(&lens[k], o[k] + N, 8, hipMemcpyDeviceToHost, c->stream));
            off[k] = o[k];
        }
        HIP_CHECK(hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        nReads[0] = cnt[0]; nReads[1] = nReads[2] = cnt[1];
        role = r;
    }
    *S = bfq_pairs_stats{};
    S->records = N; S->pairs = nReads[1]; S->singles = nReads[0];
    for (int k = 0; k < 3; k++) S->out_len[k] = lens[k];
    sink.sized(lens);
    if (measure) { c->profCollect(); return; }
    u8 *dst[3];
    for (int k = 0; k < 3; k++) dst[k] = sink.device ? sink.d_dst[k] : c->alloc<u8>(lens[k] + 64);
    if (role) bfq_pairs_split_roles(c, t, role, off, dst);
    else bfq_pairs_split(c, t, off[1], dst[1], dst[2]);
    if (!sink.device)
        for (int k = 0; k < 3; k++)
            if (lens[k]) sink.put(k, dst[k], lens[k]);
    c->sync();
    c->profCollect();
}

static void merge_core(bfq_ctx *c, const TextIn src[3], const bfq_pairs_opts &O, bool measure, const PrSink &sink, u64 nReads[3], bfq_pairs_stats *S)
{
    PrText t[3];
    pr_stage(c, src, 1, 8, !measure && !sink.device, t);
    bfq_pairs_err X;
    X.merge = 1;
    if (t[1].N != t[2].N) { c->profCollect(); X.kind = BFQ_PAIRS_E_COUNTS; X.n = t[1].N; X.m = t[2].N; pr_refuse(X); }
    const u64 P = t[1].N;
    if (O.check_names) {
        const u64 bad = pr_first_bad(c, t[1], &t[2], P, O.mate_suffix);
        if (bad != BFQ_PAIRS_NONE) { c->profCollect(); X.kind = BFQ_PAIRS_E_NAMES; X.n = bad; pr_refuse(X); }
    }
    const u64 total = t[0].len + t[1].len + t[2].len;
    *S = bfq_pairs_stats{};
    S->records = 2 * P + t[0].N; S->pairs = P; S->singles = t[0].N; S->out_len[0] = total;
    nReads[0] = t[0].N; nReads[1] = nReads[2] = P;
    sink.sized(&total);
    if (measure) { c->profCollect(); return; }
    u8 *dst = sink.device ? sink.d_dst[0] : c->alloc<u8>(total + 64);
    bfq_pairs_merge(c, t[1], t[2], dst);
    if (t[0].len) HIP_CHECK(hipMemcpyAsync(dst + t[1].len + t[2].len, t[0].buf, (size_t)t[0].len, hipMemcpyDeviceToDevice, c->stream));
    if (!sink.device && total) sink.put(0, dst, total);
    c->sync();
    c->profCollect();
}

// ---------------------------------------------------------------- what the entry points share
// the capacities against the lengths: a short one leaves out_len[] = the lengths needed
static void pr_check_caps(bfq_ctx *c, const uint64_t *cap, const u64 *lens, int n, uint64_t *out_len, u32 merge)
{
    bool ok = true;
    for (int k = 0; k < n; k++) ok = ok && cap[k] >= lens[k];
    if (ok) return;
    for (int k = 0; k < n; k++) out_len[k] = lens[k];
    c->profCollect();
    bfq_pairs_err X;
    X.kind = BFQ_PAIRS_E_CAP; X.merge = merge;
    pr_refuse(X);
}

// host or device buffers out: the body of the memory forms of the split, the merge (n = 1) and the repair.  run(sink, nr, &S)
// resolves the options and calls the core.
template <class Stats, class Run>
static void pr_run_mem(bfq_ctx *c, uint8_t *const *out, const uint64_t *cap, int n, bool device, bool measure, u32 merge, uint64_t *out_len, uint64_t *n_reads,
                       Stats *stats, Run run)
{
    if (!measure)
        for (int k = 0; k < n; k++)
            if (!out[k] && cap[k]) throw BfqError{BFQ_E_ARG, "null argument"};
    PrSink sink;
    sink.device = device;
    sink.sized = [&](const u64 *lens) { if (!measure) pr_check_caps(c, cap, lens, n, out_len, merge); };
    if (!measure && device) for (int k = 0; k < n; k++) sink.d_dst[k] = out[k];
    sink.put = [&](int k, const u8 *d_text, u64 len) { bfq_download_phase(c, out[k], d_text, len); };
    u64 nr[3] = {0, 0, 0};
    Stats S;
    run(sink, nr, &S);
    for (int k = 0; k < n; k++) out_len[k] = S.out_len[k];
    if (n_reads) for (int k = 0; k < 3; k++) n_reads[k] = nr[k];
    if (stats) *stats = S;
}

// open files out: the body of the *_fd forms.  The files are opened once the lengths are known, committed at them, and left
// empty when the call fails (OutFiles, bfq_outfiles.h).
template <class Stats, class Run>
static void pr_run_fd(bfq_ctx *c, const int *out_fd, int n, uint64_t *out_len, uint64_t *n_reads, Stats *stats, Run run)
{
    OutFiles F(out_fd, n, [c] { bfq_write_wait(c); });
    PrSink sink;
    sink.sized = [&](const u64 *lens) {
        F.openAt(lens);
        u64 sum = 0;
        for (int k = 0; k < n; k++) sum += lens[k];
        c->call.writeHint = (size_t)sum;
    };
    sink.put = [&](int k, const u8 *d_text, u64 len) { if (F.present(k)) bfq_write_async(c, F.at(k, 0), d_text, len); };
    u64 nr[3] = {0, 0, 0};
    Stats S;
    run(sink, nr, &S);
    bfq_phase("d2h_write");
    F.commit(S.out_len);
    for (int k = 0; k < n; k++) out_len[k] = S.out_len[k];
    if (n_reads) for (int k = 0; k < 3; k++) n_reads[k] = nr[k];
    if (stats) *stats = S;
}

// the texts of a call's descriptors (< 0: absent): a text is as long as its file
static void pr_texts_fd(const int text_fd[3], TextIn src[3])
{
    for (int k = 0; k < 3; k++) {
        if (text_fd[k] < 0) continue;
        struct stat st;
        if (fstat(text_fd[k], &st) != 0) throw BfqError{BFQ_E_IO, std::string("cannot stat a text file: ") + strerror(errno)};
        src[k].ref = HostRef::file(text_fd[k]); src[k].len = (u64)st.st_size;
    }
}

// ---------------------------------------------------------------- the split's entry points
static int pr_split_mem(bfq_ctx *c, TextIn in, const bfq_pairs_opts *opts, uint8_t *const *out, const uint64_t *cap, bool device, bool measure,
                        uint64_t *out_len, uint64_t *n_reads, bfq_pairs_stats *stats)
{
    zero3(out_len); zero3(n_reads);
    if (stats) *stats = bfq_pairs_stats{};
    return guarded(c, [&] {
        if (!out_len || (!in.present() && in.len) || (!measure && (!out || !cap))) throw BfqError{BFQ_E_ARG, "null argument"};
        pr_run_mem(c, out, cap, 3, device, measure, 0, out_len, n_reads, stats,
                   [&](const PrSink &sink, u64 *nr, bfq_pairs_stats *S) { split_core(c, in, pr_opts(opts), measure, sink, nr, S); });
    });
}

extern "C" int bfq_fastq_deinterleave_measure(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const bfq_pairs_opts *opts, uint64_t out_len[3],
                                              uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    TextIn in;
    in.ref = HostRef::mem(h_text); in.len = len;
    return pr_split_mem(c, in, opts, nullptr, nullptr, false, true, out_len, n_reads, stats);
}
extern "C" int bfq_fastq_deinterleave(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const h_out[3],
                                      const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    TextIn in;
    in.ref = HostRef::mem(h_text); in.len = len;
    return pr_split_mem(c, in, opts, h_out, cap, false, false, out_len, n_reads, stats);
}
extern "C" int bfq_fastq_deinterleave_device(bfq_ctx *c, const uint8_t *d_text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const d_out[3],
                                             const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    TextIn in;
    in.d = d_text; in.len = len;
    return pr_split_mem(c, in, opts, d_out, cap, true, false, out_len, n_reads, stats);
}

extern "C" int bfq_fastq_deinterleave_fd(bfq_ctx *c, int in_fd, uint64_t len, const bfq_pairs_opts *opts, const int out_fd[3], uint64_t out_len[3],
                                         uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    zero3(out_len); zero3(n_reads);
    if (stats) *stats = bfq_pairs_stats{};
    return guarded(c, [&] {
        if (!out_len || !out_fd) throw BfqError{BFQ_E_ARG, "null argument"};
        if (in_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        pr_run_fd(c, out_fd, 3, out_len, n_reads, stats, [&](const PrSink &sink, u64 *nr, bfq_pairs_stats *S) {
            const bfq_pairs_opts O = pr_opts(opts);
            TextIn in;
            in.ref = HostRef::file(in_fd); in.len = len;
            split_core(c, in, O, false, sink, nr, S);
        });
    });
}

// ---------------------------------------------------------------- the merge's entry points
static int pr_merge_mem(bfq_ctx *c, const uint8_t *const *text, const uint64_t *text_len, const bfq_pairs_opts *opts, uint8_t *out, uint64_t cap, bool device,
                        bool measure, uint64_t *out_len, uint64_t *n_reads, bfq_pairs_stats *stats)
{
    if (out_len) *out_len = 0;
    zero3(n_reads);
    if (stats) *stats = bfq_pairs_stats{};
    return guarded(c, [&] {
        if (!text || !text_len || !out_len || (!measure && !out && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        pr_run_mem(c, &out, &cap, 1, device, measure, 1, out_len, n_reads, stats, [&](const PrSink &sink, u64 *nr, bfq_pairs_stats *S) {
            const bfq_pairs_opts O = pr_opts(opts);
            TextIn src[3];
            bfq_texts_of(text, text_len, device, src);
            merge_core(c, src, O, measure, sink, nr, S);
        });
    });
}

extern "C" int bfq_fastq_interleave_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts,
                                            uint64_t *out_len, uint64_t n_reads[3], bfq_pairs_stats *stats)
{
    return pr_merge_mem(c, h_text, text_len, opts, nullptr, 0, false, true, out_len, n_reads, stats);
}
extern "C" int bfq_fastq_interleave(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *h_out,
                                    uint64_t cap, uint64_t *out_len, bfq_pairs_stats *stats)
{
    return pr_merge_mem(c, h_text, text_len, opts, h_out, cap, false, false, out_len, nullptr, stats);
}
extern "C" int bfq_fastq_interleave_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *d_out,
                                           uint64_t cap, uint64_t *out_len, bfq_pairs_stats *stats)
{
    return pr_merge_mem(c, d_text, text_len, opts, d_out, cap, true, false, out_len, nullptr, stats);
}

extern "C" int bfq_fastq_interleave_fd(bfq_ctx *c, const int text_fd[3], const bfq_pairs_opts *opts, int out_fd, uint64_t *out_len, bfq_pairs_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_pairs_stats{};
    return guarded(c, [&] {
        if (!out_len || !text_fd) throw BfqError{BFQ_E_ARG, "null argument"};
        if (out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        pr_run_fd(c, &out_fd, 1, out_len, nullptr, stats, [&](const PrSink &sink, u64 *nr, bfq_pairs_stats *S) {
            const bfq_pairs_opts O = pr_opts(opts);
            TextIn src[3];
            pr_texts_fd(text_fd, src);
            merge_core(c, src, O, false, sink, nr, S);
        });
    });
}

// ---------------------------------------------------------------- the repair
// arena bytes per record beside the index: role, two role flags and anchor (11) stay; under them first the hashes, hints, two
// sort records, the sorted (g, hint) and h words and the run starts (57, + at most 1 of radix counts), then, in the same
// space, two ranks, the slot, three sizes and three offsets (72): 83 at the peak
#define RP_PER_REC 88u

extern "C" void bfq_repair_default_opts(bfq_repair_opts *o) { if (o) bfq_repair_defaults(o); }

static bfq_repair_opts rp_opts(const bfq_repair_opts *in)
{
    bfq_repair_opts O;
    bfq_pairs_err X;
    if (!bfq_repair_resolve(in, &O, &X)) pr_refuse(X);
    return O;
}

static void repair_core(bfq_ctx *c, const TextIn src[3], const bfq_repair_opts &O, bool measure, const PrSink &sink, u64 nReads[3], bfq_repair_stats *S)
{
    PrText t[3];
    pr_stage(c, src, 2, RP_PER_REC, !measure && !sink.device, t);
    const u64 N = t[0].N + t[1].N + t[2].N;
    u8 *role = c->alloc<u8>(N + 1), *f1 = c->alloc<u8>(N + 1), *f0 = c->alloc<u8>(N + 1);
    u64 *anchor = c->alloc<u64>(N + 1), *d_stat = c->alloc<u64>(9);   // d_stat: longest run, first bad record, dup_groups, mixed_runs, P, Z, three lengths
    u64 stat[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    {
        const size_t m = c->mark();
        u64 *h = c->alloc<u64>(N + 1), *sg = c->alloc<u64>(N + 1), *sh = c->alloc<u64>(N + 1), *start = c->alloc<u64>(N + 1);
        u8 *hint = c->alloc<u8>(N + 1);
        SortRec a{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)}, b{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)};
        bfq_repair_sort(c, t, N, O, h, hint, a, b, sg, sh, start, d_stat);
        HIP_CHECK(hipMemcpyAsync(stat, d_stat, 16, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        if (stat[1] != BFQ_PAIRS_NONE) {                          // a run too long to walk: refused before anything walks it
            c->profCollect();
            bfq_pairs_err X;
            const u64 n[3] = {t[0].N, t[1].N, t[2].N};
            X.kind = BFQ_PAIRS_E_RUN; X.merge = 2;
            X.k = bfq_repair_text_of(stat[1], n, &X.n);
            pr_refuse(X);
        }
        HIP_CHECK(hipMemsetAsync(d_stat + 2, 0, 16, c->stream));
        bfq_repair_group(c, t, N, O.mate_suffix, start, sg, sh, role, anchor, f1, f0, d_stat + 2);
        c->release(m);   // stream-ordered, as in k_scan.hip
    }
    u64 *rank1 = c->alloc<u64>(N + 2), *rank0 = c->alloc<u64>(N + 2), *slot = c->alloc<u64>(N + 1), *sz[3], *o[3];
    for (int k = 0; k < 3; k++) { sz[k] = c->alloc<u64>(N + 1); o[k] = c->alloc<u64>(N + 2); }
    bfq_exscan_u8(c, f1, rank1, N, d_stat + 4);
    bfq_exscan_u8(c, f0, rank0, N, d_stat + 5);
    HIP_CHECK(hipMemcpyAsync(stat + 2, d_stat + 2, 32, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const u64 P = stat[4], Z = stat[5], cnt[3] = {Z, P, P};
    bfq_repair_place(c, t, N, role, anchor, rank1, rank0, slot, sz);
    for (int k = 0; k < 3; k++) bfq_exscan_u64(c, sz[k], o[k], cnt[k], d_stat + 6 + k);
    HIP_CHECK(hipMemcpyAsync(stat + 6, d_stat + 6, 24, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const u64 lens[3] = {stat[6], stat[7], stat[8]};
    *S = bfq_repair_stats{};
    S->records = N; S->pairs = P; S->singles = Z; S->dup_groups = stat[2]; S->mixed_runs = stat[3]; S->max_run = stat[0];
    for (int k = 0; k < 3; k++) { S->out_len[k] = lens[k]; S->n_in[k] = t[k].N; }
    nReads[0] = Z; nReads[1] = nReads[2] = P;
    sink.sized(lens);
    if (measure) { c->profCollect(); return; }
    u8 *dst[3];
    for (int k = 0; k < 3; k++) dst[k] = sink.device ? sink.d_dst[k] : c->alloc<u8>(lens[k] + 64);
    const u64 *const off[3] = {o[0], o[1], o[2]};
    bfq_repair_move(c, t, N, role, slot, off, dst);
    if (!sink.device)
        for (int k = 0; k < 3; k++)
            if (lens[k]) sink.put(k, dst[k], lens[k]);
    c->sync();
    c->profCollect();
}

static int rp_mem(bfq_ctx *c, const uint8_t *const *text, const uint64_t *text_len, const bfq_repair_opts *opts, uint8_t *const *out, const uint64_t *cap,
                  bool device, bool measure, uint64_t *out_len, uint64_t *n_reads, bfq_repair_stats *stats)
{
    zero3(out_len); zero3(n_reads);
    if (stats) *stats = bfq_repair_stats{};
    return guarded(c, [&] {
        if (!text || !text_len || !out_len || (!measure && (!out || !cap))) throw BfqError{BFQ_E_ARG, "null argument"};
        pr_run_mem(c, out, cap, 3, device, measure, 2, out_len, n_reads, stats, [&](const PrSink &sink, u64 *nr, bfq_repair_stats *S) {
            const bfq_repair_opts O = rp_opts(opts);
            TextIn src[3];
            bfq_texts_of(text, text_len, device, src);
            repair_core(c, src, O, measure, sink, nr, S);
        });
    });
}

extern "C" int bfq_fastq_repair_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint64_t out_len[3],
                                        uint64_t n_reads[3], bfq_repair_stats *stats)
{
    return rp_mem(c, h_text, text_len, opts, nullptr, nullptr, false, true, out_len, n_reads, stats);
}
extern "C" int bfq_fastq_repair(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint8_t *const h_out[3],
                                const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats)
{
    return rp_mem(c, h_text, text_len, opts, h_out, cap, false, false, out_len, n_reads, stats);
}
extern "C" int bfq_fastq_repair_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts,
                                       uint8_t *const d_out[3], const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats)
{
    return rp_mem(c, d_text, text_len, opts, d_out, cap, true, false, out_len, n_reads, stats);
}

extern "C" int bfq_fastq_repair_fd(bfq_ctx *c, const int text_fd[3], const bfq_repair_opts *opts, const int out_fd[3], uint64_t out_len[3], uint64_t n_reads[3],
                                   bfq_repair_stats *stats)
{
    zero3(out_len); zero3(n_reads);
    if (stats) *stats = bfq_repair_stats{};
    return guarded(c, [&] {
        if (!out_len || !text_fd || !out_fd) throw BfqError{BFQ_E_ARG, "null argument"};
        pr_run_fd(c, out_fd, 3, out_len, n_reads, stats, [&](const PrSink &sink, u64 *nr, bfq_repair_stats *S) {
            const bfq_repair_opts O = rp_opts(opts);
            TextIn src[3];
            pr_texts_fd(text_fd, src);
            repair_core(c, src, O, false, sink, nr, S);
        });
    });
}

extern "C" int bfq_fastq_repair_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint8_t *const h_out[3],
                                     const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats)
{
    zero3(out_len); zero3(n_reads);
    if (stats) *stats = bfq_repair_stats{};
    return host_guarded(g_pairsHostErr, [&] {
        if (!text || !text_len || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_repair_opts O = rp_opts(opts);
        const bool measure = !h_out && !cap;
        if (!measure && (!h_out || !cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        if (!measure)
            for (int k = 0; k < 3; k++)
                if (!h_out[k] && cap[k]) throw BfqError{BFQ_E_ARG, "null argument"};
        bfq_repair_stats S;
        bfq_pairs_err X;
        u64 nr[3];
        const int r = bfq_pairs_repair_host(text, text_len, O, h_out, cap, measure, &S, nr, &X);
        if (r == 2) pr_refuse(X);
        for (int k = 0; k < 3; k++) out_len[k] = S.out_len[k];
        if (r == 3) { X.kind = BFQ_PAIRS_E_CAP; X.merge = 2; pr_refuse(X); }
        if (n_reads) for (int k = 0; k < 3; k++) n_reads[k] = nr[k];
        if (stats) *stats = S;
    });
}
