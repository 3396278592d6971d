// bfq_dedup.hip -- exact duplicate removal (include/bfqzip_hip.h, bfq_fastq_dedup*): the host side.  The definition and the
// host form are bfq_dedup.h's; the kernels are k_dedup.hip's.  One call:
//   1  the texts staged as the pairs calls stage theirs (bfq_pairs_stage: looked at, uploaded or taken where they lie, their
//      lines counted, the arena reserved from the counts, the texts indexed with the refusals of every FASTQ entry point)
//   2  hash, sort, the rounds of the grouping (one counter read per round), sizes, winners and statistics, the kept records'
//      sizes and their scan: exact output lengths, and the capacities checked against them.  Up to here nothing of the
//      caller's has been touched
//   3  the move, one copy of every record: into the caller's device buffers, or into the arena and from there through
//      bfq_download (host buffers) or the background writers (files: committed or left empty, OutFiles)
//   arena   per text 8 bytes per line and 44 per record of index; per unit 1 byte of flags that stay, and under them first 113
//           of hashes, scores, two sort records, the sorted g and h, run starts, heads, proposals, groups, group sizes, best
//           scores and winners (+ at most 1 of radix counts), then, in the same space, 32 of sizes and offsets; the outputs
//           unless they are the caller's device buffers
// bfq_fastq_dedup_host runs bfq_dedup.h by one thread, for tests and as the statement of the algorithm: no entry point here
// falls back to it.
#include <string.h>
#include <stdio.h>
#include <sys/stat.h>
#include <functional>
#include "bfq_internal.h"
#include "bfq_dedup.h"

static_assert(sizeof(bfq_dedup_opts) == 24 && sizeof(bfq_dedup_stats) == 616, "the C-ABI's structures");
#define DD_PER_REC 120u

static void dd_refuse(const bfq_dedup_err &X) { throw BfqError{bfq_dedup_code(X), bfq_dedup_message(X)}; }
static bfq_dedup_opts dd_opts(const bfq_dedup_opts *in)
{
    bfq_dedup_opts O;
    bfq_dedup_err X;
    if (!bfq_dedup_resolve(in, &O, &X)) dd_refuse(X);
    return O;
}
static inline void zero2(uint64_t *a) { if (a) a[0] = a[1] = 0; }

extern "C" void bfq_dedup_default_opts(bfq_dedup_opts *o) { if (o) bfq_dedup_defaults(o); }

static thread_local std::string g_dedupHostErr;
extern "C" const char *bfq_dedup_host_error(void) { return g_dedupHostErr.c_str(); }

// what becomes of the outputs 0, 1 (kept) and 2, 3 (removed): sized(len) runs once the lengths are exact and before anything
// is written (it throws for a short capacity, and opens files); want[k]: output k is written; d_dst[k]: the caller's device
// buffer, else the arena and then put()
struct DdSink {
    std::function<void(const u64 *)> sized;
    bool want[4] = {true, true, false, false};
    u8 *d_dst[4] = {nullptr, nullptr, nullptr, nullptr};
    bool device = false;
    std::function<void(int, const u8 *, u64)> put;
};

// src[1] given (paired): the two texts must hold as many records
static void dedup_core(bfq_ctx *c, const TextIn src[2], bool paired, const bfq_dedup_opts &O, bool measure, const DdSink &sink, bfq_dedup_stats *S)
{
    const TextIn s3[3] = {src[0], paired ? src[1] : TextIn{}, TextIn{}};
    PrText t3[3];
    bfq_pairs_stage(c, s3, [](const u8 *first, u64 len, u32 k) {
        bfq_dedup_err X;
        if (!bfq_dedup_gzip_ok(first, len, k, &X)) dd_refuse(X);
    }, "removing duplicates", DD_PER_REC, !measure && !sink.device, t3);
    bfq_dedup_err X;
    if (paired && t3[0].N != t3[1].N) { c->profCollect(); X.kind = BFQ_DEDUP_E_COUNTS; X.n = t3[0].N; X.m = t3[1].N; dd_refuse(X); }
    DdTexts T;
    T.t[0] = t3[0]; T.t[1] = t3[1]; T.nt = paired ? 2u : 1u;
    const u64 N = t3[0].N;
    u8 *kept = c->alloc<u8>(N + 1);
    u64 *d_stat = c->alloc<u64>(DD_S_NUM + 3), stat[DD_S_NUM + 3] = {0};       // behind the statistics: the first bad record, the two kept lengths
    u64 rounds = 0;
    {
        const size_t m = c->mark();
        DdGroups G;
        u64 *h = c->alloc<u64>(N + 1), *score = O.keep ? c->alloc<u64>(N + 1) : nullptr;
        G.sg = c->alloc<u64>(N + 1); G.sh = c->alloc<u64>(N + 1); G.start = c->alloc<u64>(N + 1); G.head = c->alloc<u64>(N + 1); G.next = c->alloc<u64>(N + 1);
        G.rep = c->alloc<u64>(N + 1); G.mixed = c->alloc<u8>(N + 1);
        u64 *gsize = c->alloc<u64>(N + 1), *best = O.keep ? c->alloc<u64>(N + 1) : nullptr, *win = O.keep ? c->alloc<u64>(N + 1) : nullptr;
        SortRec a{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)}, b{c->alloc<u32>(N + 4), c->alloc<u64>(N + 4)};
        bfq_dedup_sort(c, T, N, O, h, score, a, b, G, d_stat);
        while (N) {                                               // round k resolves the k-th different key of every run
            const u64 left = bfq_dedup_round(c, T, N, G, d_stat, rounds == 0);
            rounds++;
            if (!left) break;
            if (rounds < BFQ_DEDUP_KINDS_MAX) continue;
            HIP_CHECK(hipMemsetAsync(d_stat + DD_S_NUM, 0xFF, 8, c->stream));       // a run with more different keys than rounds: refused
            bfq_dedup_first_bad(c, N, G, d_stat + DD_S_NUM);
            HIP_CHECK(hipMemcpyAsync(&X.n, d_stat + DD_S_NUM, 8, hipMemcpyDeviceToHost, c->stream));
            c->sync();
            c->profCollect();
            X.kind = BFQ_DEDUP_E_KINDS;
            dd_refuse(X);
        }
        bfq_dedup_winners(c, N, O.keep, G, score, gsize, best, win, kept, d_stat);
        c->release(m);   // stream-ordered, as in k_scan.hip
    }
    u64 *sz[2], *o[2];
    for (u32 k = 0; k < 2; k++) { sz[k] = k < T.nt ? c->alloc<u64>(N + 1) : nullptr; o[k] = k < T.nt ? c->alloc<u64>(N + 2) : nullptr; }
    bfq_dedup_sizes(c, T, N, kept, sz);
    for (u32 k = 0; k < T.nt; k++) bfq_exscan_u64(c, sz[k], o[k], N, d_stat + DD_S_NUM + 1 + k);
    HIP_CHECK(hipMemcpyAsync(stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    *S = bfq_dedup_stats{};
    S->units = N; S->kept = stat[DD_S_KEPT]; S->removed = N - S->kept;
    S->max_group = stat[DD_S_MAXGROUP]; S->max_group_first = N ? stat[DD_S_FIRST] : 0;
    for (u32 l = 0; l < 32; l++) {
        S->level_groups[l] = stat[DD_S_LGROUPS + l]; S->level_units[l] = stat[DD_S_LUNITS + l];
        if (l) S->dup_groups += S->level_groups[l];
    }
    S->mixed_runs = stat[DD_S_MIXED]; S->max_run = stat[DD_S_MAXRUN]; S->rounds = rounds;
    u64 lens[4] = {0, 0, 0, 0};
    for (u32 k = 0; k < T.nt; k++) {
        lens[k] = S->out_len[k] = N ? stat[DD_S_NUM + 1 + k] : 0;
        lens[2 + k] = S->dup_len[k] = T.t[k].len - lens[k];
    }
    sink.sized(lens);
    if (measure) { c->profCollect(); return; }
    u8 *dst[4];
    for (int k = 0; k < 4; k++) dst[k] = !sink.want[k] ? nullptr : sink.device ? sink.d_dst[k] : c->alloc<u8>(lens[k] + 64);
    const u64 *const off[2] = {o[0], o[1]};
    bfq_dedup_move(c, T, N, kept, off, dst, dst + 2);
    if (!sink.device)
        for (int k = 0; k < 4; k++)
            if (sink.want[k] && lens[k]) sink.put(k, dst[k], lens[k]);
    c->sync();
    c->profCollect();
}

// ---------------------------------------------------------------- the entry points
static void dd_set_lens(const u64 *lens, uint64_t *out_len, uint64_t *dup_len)
{
    for (int k = 0; k < 2; k++) { out_len[k] = lens[k]; dup_len[k] = lens[2 + k]; }
}

static int dd_mem(bfq_ctx *c, const uint8_t *const *text, const uint64_t *text_len, const bfq_dedup_opts *opts, uint8_t *const *out, const uint64_t *out_cap,
                  uint8_t *const *dup, const uint64_t *dup_cap, bool device, bool measure, uint64_t *out_len, uint64_t *dup_len, bfq_dedup_stats *stats)
{
    zero2(out_len); zero2(dup_len);
    if (stats) *stats = bfq_dedup_stats{};
    return guarded(c, [&] {
        if (!text || !text_len || !out_len || !dup_len || (!measure && (!out || !out_cap)) || (dup && !dup_cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        if (!measure)
            for (int k = 0; k < 2; k++)
                if ((!out[k] && out_cap[k]) || (dup && !dup[k] && dup_cap[k])) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_dedup_opts O = dd_opts(opts);
        DdSink sink;
        sink.device = device;
        for (int k = 0; k < 2; k++) {
            sink.want[2 + k] = !measure && dup;
            if (!measure && device) { sink.d_dst[k] = out[k]; sink.d_dst[2 + k] = dup ? dup[k] : nullptr; }
        }
        sink.sized = [&](const u64 *lens) {                        // a short capacity leaves the lengths needed
            if (measure) return;
            bool ok = true;
            for (int k = 0; k < 2; k++) ok = ok && out_cap[k] >= lens[k] && (!dup || dup_cap[k] >= lens[2 + k]);
            if (ok) return;
            dd_set_lens(lens, out_len, dup_len);
            c->profCollect();
            bfq_dedup_err X;
            X.kind = BFQ_DEDUP_E_CAP;
            dd_refuse(X);
        };
        sink.put = [&](int k, const u8 *d_text, u64 len) { bfq_download_phase(c, k < 2 ? out[k] : dup[k - 2], d_text, len); };
        TextIn src[2];
        for (int k = 0; k < 2; k++) {
            if (device) src[k].d = text[k]; else src[k].ref = HostRef::mem(text[k]);
            src[k].len = text[k] ? text_len[k] : 0;
        }
        bfq_dedup_stats S;
        dedup_core(c, src, text[1] != nullptr, O, measure, sink, &S);
        for (int k = 0; k < 2; k++) { out_len[k] = S.out_len[k]; dup_len[k] = S.dup_len[k]; }
        if (stats) *stats = S;
    });
}

extern "C" int bfq_fastq_dedup_measure(bfq_ctx *c, const uint8_t *const h_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint64_t out_len[2],
                                       uint64_t dup_len[2], bfq_dedup_stats *stats)
{
    return dd_mem(c, h_text, text_len, opts, nullptr, nullptr, nullptr, nullptr, false, true, out_len, dup_len, stats);
}
extern "C" int bfq_fastq_dedup(bfq_ctx *c, const uint8_t *const h_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const h_out[2],
                               const uint64_t out_cap[2], uint8_t *const h_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                               bfq_dedup_stats *stats)
{
    return dd_mem(c, h_text, text_len, opts, h_out, out_cap, h_dup, dup_cap, false, false, out_len, dup_len, stats);
}
extern "C" int bfq_fastq_dedup_device(bfq_ctx *c, const uint8_t *const d_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const d_out[2],
                                      const uint64_t out_cap[2], uint8_t *const d_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                                      bfq_dedup_stats *stats)
{
    return dd_mem(c, d_text, text_len, opts, d_out, out_cap, d_dup, dup_cap, true, false, out_len, dup_len, stats);
}

// open files out: opened once the lengths are known, committed at them, and left empty when the call fails (OutFiles)
extern "C" int bfq_fastq_dedup_fd(bfq_ctx *c, const int text_fd[2], const bfq_dedup_opts *opts, const int out_fd[2], const int dup_fd[2], uint64_t out_len[2],
                                  uint64_t dup_len[2], bfq_dedup_stats *stats)
{
    zero2(out_len); zero2(dup_len);
    if (stats) *stats = bfq_dedup_stats{};
    return guarded(c, [&] {
        if (!text_fd || !out_fd || !out_len || !dup_len) throw BfqError{BFQ_E_ARG, "null argument"};
        if (out_fd[0] < 0 || (text_fd[1] >= 0 && out_fd[1] < 0)) throw BfqError{BFQ_E_ARG, "bad file descriptor"};   // (kept records have a place)
        const int fds[4] = {out_fd[0], out_fd[1], dup_fd ? dup_fd[0] : -1, dup_fd ? dup_fd[1] : -1};
        OutFiles F(fds, 4, [c] { bfq_write_wait(c); });
        const bfq_dedup_opts O = dd_opts(opts);
        DdSink sink;
        for (int k = 0; k < 4; k++) sink.want[k] = F.present(k);
        sink.sized = [&](const u64 *lens) {
            F.openAt(lens);
            u64 sum = 0;
            for (int k = 0; k < 4; k++) sum += F.present(k) ? lens[k] : 0;
            c->call.writeHint = (size_t)sum;
        };
        sink.put = [&](int k, const u8 *d_text, u64 len) { bfq_write_async(c, F.at(k, 0), d_text, len); };
        TextIn src[2];
        for (int k = 0; k < 2; k++) {                               // a text is as long as its file
            if (text_fd[k] < 0) continue;
            struct stat st;
            if (fstat(text_fd[k], &st) != 0) throw BfqError{BFQ_E_IO, std::string("cannot stat a text file: ") + strerror(errno)};
            src[k].ref = HostRef::file(text_fd[k]); src[k].len = (u64)st.st_size;
        }
        bfq_dedup_stats S;
        dedup_core(c, src, text_fd[1] >= 0, O, false, sink, &S);
        bfq_phase("d2h_write");
        const u64 lens[4] = {S.out_len[0], S.out_len[1], S.dup_len[0], S.dup_len[1]};
        F.commit(lens);
        dd_set_lens(lens, out_len, dup_len);
        if (stats) *stats = S;
    });
}

extern "C" int bfq_fastq_dedup_host(const uint8_t *const text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const h_out[2],
                                    const uint64_t out_cap[2], uint8_t *const h_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                                    bfq_dedup_stats *stats)
{
    zero2(out_len); zero2(dup_len);
    if (stats) *stats = bfq_dedup_stats{};
    return host_guarded(g_dedupHostErr, [&] {
        if (!text || !text_len || !out_len || !dup_len || (h_dup && !dup_cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_dedup_opts O = dd_opts(opts);
        const bool measure = !h_out && !out_cap;
        if (!measure && (!h_out || !out_cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        if (!measure)
            for (int k = 0; k < 2; k++)
                if ((!h_out[k] && out_cap[k]) || (h_dup && !h_dup[k] && dup_cap[k])) throw BfqError{BFQ_E_ARG, "null argument"};
        bfq_dedup_stats S;
        bfq_dedup_err X;
        const int r = bfq_dedup_host(text, text_len, O, h_out, out_cap, h_dup, dup_cap, measure, &S, &X);
        if (r == 2) dd_refuse(X);
        for (int k = 0; k < 2; k++) { out_len[k] = S.out_len[k]; dup_len[k] = S.dup_len[k]; }
        if (r == 3) { X.kind = BFQ_DEDUP_E_CAP; dd_refuse(X); }
        if (stats) *stats = S;
    });
}
