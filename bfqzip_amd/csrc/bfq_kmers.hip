// bfq_kmers.hip -- one or two FASTQ texts in, their k-mer spectrum out (include/bfqzip_hip.h, bfq_fastq_kmers*).  The kernels
// are k_kmers.hip's; this file moves the bytes, cuts the value ranges and sizes the memory:
//   text buffer  A's parts back to back, then B's (256-byte aligned), uploaded through the staging workers, as the compare's
//   arena        fixed: both record indexes, one count and one place per read of both texts, the histogram of the 4096 bins,
//                  the report, the list entries that were asked for (at most one per valid window)
//                per record of the largest range: two sort buffers of 12 bytes (the heads of the runs go into the one the
//                  sort left free), the radix passes' 12 x 256 bytes per block, the run kernels' counts per chunk
// Memory of a call = text buffer + fixed + range(R), R = the records of the largest range.  With part_records = 0, R is the
// largest the limit leaves room for -- the limit: ws_cap_mib, or without one 90 % of what the device has free beside the text
// buffer -- and never above KM_MAX_PART.  A range is at least one bin: a bin that does not fit is refused by its size.
// Nothing is gathered: the windows are read where they lie in the texts.  The caller's report and list are written once, at
// the end; a refusal leaves the report zeroed and the list untouched.
#include <string.h>
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_kmers.h"

static_assert(sizeof(bfq_kmer_opts) == 24 && sizeof(bfq_kmer_entry) == 16 && sizeof(bfq_kmer_report) == 8 * (21 + 256 + 256 + 256 + 9 + 8), "the C-ABI's structures");

struct KmInput { const TextSrc *parts; int nparts; u64 len; TextMeasure M; };   // len: a bound once measured, the length once placed

static void km_prefix(const BfqError &e, const char *which, bool all) { if (!all && e.code != BFQ_E_ARG) throw e; throw BfqError{e.code, std::string(which) + ": " + e.msg}; }
static void km_measure(KmInput &in, const char *which)
{
    try { bfq_text_measure(in.parts, in.nparts, &in.M); }
    catch (const BfqError &e) { km_prefix(e, which, false); }
    in.len = in.M.bound;
}
static void km_upload(bfq_ctx *c, KmInput &in, const char *which, u8 *d_dst, u8 *d_stage)
{
    u64 ps[BFQ_MAX_PARTS + 1];
    try { bfq_text_put(c, in.parts, &in.M, d_dst, d_stage, ps); }
    catch (const BfqError &e) { km_prefix(e, which, false); }
    in.len = ps[in.nparts];
}
static void km_index(bfq_ctx *c, const char *which, const u8 *d_text, u64 len, DevFastq *fq)
{
    c->zeroCounters();
    try { bfq_fastq_index(c, d_text, len, fq); }
    catch (const BfqError &e) { km_prefix(e, which, true); }
}

// arena bytes of one range of R records: the two sort buffers (with the slack the tiles read into), bfq_radix_sort's counts
// and places per block and their scan, bfq_kmers_runs' buffers
static size_t km_range_bytes(u64 R)
{
    const u64 nb = ceil_div(R, bfq_radix_block_elems(R));
    return 2 * (bfq_align256(4 * (R + 64)) + bfq_align256(8 * (R + 64))) + bfq_align256(4 * 256 * nb) + bfq_align256(8 * 256 * nb) + bfq_scan_bytes(256 * nb) +
           bfq_kmers_seg_bytes(R) + 4096;
}

static void kmers_core(bfq_ctx *c, KmInput A, KmInput B, bool haveB, const bfq_kmer_opts &O, bfq_kmer_report *rep, bfq_kmer_entry *h_list, u64 capList)
{
    const char *what = "counting k-mers";
    km_measure(A, "A");
    if (haveB) km_measure(B, "B");
    const u64 offB = (A.len + 64 + 255) & ~255ull, sum = offB + (haveB ? (B.len + 64 + 255) & ~255ull : 0);
    const u64 stage = std::max(A.M.stage, haveB ? B.M.stage : 0);
    if (c->wsLimit() && sum + stage > c->wsLimit()) bfq_nomem_cap(c, what, "the texts", sum + stage);
    bfq_phase("alloc");
    u8 *d_a = c->textBuf(sum + stage + 64), *d_b = d_a + offB;
    bfq_phase("read_h2d");
    km_upload(c, A, "A", d_a, d_a + sum);
    if (haveB) km_upload(c, B, "B", d_b, d_a + sum);
    bfq_phase("alloc");
    const u64 maxLen = std::max(A.len, haveB ? B.len : 0);
    c->reserve(bfq_count_lines_bytes(maxLen) + (64u << 20));
    bfq_phase("gpu");
    const u64 nlA = bfq_fastq_count_lines(c, d_a, A.len), nlB = haveB ? bfq_fastq_count_lines(c, d_b, B.len) : 0;
    const u64 Nb = nlA / 4 + nlB / 4 + 2;                          // reads of both texts
    const u64 listCap = std::min(capList, (A.len + (haveB ? B.len : 0)) / 2);   // a text of len bytes has at most len / 2 windows
    const size_t fixed = bfq_fastq_index_bytes(A.len, nlA) + (haveB ? bfq_fastq_index_bytes(B.len, nlB) : 0) + 2 * (16 * (size_t)(Nb + 64) +
                         4 * (size_t)(maxLen / BFQ_NL_CHUNK) + 4096) + bfq_align256(4 * Nb) + bfq_align256(8 * (Nb + 1)) + bfq_scan_bytes(Nb) + 8 * (KM_BINS + 8) +
                         sizeof(bfq_kmer_report) + bfq_align256(16 * (size_t)listCap) + (1u << 20);
    size_t limit = c->wsLimit();
    if (!limit) {
        size_t fr = 0, tot = 0;
        HIP_CHECK(hipMemGetInfo(&fr, &tot));
        limit = sum + (size_t)((double)(fr + c->ws.cap) * 0.9);
    }
    if (sum + fixed + km_range_bytes(1) > limit) {
        if (c->wsLimit()) bfq_nomem_cap(c, what, "the texts + their index + one sort record", sum + fixed + km_range_bytes(1));
        throw BfqError{BFQ_E_NOMEM, "counting k-mers: the texts and their index do not fit the device's free memory"};
    }
    // the most records a range may hold (halving search: km_range_bytes grows with R)
    u64 roomR = 1;
    for (u64 step = 1ull << 40; step; step >>= 1)
        if (roomR + step <= KM_MAX_PART && sum + fixed + km_range_bytes(roomR + step) <= limit) roomR += step;

    // the fixed part: indexes, the first pass
    struct Fixed { DevFastq fa, fb; u32 *cnt; u64 *off, *d_hist, *d_scal; bfq_kmer_report *d_rep; bfq_kmer_entry *d_list; };
    auto lay = [&](size_t bytes) {
        Fixed F{};
        bfq_phase("alloc");
        c->reserve(bytes);
        bfq_phase("gpu");
        km_index(c, "A", d_a, A.len, &F.fa);
        if (haveB) km_index(c, "B", d_b, B.len, &F.fb);
        F.cnt = c->alloc<u32>(F.fa.N + F.fb.N + 1);
        F.off = c->alloc<u64>(F.fa.N + F.fb.N + 2);
        F.d_hist = c->alloc<u64>(KM_BINS + 8);
        F.d_scal = F.d_hist + KM_BINS;
        F.d_rep = c->alloc<bfq_kmer_report>(1);
        F.d_list = listCap ? c->alloc<bfq_kmer_entry>(listCap) : nullptr;
        return F;
    };
    Fixed F = lay(fixed + km_range_bytes(1));
    KmText ta{d_a, (const FqRec *)F.fa.rec, F.fa.N}, tb{d_b, (const FqRec *)F.fb.rec, F.fb.N};
    u64 hist[KM_BINS + 8];
    HIP_CHECK(hipMemsetAsync(F.d_hist, 0, 8 * (KM_BINS + 8), c->stream));
    bfq_kmers_hist(c, ta, O.k, O.canonical, F.fa.total, F.d_hist, F.d_scal);
    if (haveB) bfq_kmers_hist(c, tb, O.k, O.canonical, F.fb.total, F.d_hist, F.d_scal + 3);
    HIP_CHECK(hipMemcpyAsync(hist, F.d_hist, 8 * (KM_BINS + 8), hipMemcpyDeviceToHost, c->stream));
    c->sync();
    bfq_kmer_report R;
    memset(&R, 0, sizeof R);
    R.k = O.k; R.solid = O.solid; R.canonical = O.canonical;
    R.n_reads_a = F.fa.N; R.reads_short_a = hist[KM_BINS]; R.windows_a = hist[KM_BINS + 1]; R.windows_skipped_a = hist[KM_BINS + 2];
    R.n_reads_b = F.fb.N; R.reads_short_b = hist[KM_BINS + 3]; R.windows_b = hist[KM_BINS + 4]; R.windows_skipped_b = hist[KM_BINS + 5];

    // the ranges
    const std::vector<KmRange> ranges = bfq_kmer_ranges(hist, O.part_records ? std::min<u64>(O.part_records, roomR) : roomR);
    u64 maxR = 0;
    for (const KmRange &r : ranges) {
        if (r.records > roomR) {                                  // one bin that is larger than the room
            char b[240];
            snprintf(b, sizeof b, "counting k-mers: bin %u of the k-mers' top 12 bits alone holds %llu windows, and %.2f GiB of device memory (%s) leave room "
                     "for %llu sort records", r.lo, (unsigned long long)r.records, limit / 1073741824.0,
                     c->wsLimit() ? "the cap: bfq_params.ws_cap_mib / BFQ_WS_CAP" : "what the device has free", (unsigned long long)roomR);
            throw BfqError{BFQ_E_NOMEM, b};
        }
        maxR = std::max(maxR, r.records);
    }
    R.n_partitions = ranges.size();
    const size_t need = fixed + km_range_bytes(std::max<u64>(maxR, 1));
    if (need > c->ws.cap) {                                        // the arena grows: the indexes are made again in the new one
        F = lay(need);
        ta.rec = (const FqRec *)F.fa.rec; tb.rec = (const FqRec *)F.fb.rec;
    }
    HIP_CHECK(hipMemsetAsync(F.d_rep, 0, sizeof R, c->stream));
    const u64 NA = F.fa.N, NB = F.fb.N;
    const size_t top = c->mark();
    for (const KmRange &r : ranges) {
        const u64 n = r.records;
        bfq_kmers_count(c, ta, O.k, O.canonical, r.lo, r.hi, F.fa.total, F.cnt);
        if (haveB) bfq_kmers_count(c, tb, O.k, O.canonical, r.lo, r.hi, F.fb.total, F.cnt + NA);
        bfq_exscan_u32(c, F.cnt, F.off, NA + NB, nullptr);
        SortRec a{c->alloc<u32>(n + 64), c->alloc<u64>(n + 64)}, b{c->alloc<u32>(n + 64), c->alloc<u64>(n + 64)};
        bfq_kmers_emit(c, ta, O.k, O.canonical, r.lo, r.hi, 0, F.fa.total, n, F.off, a);
        if (haveB) bfq_kmers_emit(c, tb, O.k, O.canonical, r.lo, r.hi, 1, F.fb.total, n, F.off + NA, a);
        const SortRec s = bfq_kmers_sort(c, a, b, n, O.k);
        bfq_kmers_runs(c, s, n, O.k, O.solid, s.w0 == a.w0 ? b.w12 : a.w12, F.d_rep, F.d_list, listCap);
        c->release(top);
    }
    bfq_kmer_report D;
    HIP_CHECK(hipMemcpyAsync(&D, F.d_rep, sizeof D, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    memcpy(&R.distinct_a, &D.distinct_a, sizeof R - offsetof(bfq_kmer_report, distinct_a));
    const u64 nout = std::min<u64>(R.n_listed, listCap);
    if (nout) bfq_download_phase(c, h_list, F.d_list, sizeof(bfq_kmer_entry) * nout);
    c->sync();
    c->profCollect();
    *rep = R;
}

static bfq_kmer_opts km_check_args(const void *a, int na, const void *b, int nb, const bfq_kmer_opts *opts, bfq_kmer_report *rep, bfq_kmer_entry *h_list, u64 capList)
{
    if (!rep) throw BfqError{BFQ_E_ARG, "null argument"};
    if (!a || na < 1 || na > BFQ_MAX_PARTS || nb < 0 || nb > BFQ_MAX_PARTS || (nb && !b))
        throw BfqError{BFQ_E_ARG, "bfq_fastq_kmers: 1..BFQ_MAX_PARTS parts for A, 0..BFQ_MAX_PARTS for B"};
    if (capList && !h_list) throw BfqError{BFQ_E_ARG, "bfq_fastq_kmers: cap_list without a buffer"};
    bfq_kmer_opts O;
    if (const char *why = bfq_kmer_resolve(opts, &O)) throw BfqError{BFQ_E_ARG, why};
    return O;
}

extern "C" int bfq_fastq_kmers(bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb, const bfq_kmer_opts *opts, bfq_kmer_report *rep,
                               bfq_kmer_entry *h_list, uint64_t cap_list)
{
    if (rep) memset(rep, 0, sizeof *rep);
    return guarded(c, [&] {
        const bfq_kmer_opts O = km_check_args(a, na, b, nb, opts, rep, h_list, cap_list);
        TextSrc sa[BFQ_MAX_PARTS], sb[BFQ_MAX_PARTS];
        for (int p = 0; p < na; p++) sa[p] = TextSrc{HostRef::mem(a[p].data), a[p].len};
        for (int p = 0; p < nb; p++) sb[p] = TextSrc{HostRef::mem(b[p].data), b[p].len};
        KmInput A{sa, na, 0, {}}, B{sb, nb, 0, {}};
        try { kmers_core(c, A, B, nb > 0, O, rep, h_list, cap_list); }
        catch (...) { memset(rep, 0, sizeof *rep); throw; }
    });
}

extern "C" int bfq_fastq_kmers_fd(bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, const bfq_kmer_opts *opts, bfq_kmer_report *rep,
                                  bfq_kmer_entry *h_list, uint64_t cap_list)
{
    if (rep) memset(rep, 0, sizeof *rep);
    return guarded(c, [&] {
        const bfq_kmer_opts O = km_check_args(&a_fd, 1, &b_fd, b_fd >= 0 ? 1 : 0, opts, rep, h_list, cap_list);
        if (a_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        const TextSrc sa{HostRef::file(a_fd), a_len}, sb{HostRef::file(b_fd), b_len};
        KmInput A{&sa, 1, 0, {}}, B{&sb, 1, 0, {}};
        try { kmers_core(c, A, B, b_fd >= 0, O, rep, h_list, cap_list); }
        catch (...) { memset(rep, 0, sizeof *rep); throw; }
    });
}
