// bfq_compare.hip -- two FASTQ texts in, one report out (include/bfqzip_hip.h, bfq_fastq_compare*): what a run changed.  The
// kernels are k_compare.hip's; this file moves the bytes and sizes the memory:
//   text buffer  A's parts back to back, then B's (256-byte aligned), uploaded through the staging workers
//   arena        both line and record indexes, the permutation and its inverse when one is given, the per-read counts and
//                their scan, the report, the diff records that were asked for
// Nothing is gathered: the compare reads the lines where they lie in the texts.  The caller's report is written once, at the
// end; a refusal leaves it zeroed and the diff buffer untouched.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_perm.h"

using CmpSrc = TextSrc;
struct CmpInput { const CmpSrc *parts; int nparts; u64 len; TextMeasure M; };   // len: a bound once measured, the length once placed

static void cmp_nomem(bfq_ctx *c, size_t need) { bfq_nomem_cap(c, "comparing", "both texts + index + diff records", need); }

// the length a text has on the device (the shared pair of bfq_bgzf.hip: a part that lacks its final newline gets one, a
// BGZF part is inflated); what is refused is passed on with the input's name in front
static void cmp_measure(CmpInput &in, const char *which)
{
    try { bfq_text_measure(in.parts, in.nparts, &in.M); }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw BfqError{e.code, std::string(which) + ": " + e.msg}; }
    in.len = in.M.bound;
}
static void cmp_upload(bfq_ctx *c, CmpInput &in, const char *which, u8 *d_dst, u8 *d_stage)
{
    u64 ps[BFQ_MAX_PARTS + 1];
    try { bfq_text_put(c, in.parts, &in.M, d_dst, d_stage, ps); }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw BfqError{e.code, std::string(which) + ": " + e.msg}; }
    in.len = ps[in.nparts];
}
// the record index of one text; what the parser refuses is passed on with the input's name in front
static void cmp_index(bfq_ctx *c, const char *which, const u8 *d_text, u64 len, DevFastq *fq)
{
    c->zeroCounters();
    try { bfq_fastq_index(c, d_text, len, fq); }
    catch (const BfqError &e) { throw BfqError{e.code, std::string(which) + ": " + e.msg}; }
}

static void compare_core(bfq_ctx *c, CmpInput A, CmpInput B, const u8 *h_permz, u64 permzLen, bool havePerm, bfq_compare_report *rep,
                         bfq_compare_diff *h_diffs, u64 capDiffs)
{
    cmp_measure(A, "A");
    cmp_measure(B, "B");
    u64 PN = 0;
    if (havePerm && !bfq_perm_header(h_permz, permzLen, &PN, nullptr, nullptr))
        throw BfqError{BFQ_E_ARG, "perm: not a BFQPERM1 container (magic, entry width, length or padding)"};
    const u64 offB = (A.len + 64 + 255) & ~255ull, sum = offB + ((B.len + 64 + 255) & ~255ull);   // every text 256-byte aligned and padded
    const u64 stage = std::max(A.M.stage, B.M.stage);           // a BGZF part's compressed bytes: behind both texts
    if (c->wsLimit() && sum + stage > c->wsLimit()) cmp_nomem(c, sum + stage);
    bfq_phase("alloc");
    u8 *d_a = c->textBuf(sum + stage + 64), *d_b = d_a + offB;
    bfq_phase("read_h2d");
    cmp_upload(c, A, "A", d_a, d_a + sum);
    cmp_upload(c, B, "B", d_b, d_a + sum);
    bfq_phase("alloc");
    const u64 maxLen = std::max(A.len, B.len);
    c->reserve(bfq_count_lines_bytes(maxLen) + (64u << 20));
    bfq_phase("gpu");
    const u64 nlA = bfq_fastq_count_lines(c, d_a, A.len), nlB = bfq_fastq_count_lines(c, d_b, B.len);
    const u64 Nb = std::max(nlA, nlB) / 4 + 1;
    // per text: line ends, chunk counts of the line index, records + read offsets + lengths, the scans' partial sums; once: the
    // container's payload, the permutation and its inverse, the per-read counts and their scan, the report, the diff records
    const u64 diffCap = std::min(capDiffs, A.len / 2);            // a text of len bytes has at most len / 2 bases
    // (slack, as reserved so far: 16 bytes per read, 16 per chunk of text where the line kernels take 12, and 4 KiB)
    const size_t perText = bfq_fastq_index_bytes(maxLen, std::max(nlA, nlB)) + 16 * (size_t)(Nb + 64) + 4 * (size_t)(maxLen / BFQ_NL_CHUNK) + 4096;
    const size_t need = 2 * perText + (havePerm ? 24 : 0) * (size_t)(Nb + 64) + (4 + 8) * (size_t)(Nb + 64) + (size_t)(Nb >> 7) + sizeof(bfq_compare_report) +
                        16 * (size_t)diffCap + (8u << 20);
    if (c->wsLimit() && sum + need > c->wsLimit()) cmp_nomem(c, sum + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    DevFastq fa, fb;
    cmp_index(c, "A", d_a, A.len, &fa);
    cmp_index(c, "B", d_b, B.len, &fb);
    const u64 N = fa.N;
    if (fb.N != N) {
        char b[200];
        snprintf(b, sizeof b, "the texts differ in their number of records: %llu in A, %llu in B", (unsigned long long)N, (unsigned long long)fb.N);
        throw BfqError{BFQ_E_ARG, b};
    }
    const u64 *inv = nullptr;
    if (havePerm) {
        if (PN != N) {
            char b[200];
            snprintf(b, sizeof b, "perm: a permutation of %llu reads for texts of %llu records", (unsigned long long)PN, (unsigned long long)N);
            throw BfqError{BFQ_E_ARG, b};
        }
        const u64 nw = bfq_perm_words(N, bfq_perm_width(N));
        u64 *words = c->alloc<u64>(nw + 1), *perm = c->alloc<u64>(N + 1), *iv = c->alloc<u64>(N + 1);
        if (nw) bfq_upload(c, words, h_permz + BFQ_PERM_HDR, 8 * nw);
        const u64 bad = bfq_perm_unpack_invert(c, words, N, perm, iv);
        if (bad != BFQ_PERM_NOPOS) {
            char b[200];
            snprintf(b, sizeof b, "perm: not a permutation: entry %llu is out of range or repeats an earlier one", (unsigned long long)bad);
            throw BfqError{BFQ_E_ARG, b};
        }
        inv = iv;
    }
    const CmpText ta{d_a, (const FqRec *)fa.rec}, tb{d_b, (const FqRec *)fb.rec};
    bfq_compare_report *d_rep = c->alloc<bfq_compare_report>(1);
    u64 *d_bad = c->alloc<u64>(1);
    u32 *readDiffs = c->alloc<u32>(N + 1);
    HIP_CHECK(hipMemsetAsync(d_rep, 0, sizeof *d_rep, c->stream));
    HIP_CHECK(hipMemsetAsync(&d_rep->first_changed_read, 0xFF, 8, c->stream));
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    // pass 1: the pairs fit (or the first one that does not), the header classes
    bfq_compare_check(c, ta, tb, inv, N, d_rep, d_bad);
    u64 bad = ~0ull;
    HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (bad != ~0ull) {
        u64 j = bad;
        FqRec ra, rb;
        if (inv) HIP_CHECK(hipMemcpyAsync(&j, inv + bad, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(&ra, ta.rec + bad, sizeof ra, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        HIP_CHECK(hipMemcpyAsync(&rb, tb.rec + j, sizeof rb, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        char b[200];
        snprintf(b, sizeof b, "read %llu: its sequence has %u bases in A and %u in B", (unsigned long long)bad, ra.len, rb.len);
        throw BfqError{BFQ_E_ARG, b};
    }
    // pass 2: the counts
    bfq_compare_pass(c, ta, tb, inv, N, fa.total, d_rep, readDiffs);
    bfq_compare_report R;
    HIP_CHECK(hipMemcpyAsync(&R, d_rep, sizeof R, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    R.n_reads = N;
    R.total_bases = fa.total;
    // pass 3: the first differing positions
    const u64 nout = std::min(std::min((u64)R.n_diffs, capDiffs), diffCap);
    if (nout) {
        u64 *diffOff = c->alloc<u64>(N + 2);
        bfq_compare_diff *d_diffs = c->alloc<bfq_compare_diff>(nout);
        bfq_exscan_u32(c, readDiffs, diffOff, N, nullptr);
        bfq_compare_emit(c, ta, tb, inv, N, fa.total, readDiffs, diffOff, nout, d_diffs);
        bfq_phase("d2h_write");
        bfq_download(c, h_diffs, d_diffs, sizeof(bfq_compare_diff) * nout);
    }
    c->sync();
    c->profCollect();
    *rep = R;
}

static void cmp_check_args(const void *a, int na, const void *b, int nb, bfq_compare_report *rep, bfq_compare_diff *h_diffs, u64 capDiffs)
{
    if (!rep) throw BfqError{BFQ_E_ARG, "null argument"};
    if (!a || !b || na < 1 || na > BFQ_MAX_PARTS || nb < 1 || nb > BFQ_MAX_PARTS) throw BfqError{BFQ_E_ARG, "bfq_fastq_compare: 1..BFQ_MAX_PARTS parts for each of A and B"};
    if (capDiffs && !h_diffs) throw BfqError{BFQ_E_ARG, "bfq_fastq_compare: cap_diffs without a buffer"};
}

extern "C" int bfq_fastq_compare(bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb, const uint8_t *h_permz,
                                 uint64_t permz_len, bfq_compare_report *rep, bfq_compare_diff *h_diffs, uint64_t cap_diffs)
{
    if (rep) memset(rep, 0, sizeof *rep);
    return guarded(c, [&] {
        cmp_check_args(a, na, b, nb, rep, h_diffs, cap_diffs);
        CmpSrc sa[BFQ_MAX_PARTS], sb[BFQ_MAX_PARTS];
        for (int p = 0; p < na; p++) sa[p] = CmpSrc{HostRef::mem(a[p].data), a[p].len};
        for (int p = 0; p < nb; p++) sb[p] = CmpSrc{HostRef::mem(b[p].data), b[p].len};
        CmpInput A{sa, na, 0, {}}, B{sb, nb, 0, {}};
        try { compare_core(c, A, B, h_permz, permz_len, h_permz != nullptr || permz_len != 0, rep, h_diffs, cap_diffs); }
        catch (...) { memset(rep, 0, sizeof *rep); throw; }
    });
}

extern "C" int bfq_fastq_compare_fd(bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, int perm_fd, uint64_t permz_len,
                                    bfq_compare_report *rep, bfq_compare_diff *h_diffs, uint64_t cap_diffs)
{
    if (rep) memset(rep, 0, sizeof *rep);
    return guarded(c, [&] {
        cmp_check_args(&a_fd, 1, &b_fd, 1, rep, h_diffs, cap_diffs);
        if (a_fd < 0 || b_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        std::vector<u8> permz;                                    // a container is ~3 bytes per read: read whole
        if (perm_fd >= 0) {
            permz.resize(permz_len);
            u64 got = 0;
            while (got < permz_len) {
                const ssize_t r = pread(perm_fd, permz.data() + got, (size_t)(permz_len - got), (off_t)got);
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) break;
                got += (u64)r;
            }
            if (got != permz_len) throw BfqError{BFQ_E_ARG, "perm: the file is shorter than permz_len"};
        }
        const CmpSrc sa{HostRef::file(a_fd), a_len}, sb{HostRef::file(b_fd), b_len};
        CmpInput A{&sa, 1, 0, {}}, B{&sb, 1, 0, {}};
        try { compare_core(c, A, B, permz.data(), permz_len, perm_fd >= 0, rep, h_diffs, cap_diffs); }
        catch (...) { memset(rep, 0, sizeof *rep); throw; }
    });
}
