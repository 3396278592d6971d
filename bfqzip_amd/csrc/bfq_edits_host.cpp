// bfq_edits_host.cpp -- the BFQEDIT1 container stated on the host (include/bfqzip_hip.h; layout and arithmetic: bfq_edits.h):
// bound, info, encode, decode, and the one-thread forms of making a run's edits from two FASTQ texts and of applying them to
// a text.  They are what the kernels of k_edits.hip are tested against; no entry point falls back to them.  No context, no GPU.
#include <string.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "bfq_internal_host.h"
#include "bfq_edits.h"

static thread_local std::string g_editsHostErr;
extern "C" const char *bfq_edits_host_error(void) { return g_editsHostErr.c_str(); }

extern "C" uint64_t bfq_edits_bound(uint64_t n_edits, uint64_t total_bases) { return bfq_edits_bound_of(n_edits, total_bases); }

extern "C" int64_t bfq_edits_member_len(const uint8_t *h_edits, uint64_t len)
{
    BfqEditMember M;
    return bfq_edits_member(h_edits, len, &M, nullptr) ? -1 : (int64_t)M.bytes();
}

extern "C" int bfq_edits_info(const uint8_t *h_edits, uint64_t len, uint64_t *n_reads, uint64_t *total_bases, uint64_t *n_edits, uint64_t *members)
{
    if (n_reads) *n_reads = 0;
    if (total_bases) *total_bases = 0;
    if (n_edits) *n_edits = 0;
    if (members) *members = 0;
    return host_guarded(g_editsHostErr, [&] {
        u64 N = 0, T = 0, E = 0, m = 0, at = 0;
        if (!h_edits || !len) throw BfqError{BFQ_E_ARG, "not a BFQEDIT1 container (magic)"};
        while (at < len) {
            BfqEditMember M;
            if (const char *e = bfq_edits_member(h_edits + at, len - at, &M, nullptr)) {
                char b[160];
                snprintf(b, sizeof b, "member %llu: %s", (unsigned long long)m, e);
                throw BfqError{BFQ_E_ARG, b};
            }
            N = N + M.N < N ? ~0ull : N + M.N;                    // (the sums saturate)
            T = T + M.T < T ? ~0ull : T + M.T;
            E += M.E; m++;
            at += M.bytes();
        }
        if (n_reads) *n_reads = N;
        if (total_bases) *total_bases = T;
        if (n_edits) *n_edits = E;
        if (members) *members = m;
    });
}

extern "C" int bfq_edits_encode(const uint64_t *h_pos, const uint8_t *h_byte, uint64_t n_edits, uint64_t n_reads, uint64_t total_bases,
                                uint64_t shape, uint64_t target_sum, uint8_t *h_out, uint64_t cap, uint64_t *out_len)
{
    return bfq_edits_encode_host((const u64 *)h_pos, h_byte, n_edits, n_reads, total_bases, shape, target_sum, h_out, cap, (u64 *)out_len);
}

extern "C" int bfq_edits_decode(const uint8_t *h_edits, uint64_t len, uint64_t *h_pos, uint8_t *h_byte, uint64_t cap_entries,
                                uint64_t *n_reads, uint64_t *total_bases, uint64_t *n_edits, uint64_t *shape, uint64_t *target_sum,
                                uint64_t *first_bad)
{
    BfqEditMember M;
    const char *why = nullptr;
    const int rc = bfq_edits_decode_host(h_edits, len, (u64 *)h_pos, h_byte, cap_entries, &M, (u64 *)first_bad, &why);
    g_editsHostErr = why ? why : "";
    if (rc != BFQ_OK) return rc;
    if (n_reads) *n_reads = M.N;
    if (total_bases) *total_bases = M.T;
    if (n_edits) *n_edits = M.E;
    if (shape) *shape = M.shape;
    if (target_sum) *target_sum = M.targetSum;
    return BFQ_OK;
}

namespace {
// the sequence lines of a FASTQ text: a text that lacks its final newline is read as if it had one
struct EdHostText {
    std::vector<u64> start;                                       // of every read's sequence in the text
    std::vector<u32> len;
    u64 total = 0;
};
void ed_host_index(const u8 *t, u64 n, const char *which, EdHostText &X)
{
    auto refuse = [&](int code, const char *m) { throw BfqError{code, std::string(which) + m}; };
    std::vector<u64> ends;
    for (u64 i = 0; i < n; i++)
        if (t[i] == 10) ends.push_back(i);
    if (n && t[n - 1] != 10) ends.push_back(n);
    if (ends.size() % 4) refuse(BFQ_E_ARG, "FASTQ: number of lines is not a multiple of 4");
    const u64 N = ends.size() / 4;
    auto line = [&](u64 li, u64 *s, u64 *e) {
        *s = li ? ends[li - 1] + 1 : 0;
        *e = ends[li];
        if (*e > *s && t[*e - 1] == 13) --*e;
    };
    for (u64 i = 0; i < N; i++) {
        u64 s, e, qs, qe;
        line(4 * i + 1, &s, &e);
        line(4 * i + 3, &qs, &qe);
        if (qe - qs != e - s) refuse(BFQ_E_ARG, "FASTQ: len(DNA) != len(QS) in a record");
        if (e - s > BFQ_MAX_READ_LEN) refuse(BFQ_E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN");
        X.start.push_back(s);
        X.len.push_back((u32)(e - s));
        X.total += e - s;
    }
}
[[noreturn]] void ed_refuse(const char *fmt, unsigned long long a, unsigned long long b, unsigned long long c = 0)
{
    char m[240];
    snprintf(m, sizeof m, fmt, a, b, c);
    throw BfqError{BFQ_E_ARG, m};
}
}   // namespace

extern "C" int bfq_fastq_edits_host(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, uint8_t *h_out, uint64_t cap,
                                    uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return host_guarded(g_editsHostErr, [&] {
        if ((!a && a_len) || (!b && b_len) || !h_out || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        EdHostText A, B;
        ed_host_index(a, a_len, "A: ", A);
        ed_host_index(b, b_len, "B: ", B);
        const u64 N = A.len.size();
        if (B.len.size() != N) ed_refuse("the texts differ in their number of records: %llu in A, %llu in B", N, B.len.size());
        for (u64 r = 0; r < N; r++)
            if (A.len[r] != B.len[r]) ed_refuse("read %llu: its sequence has %llu bases in A and %llu in B", r, A.len[r], B.len[r]);
        std::vector<u64> pos;
        std::vector<u8> byte;
        u64 shape = 0, tsum = 0, g0 = 0, touched = 0;
        for (u64 r = 0; r < N; r++) {
            shape += bfq_edit_shape_term(r, A.len[r]);
            const u8 *sa = a + A.start[r], *sb = b + B.start[r];
            bool any = false;
            for (u32 j = 0; j < A.len[r]; j++)
                if (sa[j] != sb[j]) {
                    if (!bfq_edit_byte_ok(sa[j])) ed_refuse("read %llu: the byte at base %llu of A is outside 33..126", r, j);
                    pos.push_back(g0 + j); byte.push_back(sa[j]);
                    tsum += bfq_edit_sum_term(g0 + j, sb[j]);
                    any = true;
                }
            touched += any;
            g0 += A.len[r];
        }
        u64 ol = 0;
        if (bfq_edits_encode_host(pos.data(), byte.data(), pos.size(), N, A.total, shape, tsum, h_out, cap, &ol) != BFQ_OK)
            ed_refuse("the container needs %llu bytes, the buffer has %llu", bfq_edits_bound_of(pos.size(), A.total), cap);
        *out_len = ol;
        if (stats) { stats->reads = N; stats->bases = A.total; stats->edits = pos.size(); stats->reads_touched = touched; stats->bytes = ol; }
    });
}

extern "C" int bfq_fastq_unedit_host(const uint8_t *text, uint64_t len, const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out,
                                     uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return host_guarded(g_editsHostErr, [&] {
        if ((!text && len) || !h_edits || !h_out || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        EdHostText X;
        ed_host_index(text, len, "", X);
        const u64 N = X.len.size();
        std::vector<u64> roff(N + 1, 0);
        for (u64 r = 0; r < N; r++) roff[r + 1] = roff[r] + X.len[r];
        // every member is decoded and checked against the text before a byte is written
        std::vector<u64> pos;
        std::vector<u8> byte;
        u64 at = 0, m = 0, r0 = 0, E = 0, touched = 0;
        while (at < edits_len || !m) {
            BfqEditMember M;
            if (const char *e = bfq_edits_member(h_edits + at, edits_len - at, &M, nullptr)) ed_refuse((std::string("edits member %llu: ") + e).c_str(), m, 0);
            pos.resize(E + M.E); byte.resize(E + M.E);
            u64 bad = BFQ_EDIT_NOPOS;
            const char *why = nullptr;
            const int rc = bfq_edits_decode_host(h_edits + at, M.bytes(), pos.data() + E, byte.data() + E, M.E, nullptr, &bad, &why);
            if (rc == BFQ_E_NOMEM) throw std::bad_alloc();
            if (rc != BFQ_OK) {
                if (bad != BFQ_EDIT_NOPOS) ed_refuse("edits member %llu: damaged BFQEDIT1 container: edit %llu is the first bad one", m, bad);
                ed_refuse((std::string("edits member %llu: ") + (why ? why : "damaged")).c_str(), m, 0);
            }
            if (M.N > N - r0 || roff[r0 + M.N] - roff[r0] != M.T)     // (r0 <= N; no sum that could wrap)
                ed_refuse("edits member %llu: edits of %llu reads for a text of %llu records, or another number of bases", m, M.N + r0, N);
            u64 shape = 0, tsum = 0;
            for (u64 r = 0; r < M.N; r++) shape += bfq_edit_shape_term(r, X.len[r0 + r]);
            if (shape != M.shape) ed_refuse("edits member %llu: the read lengths are not those of the collection these edits were made from (shape %llu against %llu)", m, M.shape, shape);
            u64 r = r0, lastRead = ~0ull;
            for (u64 k = 0; k < M.E; k++) {
                const u64 g = pos[E + k] + roff[r0];
                while (roff[r + 1] <= g) r++;
                if (r != lastRead) { touched++; lastRead = r; }
                tsum += bfq_edit_sum_term(pos[E + k], text[X.start[r] + (g - roff[r])]);
                pos[E + k] = X.start[r] + (g - roff[r]);          // where it lies in the text
            }
            if (tsum != M.targetSum) ed_refuse("edits member %llu: the text is not the output these edits were made from", m, 0);
            E += M.E; r0 += M.N; at += M.bytes(); m++;
        }
        if (r0 != N) ed_refuse("edits of %llu reads for a text of %llu records", r0, N);
        if (cap < len) ed_refuse("the output needs %llu bytes, the buffer has %llu", len, cap);
        if (len) memcpy(h_out, text, len);
        for (u64 k = 0; k < E; k++) h_out[pos[k]] = byte[k];
        *out_len = len;
        if (stats) { stats->reads = N; stats->bases = roff[N]; stats->edits = E; stats->reads_touched = touched; stats->bytes = edits_len; }
    });
}
