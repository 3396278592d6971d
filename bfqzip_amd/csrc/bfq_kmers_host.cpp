// bfq_kmers_host.cpp -- bfq_fastq_kmers_host (include/bfqzip_hip.h): the k-mer spectrum report on one thread of the host.
// It states the algorithm -- every valid window's k-mer with its source bit in one array, sorted, the runs counted -- and is
// what the tests hold the device path to; no entry point falls back to it.  Plain text only; no context, no GPU.
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "bfq_internal_host.h"
#include "bfq_kmers.h"

static thread_local std::string g_kmersHostErr;
extern "C" const char *bfq_kmers_host_error(void) { return g_kmersHostErr.c_str(); }

extern "C" int bfq_kmers_geometry(uint64_t *seg_chunk_rows, uint64_t *run_chunk_runs, uint64_t *lane_starts)
{
    if (seg_chunk_rows) *seg_chunk_rows = KM_SEG_CHUNK;
    if (run_chunk_runs) *run_chunk_runs = KM_RUN_CHUNK;
    if (lane_starts) *lane_starts = KM_STARTS;
    return BFQ_OK;
}

namespace {
struct Side { u64 reads = 0, shortReads = 0, windows = 0, skipped = 0; };

// the sequence lines of a text: a text that lacks its final newline is read as if it had one
void km_host_text(const u8 *t, u64 len, const char *which, const bfq_kmer_opts &O, u32 src, std::vector<u64> &keys, Side &S)
{
    auto refuse = [&](int code, const char *m) { throw BfqError{code, std::string(which) + ": " + m}; };
    std::vector<u64> ends;                                        // one past each line's last byte (its LF, or the end of the text)
    for (u64 i = 0; i < len; i++)
        if (t[i] == 10) ends.push_back(i);
    if (len && t[len - 1] != 10) ends.push_back(len);
    if (ends.size() % 4) refuse(BFQ_E_ARG, "FASTQ: number of lines is not a multiple of 4");
    const u64 N = ends.size() / 4;
    auto line = [&](u64 li, u64 *s, u64 *e) {
        *s = li ? ends[li - 1] + 1 : 0;
        *e = ends[li];
        if (*e > *s && t[*e - 1] == 13) --*e;
    };
    bool tooLong = false;
    for (u64 i = 0; i < N; i++) {
        u64 s, e, qs, qe;
        line(4 * i + 1, &s, &e);
        line(4 * i + 3, &qs, &qe);
        if (qe - qs != e - s) refuse(BFQ_E_ARG, "FASTQ: len(DNA) != len(QS) in a record");
        tooLong |= e - s > BFQ_MAX_READ_LEN;
    }
    if (tooLong) refuse(BFQ_E_TOO_LONG, "read longer than BFQ_MAX_READ_LEN");
    const u32 k = O.k;
    const u64 mask = (1ull << (2 * k)) - 1;
    S.reads = N;
    for (u64 i = 0; i < N; i++) {
        u64 s, e;
        line(4 * i + 1, &s, &e);
        const u64 L = e - s;
        if (L < k) { S.shortReads++; continue; }
        u64 fwd = 0, rc = 0;
        u32 run = 0;                                              // valid bases that end at this one
        for (u64 p = 0; p < L; p++) {
            const u8 b = t[s + p];
            const u32 code = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
            if (code > 3) run = 0;
            else {
                fwd = ((fwd << 2) | code) & mask;                 // one shift-in: the next window from the one before
                rc = (rc >> 2) | ((u64)(3 - code) << (2 * (k - 1)));
                run++;
            }
            if (p + 1 < k) continue;
            if (run < k) { S.skipped++; continue; }
            S.windows++;
            const u64 x = O.canonical && rc < fwd ? rc : fwd;
            keys.push_back(x << 1 | src);
        }
    }
}
}   // namespace

extern "C" int bfq_fastq_kmers_host(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, const bfq_kmer_opts *opts,
                                    bfq_kmer_report *rep, bfq_kmer_entry *h_list, uint64_t cap_list)
{
    if (rep) memset(rep, 0, sizeof *rep);
    return host_guarded(g_kmersHostErr, [&] {
        if (!rep || (!a && a_len) || (!b && b_len)) throw BfqError{BFQ_E_ARG, "null argument"};
        if (cap_list && !h_list) throw BfqError{BFQ_E_ARG, "bfq_fastq_kmers: cap_list without a buffer"};
        bfq_kmer_opts O;
        if (const char *why = bfq_kmer_resolve(opts, &O)) throw BfqError{BFQ_E_ARG, why};
        std::vector<u64> keys;
        std::vector<bfq_kmer_entry> list;
        Side A, B;
        km_host_text(a, a_len, "A", O, 0, keys, A);
        if (b) km_host_text(b, b_len, "B", O, 1, keys, B);
        std::sort(keys.begin(), keys.end());
        bfq_kmer_report R;
        memset(&R, 0, sizeof R);
        R.k = O.k; R.solid = O.solid; R.canonical = O.canonical;
        R.n_reads_a = A.reads; R.reads_short_a = A.shortReads; R.windows_a = A.windows; R.windows_skipped_a = A.skipped;
        R.n_reads_b = B.reads; R.reads_short_b = B.shortReads; R.windows_b = B.windows; R.windows_skipped_b = B.skipped;
        u64 hist[KM_BINS] = {0};
        for (u64 i = 0; i < keys.size();) {
            u64 j = i, cb = 0;
            for (; j < keys.size() && keys[j] >> 1 == keys[i] >> 1; j++) cb += keys[j] & 1;
            const u64 ca = j - i - cb, x = keys[i] >> 1;
            hist[x >> (2 * O.k - KM_TOP_BITS)] += j - i;
            if (ca) { R.distinct_a++; R.hist_a[std::min<u64>(ca, 255)]++; }
            if (cb) { R.distinct_b++; R.hist_b[std::min<u64>(cb, 255)]++; }
            R.joint[16 * std::min<u64>(ca, 15) + std::min<u64>(cb, 15)]++;
            R.trans[3 * bfq_kmer_class(ca, O.solid) + bfq_kmer_class(cb, O.solid)]++;
            if (ca && cb) R.distinct_both++;
            if (!cb) { R.only_a++; R.occ_only_a += ca; }
            if (!ca) { R.only_b++; R.occ_only_b += cb; }
            if (ca != cb) R.distinct_changed++;
            if (bfq_kmer_listed(ca, cb, O.solid)) {
                if (R.n_listed < cap_list) list.push_back(bfq_kmer_entry{x, (u32)std::min<u64>(ca, 0xFFFFFFFFu), (u32)std::min<u64>(cb, 0xFFFFFFFFu)});
                R.n_listed++;
            }
            i = j;
        }
        R.n_partitions = bfq_kmer_ranges(hist, O.part_records ? O.part_records : ~0ull).size();
        if (!list.empty()) memcpy(h_list, list.data(), sizeof(bfq_kmer_entry) * list.size());
        *rep = R;
    });
}
