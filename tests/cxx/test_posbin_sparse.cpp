// test_posbin_sparse.cpp -- the sparse form's arithmetic of bfq_posbin.h on the host: which slots of a partially filled bin
// are live, which tiles lie in its gap, the polarity rule and the default quality, and the terminator bitmap of a window
// against bfq_posbin_reads_before.  Exact-size heap buffers: under -fsanitize=address,undefined a read beside them ends
// the run.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_posbin.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

// the predicate against its definition: slot idx is live iff it lies in [0, head) or [cap - tail, cap)
static void check_regions(u64 cap, u64 head, u64 tail)
{
    u64 live = 0;
    for (u64 i = 0; i < cap + 3; i++) {
        const bool want = i < cap && (i < head || (tail <= cap ? i >= cap - tail : true));
        CHECK(bfq_posbin_live(cap, head, tail, i) == want);
        live += want;
    }
    if (head + tail <= cap) CHECK(live == head + tail);
    // a tile is skipped iff none of its slots is live
    for (u64 len : {1ull, 8ull, 64ull})
        for (u64 t0 = 0; t0 < cap + 2 * len; t0 += len) {
            bool any = false;
            for (u64 i = t0; i < t0 + len; i++) any = any || bfq_posbin_live(cap, head, tail, i);
            CHECK(bfq_posbin_gap_tile(cap, head, tail, t0, len) == !any);
        }
}

int main()
{
    const u32 C = bfq_posbin_chunk(1);
    // head = 0, tail = 0, head + tail = cap, cap below a chunk, and a bin that received more than it holds (an error the
    // check kernel counts: the predicate must still stay inside the bin)
    for (u64 cap : {1ull, 3ull, (u64)C - 1, (u64)C, 2ull * C + 3, 200ull})
        for (u64 head = 0; head <= cap + C; head += C)
            for (u64 tail : {0ull, 1ull, (u64)C - 1, cap > head ? cap - head : 0ull, cap, cap + 1}) check_regions(cap, head, tail);
    check_regions(0, 0, 0);
    CHECK(!bfq_posbin_live(5, 0, 0, 0) && bfq_posbin_gap_tile(5, 0, 0, 0, 4096));           // nothing sent: every tile is skipped
    CHECK(bfq_posbin_live(5, 0, 5, 0) && bfq_posbin_live(5, 0, 5, 4) && !bfq_posbin_live(5, 0, 5, 5));   // cap < chunk: all in the tail
    CHECK(bfq_posbin_live(16, 8, 8, 7) && bfq_posbin_live(16, 8, 8, 8));                     // head + tail = cap: no gap

    // polarity: const only for M = 2 and more than half of the bases smoothed, unless forced
    CHECK(bfq_posbin_polarity(2, -1, 51, 100) == BFQ_PB_CONST && bfq_posbin_polarity(2, -1, 50, 100) == BFQ_PB_KEEP);
    CHECK(bfq_posbin_polarity(1, -1, 100, 100) == BFQ_PB_KEEP && bfq_posbin_polarity(3, -1, 100, 100) == BFQ_PB_KEEP);
    CHECK(bfq_posbin_polarity(2, -1, 0, 0) == BFQ_PB_KEEP);
    CHECK(bfq_posbin_polarity(2, BFQ_PB_KEEP, 100, 100) == BFQ_PB_KEEP && bfq_posbin_polarity(2, BFQ_PB_CONST, 0, 100) == BFQ_PB_CONST);
    for (u32 q = 0; q < 256; q++) {
        CHECK(bfq_posbin_default_qual(BFQ_PB_KEEP, 0, q, '>') == q && bfq_posbin_default_qual(BFQ_PB_KEEP, 1, q, '>') == bfq_bin8(q));
        CHECK(bfq_posbin_default_qual(BFQ_PB_CONST, 0, q, '>') == (u32)'>' && bfq_posbin_default_qual(BFQ_PB_CONST, 1, q, '>') == bfq_bin8('>'));
    }

    // the terminator bitmap of a window, built from the read offsets the way the last kernel builds it, against the search:
    // window position idx of window q0 goes to packed slot (q0 + idx) - reads_before(q0 + idx) = o0 + idx - rank(idx)
    unsigned seed = 4242;
    auto rnd = [&](unsigned m) { seed = seed * 1103515245u + 12345u; return (seed >> 16) % m; };
    for (int round = 0; round < 40; round++) {
        const u64 W = 256;                                                // (the arithmetic does not know the window's size)
        const u64 N = round == 0 ? 1 : 1 + rnd(60);
        std::vector<u64> roff(N + 1, 0);
        for (u64 i = 0; i < N; i++) {
            const unsigned kind = round == 1 ? 0 : rnd(6);
            roff[i + 1] = roff[i] + (kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? 17 : kind == 3 ? W - 1 : 1 + rnd(300));   // empty reads, reads across windows
        }
        const u64 n = roff[N] + N;
        for (u64 q0 = 0; q0 < n; q0 += W) {
            const u64 cap = n - q0 < W ? n - q0 : W;
            std::vector<u64> bm(W / 64, 0);
            std::vector<u32> pre(W / 64, 0);
            const u64 rb = bfq_posbin_reads_before(roff.data(), N, q0);
            for (u64 i = rb; i < N; i++) {
                const u64 t = roff[i + 1] + i;
                CHECK(t >= q0);
                if (t >= q0 + cap) break;
                bm[(t - q0) >> 6] |= 1ull << ((t - q0) & 63);
            }
            u32 terms = 0;
            for (u64 w = 0; w < W / 64; w++) { pre[w] = terms; terms += (u32)bfq_popc64(bm[w]); }
            const u64 o0 = q0 - rb;
            for (u32 idx = 0; idx < cap; idx++) {
                const u64 before = bfq_posbin_reads_before(roff.data(), N, q0 + idx);
                const bool term = before < N && roff[before + 1] + before == q0 + idx;
                CHECK(bfq_posbin_is_term(bm.data(), idx) == term);
                CHECK(bfq_posbin_term_rank(bm.data(), pre.data(), idx) == before - rb);
                if (!term) CHECK(o0 + idx - bfq_posbin_term_rank(bm.data(), pre.data(), idx) == q0 + idx - before);
            }
            // the window's packed range ends where the next one begins
            const u64 next = q0 + cap;
            CHECK(o0 + (cap - terms) == next - (next < n ? bfq_posbin_reads_before(roff.data(), N, next) : N));
        }
    }

    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("posbin sparse: all checks passed\n");
    return 0;
}
