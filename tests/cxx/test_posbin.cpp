// test_posbin.cpp -- bfq_posbin.h on the host: the bin arithmetic of the position-bin inversion and the search that tells
// which read a text position lies in.  Exact-size heap buffers: under -fsanitize=address,undefined a read beside the
// offsets ends the run.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_posbin.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

int main()
{
    // shift: the smallest one that gives at most BFQ_PB_MAX_BINS bins, never below the window; bins of exact capacity
    const u64 W = BFQ_PB_W;
    const u64 sizes[] = {0, 1, 2, W - 1, W, W + 1, 2 * W + 1, 512 * W - 1, 512 * W, 512 * W + 1, 1024 * W, 1024 * W + 1, 4530000000ull,
                         (1ull << 33) - 1, 1ull << 33};
    for (u64 n : sizes) {
        const int s = bfq_posbin_shift(n);
        CHECK(s >= BFQ_PB_WSHIFT && s <= BFQ_PB_MAX_SHIFT);
        const u64 nb = bfq_posbin_bins(n, s);
        CHECK(nb <= BFQ_PB_MAX_BINS);
        CHECK(n == 0 || s == BFQ_PB_WSHIFT || bfq_posbin_bins(n, s - 1) > BFQ_PB_MAX_BINS);
        CHECK((1ull << (s - BFQ_PB_WSHIFT)) <= BFQ_PB_MAX_BINS);              // windows per first-level bin
        u64 sum = 0;
        for (u64 b = 0; b < nb; b++) {
            const u64 cap = bfq_posbin_cap(n, s, b);
            CHECK(cap >= 1 && cap <= (1ull << s) && (b + 1 == nb || cap == (1ull << s)));
            sum += cap;
        }
        CHECK(sum == n);
        CHECK(bfq_posbin_cap(n, s, nb) == 0 && bfq_posbin_cap(n, s, nb + 5) == 0);
        if (n) { CHECK(((n - 1) >> s) == nb - 1); }
        // the windows tile the bins
        const u64 nw = bfq_posbin_bins(n, BFQ_PB_WSHIFT);
        CHECK(nw == (n + W - 1) / W);
        if (n && n <= 1024 * W + 1) {
            u64 s2 = 0;
            for (u64 w = 0; w < nw; w++) s2 += bfq_posbin_cap(n, BFQ_PB_WSHIFT, w);
            CHECK(s2 == n);
        }
    }
    CHECK(bfq_posbin_shift((1ull << 33) + 1) == -1 && bfq_posbin_shift(1ull << 36) == -1);
    CHECK(bfq_posbin_shift(4530000000ull) == 24);

    // the 4-byte record keeps position-in-window, code and quality
    for (u64 pos : {0ull, 1ull, W - 1, W, 5 * W + 77, (1ull << 33) - 1})
        for (u32 code = 0; code < 6; code++)
            for (u32 q : {0u, 33u, 74u, 255u}) {
                const u32 r = bfq_posbin_rec4(bfq_pack_val(pos, code, q));
                CHECK((r & (BFQ_PB_W - 1u)) == (u32)(pos % W) && ((r >> BFQ_PB_WSHIFT) & 7u) == code && ((r >> (BFQ_PB_WSHIFT + 3)) & 0xFFu) == q);
                CHECK((r >> (BFQ_PB_WSHIFT + 11)) == 0);
            }

    // reads before a position: against a walk over the text, variable lengths with empty reads, every position
    unsigned seed = 12345;
    auto rnd = [&](unsigned m) { seed = seed * 1103515245u + 12345u; return (seed >> 16) % m; };
    for (int round = 0; round < 60; round++) {
        const u64 N = round == 0 ? 0 : round == 1 ? 1 : 1 + rnd(40);
        std::vector<u64> len(N);
        for (u64 i = 0; i < N; i++) len[i] = round == 1 ? 1 : round % 5 == 2 ? rnd(3) : rnd(2) ? rnd(20) : 300 * rnd(2) + rnd(17);
        u64 *roff = (u64 *)malloc(8 * (N + 1));                               // exactly N + 1 entries
        roff[0] = 0;
        for (u64 i = 0; i < N; i++) roff[i + 1] = roff[i] + len[i];
        const u64 n = roff[N] + N;
        u64 q = 0;
        for (u64 i = 0; i < N; i++) {
            for (u64 k = 0; k <= len[i]; k++, q++) {                          // the read's bases, then its terminator
                CHECK(bfq_posbin_reads_before(roff, N, q) == i);
                if (k < len[i]) CHECK(q - bfq_posbin_reads_before(roff, N, q) == roff[i] + k);
            }
        }
        CHECK(q == n);
        CHECK(bfq_posbin_reads_before(roff, N, n) == N && bfq_posbin_reads_before(roff, N, n + 1000) == N);
        free(roff);
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("test_posbin: ok\n");
    return 0;
}
