// test_posbin_wc.cpp -- the write-combining arithmetic of bfq_posbin.h on the host: a model of the scheme of k_posbin_l1_wc
// (carried tails, head claims in whole chunks, chunks named by one tile record each, tails to the bins' ends through the
// downward cursor) and of its second-level form in profiles/microbench/partition_wc.hip (contiguous tile ranges with the
// flush at a level-1 bin change), run over permutations of n positions.  Checked: every chunk written through the head
// cursor starts on a 64-byte boundary, every slot of every bin is written exactly once and with a record of that bin, and
// head + tail cursors equal every bin's capacity.  Exact-size heap buffers: under -fsanitize=address,undefined an index
// beside them ends the run.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_posbin.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { if (g_fail < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static const u64 NONE = ~0ull;

struct Wg {                                         // what a workgroup keeps from tile to tile
    std::vector<u64> left;                          // [bin * (C - 1) + t]
    std::vector<u32> nleft;
    u64 curBase = 0, next = 0, last = 0, step = 1;
};

struct Level {
    u64 n; int level, shiftIn, shiftOut; u32 C, tile, recBytes;
    u64 nbLocal;                                    // bins a tile can meet
    std::vector<u32> head, tail;                    // global cursors, one pair per output bin
    std::vector<u64> out;
    u64 chunks = 0, tailRecs = 0;

    void put(u64 g, u64 slot, u64 rec)
    {
        const u64 cap = bfq_posbin_cap(n, shiftOut, g);
        CHECK(slot < cap);
        if (slot >= cap) return;
        CHECK((rec >> shiftOut) == g);
        CHECK(out[(g << shiftOut) + slot] == NONE);
        out[(g << shiftOut) + slot] = rec;
    }
    void tails_out(Wg &w)
    {
        for (u64 b = 0; b < nbLocal; b++) {
            const u32 nl = w.nleft[b];
            if (!nl) continue;
            const u64 g = w.curBase + b, cap = bfq_posbin_cap(n, shiftOut, g);
            const u64 s = tail[g]; tail[g] += nl;
            for (u32 t = 0; t < nl; t++) {
                CHECK(s + t < cap);
                if (s + t < cap) put(g, bfq_posbin_tail_slot(cap, s + t), w.left[b * (C - 1) + t]);
            }
            tailRecs += nl;
            w.nleft[b] = 0;
        }
    }
    void one_tile(Wg &w, const std::vector<u64> &in, u64 tileIdx)
    {
        const u64 tbase = tileIdx * tile;
        const u64 binBase = level == 1 ? 0 : (tbase >> shiftIn) << (shiftIn - shiftOut);
        if (level == 2 && binBase != w.curBase) tails_out(w);
        w.curBase = binBase;
        const u64 cnt = tbase + tile <= n ? tile : n - tbase;
        std::vector<u32> lcnt(nbLocal, 0), lb(cnt), rk(cnt), lstart(nbLocal), cstart(nbLocal), nfl(nbLocal), gb(nbLocal, 0);
        for (u64 i = 0; i < cnt; i++) {
            const u64 l = (in[tbase + i] >> shiftOut) - binBase;
            CHECK(l < nbLocal);
            lb[i] = (u32)l; rk[i] = lcnt[l]++;
        }
        u32 recs = 0, nch = 0;
        for (u64 b = 0; b < nbLocal; b++) {
            const u32 h = bfq_posbin_head_claim(w.nleft[b], lcnt[b], C);
            CHECK(h % C == 0 && h <= w.nleft[b] + lcnt[b] && w.nleft[b] + lcnt[b] - h < C);
            CHECK(h + bfq_posbin_tail_kept(w.nleft[b], lcnt[b], C) == w.nleft[b] + lcnt[b]);
            lstart[b] = recs; cstart[b] = nch; nfl[b] = h / C;
            recs += lcnt[b]; nch += nfl[b];
            if (h) { gb[b] = head[binBase + b]; head[binBase + b] += h; }
        }
        CHECK(nch <= (tile + nbLocal * (C - 1)) / C);
        std::vector<u64> stage(cnt, NONE);
        std::vector<u32> cbin(nch, 0xFFFFFFFFu);
        for (u64 i = 0; i < cnt; i++) {
            const u32 l = lb[i];
            stage[lstart[l] + rk[i]] = in[tbase + i];
            const u32 ci = w.nleft[l] + rk[i], ch = ci / C;
            if (ch < nfl[l] && (ci % C == 0 || rk[i] == 0)) { CHECK(cbin[cstart[l] + ch] == 0xFFFFFFFFu); cbin[cstart[l] + ch] = l; }
        }
        for (u32 e = 0; e < nch * C; e++) {
            const u32 ch = e / C, l = cbin[ch];
            CHECK(l < nbLocal);
            if (l >= nbLocal) continue;
            const u32 nl = w.nleft[l], ci = (ch - cstart[l]) * C + e % C;
            const u64 rec = ci < nl ? w.left[l * (C - 1) + ci] : stage[lstart[l] + ci - nl];
            const u64 g = binBase + l, off = (u64)gb[l] + ci;
            if (e % C == 0) { CHECK((((g << shiftOut) + off) * recBytes) % BFQ_PB_CHUNK_BYTES == 0); chunks++; }
            put(g, off, rec);
        }
        for (u64 b = 0; b < nbLocal; b++) {
            const u32 n0 = w.nleft[b], h = nfl[b] * C, r = bfq_posbin_tail_kept(n0, lcnt[b], C);
            const u32 s0 = lstart[b] + h - n0;      // (wraps below zero where the bin flushed nothing: only t >= n0 is taken then)
            for (u32 t = h ? 0u : n0; t < r; t++) w.left[b * (C - 1) + t] = stage[(u32)(s0 + t)];
            w.nleft[b] = r;
        }
    }
};

// one level over `in` (n records whose value is their position), G workgroups taking turns tile by tile; returns the output
static std::vector<u64> run_level(const std::vector<u64> &in, u64 n, int level, int shiftIn, int shiftOut, u32 tile, u32 G, u64 *tailRecs)
{
    Level L;
    L.n = n; L.level = level; L.shiftIn = shiftIn; L.shiftOut = shiftOut; L.C = bfq_posbin_chunk(level); L.tile = tile;
    L.recBytes = level == 1 ? 8 : 4;
    CHECK(L.C * L.recBytes == BFQ_PB_CHUNK_BYTES);
    const u64 nbOut = bfq_posbin_bins(n, shiftOut);
    L.nbLocal = level == 1 ? nbOut : (1ull << (shiftIn - shiftOut));
    L.head.assign(nbOut + L.nbLocal, 0); L.tail.assign(nbOut + L.nbLocal, 0);
    L.out.assign(n, NONE);
    const u64 ntiles = (n + tile - 1) / tile;
    if (G > ntiles) G = (u32)ntiles;
    std::vector<Wg> wg(G);
    const u64 per = G ? (ntiles + G - 1) / G : 0;
    for (u32 g = 0; g < G; g++) {
        wg[g].left.assign(L.nbLocal * (L.C - 1), NONE); wg[g].nleft.assign(L.nbLocal, 0);
        if (level == 1) { wg[g].next = g; wg[g].last = ntiles; wg[g].step = G; }
        else { wg[g].next = g * per; wg[g].last = (g + 1) * per < ntiles ? (g + 1) * per : ntiles; wg[g].step = 1; }
    }
    for (bool any = true; any;) {
        any = false;
        for (u32 g = 0; g < G; g++)
            if (wg[g].next < wg[g].last) { L.one_tile(wg[g], in, wg[g].next); wg[g].next += wg[g].step; any = true; }
    }
    for (u32 g = 0; g < G; g++) L.tails_out(wg[g]);
    for (u64 b = 0; b < nbOut; b++) CHECK((u64)L.head[b] + L.tail[b] == bfq_posbin_cap(n, shiftOut, b));
    for (u64 i = 0; i < n; i++) if (L.out[i] == NONE) { CHECK(!"a slot was never written"); break; }
    if (tailRecs) *tailRecs = L.tailRecs;
    return L.out;
}

// both levels on a permutation of [0, n): kind 0 = scattered, 1 = in position order (a tile falls into one bin and one window)
static void run_both(u64 n, int s1, int s2, u32 tile, u32 G, int kind)
{
    std::vector<u64> in(n);
    const u64 P = 2147483647ull;                   // prime: i -> i * P mod n is a bijection for every n below it
    for (u64 i = 0; i < n; i++) in[i] = kind == 0 ? (i * P + 12345) % n : i;
    const std::vector<u64> l1 = run_level(in, n, 1, 0, s1, tile, G, nullptr);
    const std::vector<u64> l2 = run_level(l1, n, 2, s1, s2, tile, G, nullptr);
    for (u64 i = 0; i < n; i++) if ((l2[i] >> s2) != (i >> s2)) { CHECK(!"a record outside its window"); break; }
}

int main()
{
    CHECK(bfq_posbin_chunk(1) == 8 && bfq_posbin_chunk(2) == 16);
    CHECK(bfq_posbin_head_claim(7, 0, 8) == 0 && bfq_posbin_head_claim(7, 1, 8) == 8 && bfq_posbin_head_claim(0, 4096, 16) == 4096);
    CHECK(bfq_posbin_tail_kept(15, 4096, 16) == 15 && bfq_posbin_tail_slot(5, 0) == 4 && bfq_posbin_tail_slot(5, 4) == 0);
    // small bins, small tiles, every n: 2^8-position bins of 2^4-position windows, tiles of 64 records, 1 / 3 / 7 workgroups
    for (u64 n = 0; n <= 3000; n++)
        for (int kind = 0; kind < 2; kind++) run_both(n, 8, 4, 64, n % 3 == 0 ? 1 : (n % 3 == 1 ? 3 : 7), kind);
    // level-1 bins of 512 windows, as at the largest sizes: a workgroup's range crosses bins of 2^13 positions
    for (u64 n : {8191ull, 8192ull, 8193ull, 20000ull, 40961ull}) run_both(n, 13, 4, 128, 5, 0);
    // the library's geometry and tile around one window (= one level-1 bin at these sizes) ...
    const u64 W = BFQ_PB_W;
    for (u64 n : {W - 1, W, W + 1, W + 7, W + 15, 2 * W + 1, 3 * W + 9})
        for (int kind = 0; kind < 2; kind++) { CHECK(bfq_posbin_shift(n) == BFQ_PB_WSHIFT); run_both(n, BFQ_PB_WSHIFT, BFQ_PB_WSHIFT, 4096, 4, kind); }
    // ... and just above 512 windows, around the end of a level-1 bin of two windows
    {
        const u64 n0 = 512 * W + 1;
        const int s1 = bfq_posbin_shift(n0);
        CHECK(s1 == BFQ_PB_WSHIFT + 1);
        for (u64 n : {n0, (n0 | ((1ull << s1) - 1)) + 1 + 15}) {
            CHECK(bfq_posbin_shift(n) == s1);
            run_both(n, s1, BFQ_PB_WSHIFT, 4096, 512, 0);
        }
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
