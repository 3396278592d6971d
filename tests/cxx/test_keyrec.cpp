// test_keyrec.cpp -- bfq_keyrec.h on the host: the sort record of a text position as k_build_keys and the sort's generating
// first pass build it, against a byte-wise restatement that uses none of the packed-word shortcuts.  Exact-size heap
// buffers: under -fsanitize=address,undefined a read beside the text ends the run.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_keyrec.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { if (g_fail < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static u64 g_rng = 1;
static u32 rnd(u32 m) { g_rng = bfq_mix64(g_rng); return (u32)(g_rng >> 33) % m; }

// the record of position p, symbol by symbol: the 16 symbols from p on (nothing after the first terminator), two symbols per
// 5-bit group (0 for a terminator first, else 6 c0 + c1 - 5), the number of symbols before the terminator, and the payload
static void oracle(const std::vector<u8> &T, const std::vector<u8> &Q, u64 p, u32 *w0, u32 *w1, u32 *w2)
{
    const u64 n = T.size();
    u32 sym[16];
    u32 L = 16;
    for (u32 i = 0; i < 16; i++) {
        const u32 c = (p + i < n) ? T[p + i] : 0u;
        if (L == 16 && c == 0) L = i;
        sym[i] = (L < 16) ? 0u : c;
    }
    u64 key40 = 0;
    for (u32 g = 0; g < 8; g++) {
        const u32 c0 = sym[2 * g], c1 = sym[2 * g + 1];
        key40 = (key40 << 5) | (u64)(c0 ? 6 * c0 + c1 - 5 : 0u);
    }
    const u32 pc = p ? T[p - 1] : 0u;
    const u32 pq = pc ? Q[p - 1] : (u32)'#';
    const u64 pay = p | ((u64)pc << 37) | ((u64)pq << 40);
    *w0 = (u32)(key40 >> 8);
    *w1 = ((u32)(key40 & 0xFFu) << 24) | (L << 16) | (u32)(pay >> 32);
    *w2 = (u32)(pay & 0xFFFFFFFFu);
}

// the packed text as k_pack3 lays it out: 21 symbols per word, 64-byte sectors of 6 words + the next sector's first two
static std::vector<u64> pack(const std::vector<u8> &T)
{
    const u64 n = T.size(), nwords = n / BFQ_SYMS_PER_WORD + 3, nl = bfq_t3_logical(nwords);
    std::vector<u64> t3(bfq_t3_alloc(nwords), 0);
    for (u64 w = 0; w < nl; w++) {
        u64 v = 0;
        for (u32 j = 0; j < BFQ_SYMS_PER_WORD; j++) { const u64 p = w * BFQ_SYMS_PER_WORD + j; v = (v << 3) | (p < n ? (u64)T[p] : 0ull); }
        t3[bfq_t3_at(w)] = v;
        const u64 j = w / BFQ_T3_PER_SEC, r = w - j * BFQ_T3_PER_SEC;
        if (r < 2 && j) t3[(j - 1) * 8 + 6 + r] = v;
    }
    return t3;
}

// a terminated text of n symbols: terminators with probability 1 / termEvery (side by side now and then), N's, the last symbol a terminator
static void make_text(u64 n, u32 termEvery, std::vector<u8> &T, std::vector<u8> &Q)
{
    T.assign(n, 0); Q.assign(n, 0);
    for (u64 i = 0; i < n; i++) {
        const u32 x = rnd(termEvery);
        u8 c = (u8)(1 + rnd(5));                                    // A C G N T
        if (x == 0) c = 0;
        else if (x == 1 && i && T[i - 1] == 0) c = 0;               // terminators side by side (empty reads)
        else if (rnd(7) == 0) c = 4;                                // more N's
        T[i] = c;
        Q[i] = (u8)(33 + rnd(60));
    }
    T[n - 1] = 0;
}

static void check_text(u64 n, u32 termEvery)
{
    std::vector<u8> T, Q;
    make_text(n, termEvery, T, Q);
    const std::vector<u64> t3 = pack(T);
    const u64 tile = 3072;
    for (u64 p = 0; p < n; p++) {
        u32 e0, e1, e2;
        oracle(T, Q, p, &e0, &e1, &e2);
        // from the arrays
        u32 w0 = 0; u64 w12 = 0;
        bfq_keyrec_at(T.data(), Q.data(), t3.data(), p, &w0, &w12);
        CHECK(w0 == e0 && (u32)w12 == e1 && (u32)(w12 >> 32) == e2);
        // from the words, indexed the way the generating pass does: relative to the first position of the scatter tile
        const u64 tbase = p / tile * tile, wb = tbase / BFQ_SYMS_PER_WORD, sb = wb / BFQ_T3_PER_SEC;
        const u32 ob = (u32)(tbase - wb * BFQ_SYMS_PER_WORD), rb = (u32)(wb - sb * BFQ_T3_PER_SEC), s = (u32)(p - tbase);
        const u32 dq = bfq_div21_small(ob + s), o = ob + s - dq * BFQ_SYMS_PER_WORD;
        CHECK(wb + dq == p / BFQ_SYMS_PER_WORD && o == p % BFQ_SYMS_PER_WORD);
        u64 wd[2];
        for (u32 k = 0; k < 2; k++) {
            const u32 e = rb + dq + k, es = bfq_div6_small(e);
            const u64 at = sb * 8 + es * 8 + (e - es * BFQ_T3_PER_SEC);
            CHECK(at < t3.size());
            wd[k] = at < t3.size() ? t3[at] : 0;
        }
        u32 v0 = 0; u64 v12 = 0;
        bfq_keyrec(wd[0], wd[1], o, p, p ? T[p - 1] : 0xAAu, p ? Q[p - 1] : 0xAAu, &v0, &v12);   // (position 0: the bytes are ignored)
        CHECK(v0 == e0 && v12 == w12);
        CHECK(bfq_keyrec_digit0(wd[0], wd[1], o) == (e1 >> 24));
        // the key is the one the 63-bit window arithmetic of bfq_common.h gives (what the refinement compares keys with)
        const u64 sk63 = bfq_skey_of(bfq_key_at(t3.data(), p));
        CHECK(bfq_keyrec_skey(wd[0], wd[1], o) == sk63 && bfq_rec_w0(sk63) == e0 && (bfq_rec_w1(sk63, 0) >> 16) == (e1 >> 16));
        // and back: key and payload as the later stages read them
        const u64 sk = bfq_rec_skey(w0, (u32)w12), pay = bfq_rec_pay((u32)w12, (u32)(w12 >> 32));
        CHECK(bfq_val_pos(pay) == p && bfq_val_code(pay) == (p ? T[p - 1] : 0u));
        CHECK(bfq_skey_has_term(sk) == (((e1 >> 16) & 31u) < 16u));
    }
}

int main()
{
    // the small divisions of the tile-relative index arithmetic, over all they are used for
    for (u32 q = 0; q < 4096; q++) CHECK(bfq_div21_small(q) == q / 21);
    for (u32 e = 0; e < 256; e++) CHECK(bfq_div6_small(e) == e / 6);

    // sizes around the word (21), the sector (6 words = 126) and the scatter tile (3072); every position of every text is
    // checked, so position 0, word offsets 0 and 20 and the last positions of the text are all among them
    const u64 sizes[] = {1, 2, 3, 5, 15, 16, 17, 20, 21, 22, 41, 42, 43, 125, 126, 127, 3071, 3072, 3073, 3072 + 21, 2 * 3072 - 1, 2 * 3072 + 1, 4 * 3072 + 1, 20011};
    const u32 dens[] = {2, 3, 16, 151};                             // reads of about 1, 2, 15 and 150 symbols
    for (u64 n : sizes)
        for (u32 d : dens) { g_rng = n * 1000 + d; check_text(n, d); }

    // hand-made: only terminators; one long run of one base; a terminator at word offset 20 and at 0
    {
        std::vector<u8> T(50, 0), Q(50, 'I');
        const std::vector<u64> t3 = pack(T);
        for (u64 p = 0; p < 50; p++) {
            u32 e0, e1, e2, w0; u64 w12;
            oracle(T, Q, p, &e0, &e1, &e2);
            bfq_keyrec_at(T.data(), Q.data(), t3.data(), p, &w0, &w12);
            CHECK(w0 == e0 && (u32)w12 == e1 && (u32)(w12 >> 32) == e2 && e0 == 0 && (e1 >> 16) == 0 && (u8)(w12 >> 8) == '#');
        }
    }
    {
        std::vector<u8> T(301, 3), Q(301, 'F');
        T[300] = 0; T[20] = 0; T[21] = 0; T[42] = 0;
        const std::vector<u64> t3 = pack(T);
        for (u64 p = 0; p < 301; p++) {
            u32 e0, e1, e2, w0; u64 w12;
            oracle(T, Q, p, &e0, &e1, &e2);
            bfq_keyrec_at(T.data(), Q.data(), t3.data(), p, &w0, &w12);
            CHECK(w0 == e0 && (u32)w12 == e1 && (u32)(w12 >> 32) == e2);
        }
    }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
    printf("ok\n");
    return 0;
}
