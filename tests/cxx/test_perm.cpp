// test_perm.cpp -- bfq_perm.h on the host: the BFQPERM1 container (include/bfqzip_hip.h) encoded and decoded over the small
// read counts at which the entry width changes and entries start to straddle words, a bit-by-bit restatement of the layout,
// and every refusal with its first offending position.  Buffers are heap blocks of the exact size, so that a sanitizer sees
// any byte read or written beside them.  Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_perm.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state = bfq_mix64(rng_state); return rng_state; }

// bit b of the stream = bit b % 64 of word b / 64; entry j in bits [j w, (j + 1) w)
static u64 entry_bitwise(const u8 *z, u64 j, u32 w)
{
    u64 v = 0;
    for (u32 t = 0; t < w; t++) {
        const u64 b = j * w + t;
        u64 word;
        memcpy(&word, z + BFQ_PERM_HDR + 8 * (b / 64), 8);
        v |= ((word >> (b % 64)) & 1) << t;
    }
    return v;
}

static u32 width_slow(u64 N) { u32 w = 0; if (N > 2) for (u64 x = N - 1; x; x >>= 1) w++; return w ? w : 1; }

// decode must refuse z with first_bad = want and leave its outputs alone
static void refused(const std::vector<u8> &z, u64 want, const char *what)
{
    const u64 n = z.size() >= 16 ? bfq_perm_ld64(z.data() + 8) : 0;
    const u64 room = n < (1u << 20) ? n + 1 : 1;
    u64 *out = (u64 *)malloc(8 * room);
    for (u64 i = 0; i < room; i++) out[i] = 0xA5A5A5A5A5A5A5A5ull;
    u8 *copy = (u8 *)malloc(z.size() ? z.size() : 1);
    if (z.size()) memcpy(copy, z.data(), z.size());
    u64 N = 77, bad = 5;
    bfq_reorder_opts o;
    memset(&o, 0x5A, sizeof o);
    const int rc = bfq_perm_decode_host(copy, z.size(), out, room, &N, &o, &bad);
    if (rc != BFQ_E_ARG || bad != want || N != 77 || o.mode != 0x5A5A5A5A) { printf("FAIL refusal '%s': rc %d first_bad %llu (want %llu)\n", what, rc, bad, want); g_fail++; }
    for (u64 i = 0; i < room; i++) CHECK(out[i] == 0xA5A5A5A5A5A5A5A5ull);
    CHECK(bfq_perm_decode_host(copy, z.size(), out, room, nullptr, nullptr, nullptr) == BFQ_E_ARG);   // the optional outputs
    free(copy);
    free(out);
}

static void roundtrip(u64 N, int kind)
{
    std::vector<u64> p(N);
    for (u64 i = 0; i < N; i++) p[i] = kind == 1 ? N - 1 - i : i;                   // 0 identity, 1 reversal, 2 random
    if (kind == 2) for (u64 i = N; i > 1; i--) { const u64 j = rnd() % i; const u64 t = p[i - 1]; p[i - 1] = p[j]; p[j] = t; }
    const u32 w = bfq_perm_width(N);
    CHECK(w == width_slow(N));
    const u64 len = bfq_perm_bound_of(N);
    CHECK(len == 40 + 8 * ((N * w + 63) / 64));
    bfq_reorder_opts o;
    memset(&o, 0, sizeof o);
    o.mode = 2; o.k = 21; o.seed = 0x0123456789ABCDEFull + N;
    u64 *src = (u64 *)malloc(N ? 8 * N : 1);
    if (N) memcpy(src, p.data(), 8 * N);
    u8 *z = (u8 *)malloc(len);
    memset(z, 0xEE, len);
    u64 got = 0, bad = 1;
    CHECK(bfq_perm_encode_host(src, N, &o, z, len, &got, &bad) == BFQ_OK && got == len && bad == BFQ_PERM_NOPOS);
    CHECK(!memcmp(z, "BFQPERM1", 8) && bfq_perm_ld64(z + 8) == N && bfq_perm_ld32(z + 16) == w && bfq_perm_ld32(z + 20) == 2 &&
          bfq_perm_ld32(z + 24) == 21 && bfq_perm_ld32(z + 28) == 0 && bfq_perm_ld64(z + 32) == o.seed);
    for (u64 j = 0; j < N; j++) CHECK(entry_bitwise(z, j, w) == p[j]);
    for (u64 b = N * w; b < 8 * (len - 40); b++) {                                  // padding
        u64 word;
        memcpy(&word, z + 40 + 8 * (b / 64), 8);
        CHECK(!((word >> (b % 64)) & 1));
    }
    u64 n2 = 0;
    u32 w2 = 0;
    CHECK(bfq_perm_header(z, len, &n2, &w2, nullptr) && n2 == N && w2 == w);
    u64 *back = (u64 *)malloc(N ? 8 * N : 1);
    bfq_reorder_opts o2;
    u64 N2 = ~0ull;
    CHECK(bfq_perm_decode_host(z, len, back, N, &N2, &o2, &bad) == BFQ_OK && N2 == N && bad == BFQ_PERM_NOPOS);
    CHECK(o2.mode == 2 && o2.k == 21 && o2.seed == o.seed);
    for (u64 j = 0; j < N; j++) CHECK(back[j] == p[j]);
    // the device's accessors on the same payload (8-byte aligned: malloc + 40)
    const u64 *words = (const u64 *)(z + 40);
    for (u64 j = 0; j < N; j++) CHECK(bfq_perm_get(words, j, w) == p[j]);
    for (u64 q = 0; q < (len - 40) / 8; q++) CHECK(bfq_perm_word(src, N, w, q) == words[q]);
    // capacity: one byte short is refused, nothing written
    if (kind == 0) {
        u8 *small = (u8 *)malloc(len - 1);
        memset(small, 0xEE, len - 1);
        got = 9;
        CHECK(bfq_perm_encode_host(src, N, &o, small, len - 1, &got, &bad) == BFQ_E_ARG && got == 9 && bad == BFQ_PERM_NOPOS);
        for (u64 i = 0; i < len - 1; i++) CHECK(small[i] == 0xEE);
        free(small);
        if (N) CHECK(bfq_perm_decode_host(z, len, back, N - 1, &N2, nullptr, &bad) == BFQ_E_ARG && bad == BFQ_PERM_NOPOS);
    }
    free(back); free(z); free(src);
}

static std::vector<u8> container(const std::vector<u64> &p)
{
    std::vector<u8> z(bfq_perm_bound_of(p.size()));
    CHECK(bfq_perm_encode_host(p.data(), p.size(), nullptr, z.data(), z.size(), nullptr, nullptr) == BFQ_OK);
    return z;
}
// the payload with entry j overwritten (encode would refuse it)
static void poke(std::vector<u8> &z, u64 j, u64 v)
{
    const u32 w = bfq_perm_ld32(z.data() + 16);
    for (u32 t = 0; t < w; t++) {
        const u64 b = j * w + t;
        u8 &byte = z[40 + b / 8];
        byte = (u8)((byte & ~(1u << (b % 8))) | (((v >> t) & 1) << (b % 8)));
    }
}

int main()
{
    const u64 sizes[] = {0, 1, 2, 3, 4, 5, 64, 65, 127, 128, 129, 1000, 4097, 65536, 65537};
    for (u64 N : sizes)
        for (int kind = 0; kind < 3; kind++) roundtrip(N, kind);

    // ---- refusals
    std::vector<u64> p(37);
    for (u64 i = 0; i < p.size(); i++) p[i] = (i * 7 + 3) % 37;                     // w = 6: 222 bits, 34 padding bits
    const std::vector<u8> good = container(p);
    { u64 n = 0; CHECK(bfq_perm_header(good.data(), good.size(), &n, nullptr, nullptr) && n == 37); }
    { std::vector<u8> z = good; z[7] = '2'; refused(z, BFQ_PERM_NOPOS, "magic"); }
    { std::vector<u8> z = good; z[16] = 7; refused(z, BFQ_PERM_NOPOS, "w + 1"); }
    { std::vector<u8> z = good; z[16] = 5; refused(z, BFQ_PERM_NOPOS, "w - 1"); }
    { std::vector<u8> z = good; z.resize(z.size() + 8, 0); refused(z, BFQ_PERM_NOPOS, "length + 8"); }
    { std::vector<u8> z = good; z.resize(z.size() - 8); refused(z, BFQ_PERM_NOPOS, "length - 8"); }
    { std::vector<u8> z = good; z.resize(39); refused(z, BFQ_PERM_NOPOS, "shorter than the header"); }
    { std::vector<u8> z; refused(z, BFQ_PERM_NOPOS, "empty"); }
    { std::vector<u8> z = good; z[z.size() - 1] |= 0x80; refused(z, BFQ_PERM_NOPOS, "last padding bit"); }
    { std::vector<u8> z = good; z[40 + 222 / 8] |= (u8)(1u << (222 % 8)); refused(z, BFQ_PERM_NOPOS, "first padding bit"); }
    { std::vector<u8> z = good; memset(z.data() + 8, 0xFF, 8); refused(z, BFQ_PERM_NOPOS, "N >= 2^56"); }
    { std::vector<u8> z = good; poke(z, 20, 37); refused(z, 20, "entry == N"); }
    { std::vector<u8> z = good; poke(z, 36, 63); refused(z, 36, "last entry out of range"); }
    { std::vector<u8> z = good; poke(z, 30, p[4]); refused(z, 30, "a value twice"); }
    { std::vector<u8> z = good; poke(z, 4, p[30]); refused(z, 30, "a value twice: the later position"); }
    { std::vector<u8> z = good; poke(z, 9, 40); poke(z, 3, p[2]); refused(z, 3, "two faults: the first"); }
    // encode: not a permutation
    {
        u8 out[64];
        memset(out, 0xEE, sizeof out);
        u64 bad = 0, len = 3;
        std::vector<u64> q = {0, 1, 5, 3, 4};
        CHECK(bfq_perm_encode_host(q.data(), 5, nullptr, out, sizeof out, &len, &bad) == BFQ_E_ARG && bad == 2 && len == 3);
        q = {0, 1, 2, 1, 4};
        CHECK(bfq_perm_encode_host(q.data(), 5, nullptr, out, sizeof out, &len, &bad) == BFQ_E_ARG && bad == 3 && len == 3);
        for (u8 b : out) CHECK(b == 0xEE);
    }
    if (!g_fail) printf("ok\n");
    return g_fail ? 1 : 0;
}
