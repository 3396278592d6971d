// bfq_perm.h -- the permutation of a read reordering as a file: container BFQPERM1 (include/bfqzip_hip.h), shared by the
// host statement (bfq_perm_encode / bfq_perm_decode, bfq_host.cpp) and the kernels that pack and unpack it
// (k_reorder.hip).  Plain C++, no HIP types.
//   header   40 bytes: "BFQPERM1" | u64 N | u32 w | u32 mode | u32 k | u32 0 | u64 seed   (little endian)
//   payload  ceil(N w / 64) u64 words: entry j = perm[j] in bits [j w, (j + 1) w) of the bit stream, bit b of the stream
//            being bit b % 64 of word b / 64; the padding bits of the last word are 0
// w is the bit length of N - 1 (1 when N <= 2), N < 2^56.
#pragma once
#include <stdlib.h>
#include <string.h>
#include "../../include/bfqzip_hip.h"
#include "bfq_common.h"

#define BFQ_PERM_HDR 40
#define BFQ_PERM_MAGIC "BFQPERM1"
#define BFQ_PERM_NOPOS (~0ull)                           // first_bad of a fault in the header

BFQ_HD u32 bfq_perm_width(u64 N) { return N <= 2 ? 1u : (u32)(64 - bfq_clz64(N - 1)); }
BFQ_HD u64 bfq_perm_words(u64 N, u32 w) { return (N * w + 63) >> 6; }                      // N < 2^56, w <= 56: no overflow
BFQ_HD u64 bfq_perm_mask(u32 w) { return (1ull << w) - 1; }                                  // w <= 56

// entry j of a payload
BFQ_HD u64 bfq_perm_get(const u64 *words, u64 j, u32 w)
{
    const u64 bit = j * w, q = bit >> 6;
    const u32 sh = (u32)(bit & 63);
    u64 v = words[q] >> sh;
    if (sh + w > 64) v |= words[q + 1] << (64 - sh);     // (sh > 0 here; the entry ends inside the payload, so q + 1 exists)
    return v & bfq_perm_mask(w);
}
// word q of the payload of perm[0..N): the entries that overlap bits [64 q, 64 q + 64), two or three of them once w > 21
BFQ_HD u64 bfq_perm_word(const u64 *perm, u64 N, u32 w, u64 q)
{
    const u64 lo = q << 6, mask = bfq_perm_mask(w);
    u64 j = lo / w, out = 0;
    for (; j < N; j++) {
        const u64 bit = j * w;
        if (bit >= lo + 64) break;
        const u64 v = perm[j] & mask;
        out |= bit >= lo ? v << (bit - lo) : v >> (lo - bit);
    }
    return out;
}

// ---- host side: the header, and the statement of encode / decode
static inline u64 bfq_perm_ld64(const u8 *p) { u64 v; memcpy(&v, p, 8); return v; }          // (little-endian hosts, as everywhere)
static inline u32 bfq_perm_ld32(const u8 *p) { u32 v; memcpy(&v, p, 4); return v; }

static inline u64 bfq_perm_bound_of(u64 N) { return BFQ_PERM_HDR + 8 * bfq_perm_words(N, bfq_perm_width(N)); }

// magic, N, w, the total length and the zero padding; the entries are not looked at
static inline bool bfq_perm_header(const u8 *z, u64 len, u64 *N, u32 *w, bfq_reorder_opts *opts)
{
    if (!z || len < BFQ_PERM_HDR || memcmp(z, BFQ_PERM_MAGIC, 8)) return false;
    const u64 n = bfq_perm_ld64(z + 8);
    const u32 ww = bfq_perm_ld32(z + 16);
    if (n >> 56 || ww != bfq_perm_width(n) || len != bfq_perm_bound_of(n)) return false;
    const u64 used = n * ww & 63;
    if (used && bfq_perm_ld64(z + len - 8) >> used) return false;
    if (N) *N = n;
    if (w) *w = ww;
    if (opts) {
        memset(opts, 0, sizeof *opts);
        opts->mode = (int32_t)bfq_perm_ld32(z + 20);
        opts->k = (int32_t)bfq_perm_ld32(z + 24);
        opts->seed = bfq_perm_ld64(z + 32);
    }
    return true;
}
static inline void bfq_perm_put_header(u8 *out, u64 N, const bfq_reorder_opts *opts)
{
    const u32 w = bfq_perm_width(N), mode = opts ? (u32)opts->mode : 0u, k = opts ? (u32)opts->k : 0u, zero = 0;
    const u64 seed = opts ? opts->seed : 0;
    memcpy(out, BFQ_PERM_MAGIC, 8);
    memcpy(out + 8, &N, 8); memcpy(out + 16, &w, 4); memcpy(out + 20, &mode, 4); memcpy(out + 24, &k, 4);
    memcpy(out + 28, &zero, 4); memcpy(out + 32, &seed, 8);
}

// The smallest j with get(j) >= N or get(j) met at an earlier position; BFQ_PERM_NOPOS: a permutation.  *nomem: no room for
// the N bits of bookkeeping.
template <class Get> static inline u64 bfq_perm_first_bad(u64 N, Get get, bool *nomem)
{
    *nomem = false;
    if (!N) return BFQ_PERM_NOPOS;
    u64 *seen = (u64 *)calloc((size_t)((N + 63) >> 6), 8);
    if (!seen) { *nomem = true; return BFQ_PERM_NOPOS; }
    u64 bad = BFQ_PERM_NOPOS;
    for (u64 j = 0; j < N; j++) {
        const u64 v = get(j);
        if (v >= N || (seen[v >> 6] >> (v & 63) & 1)) { bad = j; break; }
        seen[v >> 6] |= 1ull << (v & 63);
    }
    free(seen);
    return bad;
}

static inline int bfq_perm_encode_host(const u64 *h_perm, u64 N, const bfq_reorder_opts *opts, u8 *h_out, u64 cap, u64 *out_len,
                                       u64 *first_bad)
{
    if (first_bad) *first_bad = BFQ_PERM_NOPOS;
    if ((!h_perm && N) || N >> 56 || !h_out || cap < bfq_perm_bound_of(N)) return BFQ_E_ARG;
    bool nomem = false;
    const u64 bad = bfq_perm_first_bad(N, [&](u64 j) { return h_perm[j]; }, &nomem);
    if (nomem) return BFQ_E_NOMEM;
    if (bad != BFQ_PERM_NOPOS) { if (first_bad) *first_bad = bad; return BFQ_E_ARG; }
    const u32 w = bfq_perm_width(N);
    const u64 nw = bfq_perm_words(N, w);
    bfq_perm_put_header(h_out, N, opts);
    for (u64 q = 0; q < nw; q++) {
        const u64 v = bfq_perm_word(h_perm, N, w, q);
        memcpy(h_out + BFQ_PERM_HDR + 8 * q, &v, 8);
    }
    if (out_len) *out_len = BFQ_PERM_HDR + 8 * nw;
    return BFQ_OK;
}

static inline int bfq_perm_decode_host(const u8 *h_permz, u64 len, u64 *h_perm, u64 cap_entries, u64 *N, bfq_reorder_opts *opts_out,
                                       u64 *first_bad)
{
    if (first_bad) *first_bad = BFQ_PERM_NOPOS;
    u64 n = 0;
    u32 w = 0;
    bfq_reorder_opts o;
    if (!bfq_perm_header(h_permz, len, &n, &w, &o) || cap_entries < n || (!h_perm && n)) return BFQ_E_ARG;
    // the payload starts 40 bytes into the container: 8-byte aligned whenever the container is
    const u8 *pay = h_permz + BFQ_PERM_HDR;
    auto get = [&](u64 j) {
        const u64 bit = j * w, q = bit >> 6;
        const u32 sh = (u32)(bit & 63);
        u64 v = bfq_perm_ld64(pay + 8 * q) >> sh;
        if (sh + w > 64) v |= bfq_perm_ld64(pay + 8 * q + 8) << (64 - sh);
        return v & bfq_perm_mask(w);
    };
    bool nomem = false;
    const u64 bad = bfq_perm_first_bad(n, get, &nomem);
    if (nomem) return BFQ_E_NOMEM;
    if (bad != BFQ_PERM_NOPOS) { if (first_bad) *first_bad = bad; return BFQ_E_ARG; }
    for (u64 j = 0; j < n; j++) h_perm[j] = get(j);
    if (N) *N = n;
    if (opts_out) *opts_out = o;
    return BFQ_OK;
}
