// k_reorder.hip -- the records of a FASTQ text in another order (include/bfqzip_hip.h, bfq_fastq_reorder).
//
// The reference's parallel driver shells out for this (`BFQzip_parallel.py --reorder`, :59-75,389-437: SPRING's
// reorder-only tool or randomFASTQ.py) and then cuts the reordered file into blocks.  Here the text is already on the
// device with its record index (k_fastq.hip), so the pre-pass is four streaming steps:
//   k_ro_keys      : one 40-bit key per read (bfq_reorder.h): the smallest hashed k-mer of its sequence line (mode 2; the
//                    pair's key is mate 1's, mate 2's when mate 1 has none) or a hash of seed + index (mode 1); written
//                    as sort records with the read index as payload.  One lane per read, 16-byte loads: at 30 M x 150
//                    it takes 19-24 ms where a wave per read with the line staged in LDS took 34-39 ms
//                    (profiles/reorder/README.md keeps that kernel and the numbers)
//   bfq_radix_sort : the suffix sort's stable LSD passes (k_radix.hip), five 8-bit digits
//   k_ro_perm      : perm[j] = index of the j-th record in the new order, and its size in every mate's text; the exclusive
//                    scan of the sizes (k_scan.hip) gives the new offsets
//   k_ro_gather    : every record copied verbatim to its new offset
// Memory-bound integer work: the key pass reads the sequence lines once, the gather reads and writes the text once.
//
// The way back (bfq_fastq_reorder_keep, bfq_fastq_unreorder, bfq_fastq_restore_ordered) keeps the permutation as a BFQPERM1
// container (bfq_perm.h) and undoes it:
//   k_perm_pack    : the container's payload from perm[], one lane per 64-bit word, assembled from the entries that overlap it
//   k_perm_unpack  : perm[] from a payload, one lane per entry
//   k_perm_invert  : inv[v] = the smallest j with perm[j] = v (64-bit atomicMin into an array preset to all-ones)
//   k_perm_check   : the smallest j with perm[j] >= N or inv[perm[j]] != j -- an entry out of range, or a value met before
//   k_ro_sizes     : the record sizes in the order of an index array; k_ro_gather with inv as its permutation does the rest
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_reorder.h"
#include "bfq_perm.h"

// One lane, one sequence line, 16 bytes per load (the text buffer is padded: the last load may run past the line)
__device__ __forceinline__ u64 ro_key_lane(const u8 *__restrict__ s, u32 L, int k, u64 mask)
{
    BfqRoRoll r;
    bfq_ro_init(r);
    for (u32 p = 0; p < L; p += 16) {
        const uint4 v = *(const uint4 *)(s + p);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        const u32 n = L - p < 16u ? L - p : 16u;
#pragma unroll
        for (u32 b = 0; b < 16; b++)
            if (b < n) bfq_ro_push(r, bfq_ro_code((u8)(w[b >> 2] >> (8 * (b & 3)))), k, mask, true);
    }
    return r.found ? r.best >> 24 : ~0ull;
}

__device__ __forceinline__ void ro_put(SortRec out, u64 i, u64 key)
{
    out.w0[i] = (u32)(key >> 8);
    out.w12[i] = ((u64)(u32)(i >> 24) << 32) | (u64)((u32)((key & 255ull) << 24) | (u32)(i & 0xFFFFFFull));
}
__device__ __forceinline__ u64 ro_index(u64 w12) { return ((w12 >> 32) << 24) | (w12 & 0xFFFFFFull); }

__global__ __launch_bounds__(256) void k_ro_keys(RoText m0, RoText m1, int nmates, u64 N, int k, SortRec out)
{
    const u64 mask = bfq_ro_mask(k);
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (u64)gridDim.x * blockDim.x) {
        u64 key = ro_key_lane(m0.buf + m0.rec[i].seqStart, m0.rec[i].len, k, mask);
        if (key == ~0ull && nmates > 1) key = ro_key_lane(m1.buf + m1.rec[i].seqStart, m1.rec[i].len, k, mask);
        ro_put(out, i, key == ~0ull ? BFQ_RO_NOKEY : key);
    }
}
__global__ __launch_bounds__(256) void k_ro_keys_random(u64 N, u64 seed, SortRec out)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (u64)gridDim.x * blockDim.x)
        ro_put(out, i, bfq_fmix64(seed + i) >> 24);
}

// record i of a text: [hdrStart of i, hdrStart of i + 1) -- the last one ends with the text
__device__ __forceinline__ u64 ro_rec_end(const RoText &t, u64 i, u64 N) { return i + 1 < N ? t.rec[i + 1].hdrStart : t.len; }

__global__ __launch_bounds__(256) void k_ro_perm(SortRec sorted, RoText m0, RoText m1, int nmates, u64 N, u64 *__restrict__ perm,
                                                 u64 *__restrict__ sizes0, u64 *__restrict__ sizes1)
{
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (u64)gridDim.x * blockDim.x) {
        const u64 i = ro_index(sorted.w12[j]);
        perm[j] = i;
        sizes0[j] = ro_rec_end(m0, i, N) - m0.rec[i].hdrStart;
        if (nmates > 1) sizes1[j] = ro_rec_end(m1, i, N) - m1.rec[i].hdrStart;
    }
}

// 16 lanes per record: bytes up to the first 16-byte boundary of the destination, 16-byte stores (the loads are as
// aligned as the source happens to be), a byte tail
__global__ __launch_bounds__(256) void k_ro_gather(RoText t, const u64 *__restrict__ perm, const u64 *__restrict__ newOff, u64 N,
                                                   u8 *__restrict__ out)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 j = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < N; j += ngrp) {
        const u64 i = perm[j], s0 = t.rec[i].hdrStart, n = ro_rec_end(t, i, N) - s0;
        const u8 *__restrict__ src = t.buf + s0;
        u8 *__restrict__ dst = out + newOff[j];
        u64 head = (16 - ((u64)(uintptr_t)dst & 15)) & 15;
        if (head > n) head = n;
        if (sub < head) dst[sub] = src[sub];
        const u64 body = (n - head) >> 4;
        for (u64 q = sub; q < body; q += 16) *(uint4 *)(dst + head + 16 * q) = *(const uint4 *)(src + head + 16 * q);
        const u64 done = head + 16 * body;
        if (done + sub < n) dst[done + sub] = src[done + sub];
    }
}

// ---- the permutation as a container, and its inverse ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_perm_pack(const u64 *__restrict__ perm, u64 N, u32 w, u64 nwords, u64 *__restrict__ out)
{
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nwords; q += (u64)gridDim.x * blockDim.x)
        out[q] = bfq_perm_word(perm, N, w, q);
}
__global__ __launch_bounds__(256) void k_perm_unpack(const u64 *__restrict__ words, u64 N, u32 w, u64 *__restrict__ perm)
{
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (u64)gridDim.x * blockDim.x)
        perm[j] = bfq_perm_get(words, j, w);
}
__global__ __launch_bounds__(256) void k_perm_invert(const u64 *__restrict__ perm, u64 N, unsigned long long *__restrict__ inv)
{
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (u64)gridDim.x * blockDim.x) {
        const u64 v = perm[j];
        if (v < N) atomicMin(inv + v, (unsigned long long)j);
    }
}
__global__ __launch_bounds__(256) void k_perm_check(const u64 *__restrict__ perm, u64 N, const u64 *__restrict__ inv,
                                                    unsigned long long *__restrict__ firstBad)
{
    u64 bad = ~0ull;
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (u64)gridDim.x * blockDim.x) {
        const u64 v = perm[j];
        if ((v >= N || inv[v] != j) && j < bad) bad = j;
    }
    if (bad != ~0ull) atomicMin(firstBad, (unsigned long long)bad);
}
// sizes of the records order[0], order[1], ... of every mate
__global__ __launch_bounds__(256) void k_ro_sizes(const u64 *__restrict__ order, RoText m0, RoText m1, int nmates, u64 N,
                                                  u64 *__restrict__ sizes0, u64 *__restrict__ sizes1)
{
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (u64)gridDim.x * blockDim.x) {
        const u64 i = order[j];
        sizes0[j] = ro_rec_end(m0, i, N) - m0.rec[i].hdrStart;
        if (nmates > 1) sizes1[j] = ro_rec_end(m1, i, N) - m1.rec[i].hdrStart;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
void bfq_reorder_keys(bfq_ctx *c, const RoText *mates, int nmates, u64 N, int mode, int k, u64 seed, SortRec out)
{
    if (!N) return;
    const RoText m0 = mates[0], m1 = nmates > 1 ? mates[1] : mates[0];
    if (mode == 1)
        KLAUNCH(c, K_RO_KEYS, 12.0 * (double)N, k_ro_keys_random, bfq_grid(N, 256), 256, N, seed, out);
    else
        KLAUNCH(c, K_RO_KEYS, 0.5 * (double)m0.len + 44.0 * (double)N, k_ro_keys, bfq_grid(N, 256), 256, m0, m1, nmates, N, k, out);
}

void bfq_reorder_perm(bfq_ctx *c, SortRec sorted, const RoText *mates, int nmates, u64 N, u64 *perm, u64 *const *sizes)
{
    if (!N) return;
    KLAUNCH(c, K_MISC, (24.0 + 72.0 * nmates) * (double)N, k_ro_perm, bfq_grid(N, 256), 256, sorted, mates[0], nmates > 1 ? mates[1] : mates[0],
            nmates, N, perm, sizes[0], nmates > 1 ? sizes[1] : sizes[0]);
}

void bfq_reorder_gather(bfq_ctx *c, const RoText &t, const u64 *perm, const u64 *newOff, u64 N, u8 *d_out)
{
    if (!N) return;
    KLAUNCH(c, K_RO_GATHER, 2.0 * (double)t.len + 48.0 * (double)N, k_ro_gather, bfq_grid(N, 16), 256, t, perm, newOff, N, d_out);
}

void bfq_perm_pack(bfq_ctx *c, const u64 *perm, u64 N, u64 *d_words)
{
    const u32 w = bfq_perm_width(N);
    const u64 nw = bfq_perm_words(N, w);
    if (nw) KLAUNCH(c, K_PERM_PACK, 8.0 * (double)N + 8.0 * (double)nw, k_perm_pack, bfq_grid(nw, 256), 256, perm, N, w, nw, d_words);
}

// perm[] and inv[] (N entries each) from the payload of a container of N entries; returns the first offending position
// (BFQ_PERM_NOPOS: a permutation).  Synchronises the stream.
u64 bfq_perm_unpack_invert(bfq_ctx *c, const u64 *d_words, u64 N, u64 *perm, u64 *inv)
{
    if (!N) return BFQ_PERM_NOPOS;
    const u32 w = bfq_perm_width(N);
    unsigned long long *d_bad = (unsigned long long *)c->alloc<u64>(1);
    HIP_CHECK(hipMemsetAsync(inv, 0xFF, 8 * N, c->stream));
    HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    KLAUNCH(c, K_PERM_INVERT, 8.0 * (double)N + 8.0 * (double)bfq_perm_words(N, w), k_perm_unpack, bfq_grid(N, 256), 256, d_words, N, w, perm);
    KLAUNCH(c, K_PERM_INVERT, 16.0 * (double)N, k_perm_invert, bfq_grid(N, 256), 256, (const u64 *)perm, N, (unsigned long long *)inv);
    KLAUNCH(c, K_PERM_INVERT, 16.0 * (double)N, k_perm_check, bfq_grid(N, 256), 256, (const u64 *)perm, N, (const u64 *)inv, d_bad);
    u64 bad = BFQ_PERM_NOPOS;
    HIP_CHECK(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    return bad;
}

void bfq_reorder_sizes(bfq_ctx *c, const u64 *order, const RoText *mates, int nmates, u64 N, u64 *const *sizes)
{
    if (!N) return;
    KLAUNCH(c, K_MISC, (8.0 + 72.0 * nmates) * (double)N, k_ro_sizes, bfq_grid(N, 256), 256, order, mates[0], nmates > 1 ? mates[1] : mates[0],
            nmates, N, sizes[0], nmates > 1 ? sizes[1] : sizes[0]);
}
