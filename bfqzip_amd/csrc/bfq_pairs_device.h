// bfq_pairs_device.h -- device helpers the record movers and groupers share (k_pairs.hip, k_dedup.hip): a record's extent, the
// 16-lane copy, the wave max-scan and the layout of the sort records that carry a 40-bit hash key and a record number.
#pragma once
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_pairs.h"

// record i of a text: [hdrStart of i, hdrStart of i + 1) -- the last one ends with the text
__device__ __forceinline__ u64 pr_rec_end(const PrText &t, u64 i) { return i + 1 < t.N ? t.rec[i + 1].hdrStart : t.len; }

__device__ __forceinline__ u64 pr_max(u64 x, u64 y) { return x > y ? x : y; }
__device__ __forceinline__ u64 pr_wave_incmax(u64 m, u32 lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 t = __shfl_up(m, (unsigned)d);
        if ((int)lane >= d) m = pr_max(m, t);
    }
    return m;
}

// n bytes by 16 lanes of which this is lane `sub`: bytes up to the first 16-byte boundary of the destination, 16-byte stores
// (the loads are as aligned as the source happens to be), a byte tail.  Reads src[0, n) and writes dst[0, n), nothing else.
__device__ __forceinline__ void pr_copy(u8 *__restrict__ dst, const u8 *__restrict__ src, u64 n, u32 sub)
{
    u64 head = (16 - ((u64)(uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    if (sub < head) dst[sub] = src[sub];
    const u64 body = (n - head) >> 4;
    for (u64 q = sub; q < body; q += 16) *(uint4 *)(dst + head + 16 * q) = *(const uint4 *)(src + head + 16 * q);
    const u64 done = head + 16 * body;
    if (done + sub < n) dst[done + sub] = src[done + sub];
}

// the sort records of a hashed record: the key where bfq_radix_sort reads its digits, the record number g in the 56 bits left
__device__ __forceinline__ void rp_sort_rec(const SortRec &out, u64 g, u64 key)
{
    out.w0[g] = (u32)(key >> 8);
    out.w12[g] = ((u64)(u32)(g >> 24) << 32) | (u64)((u32)((key & 255ull) << 24) | (u32)(g & 0xFFFFFFull));
}
__device__ __forceinline__ u64 rp_index(u64 w12) { return ((w12 >> 32) << 24) | (w12 & 0xFFFFFFull); }
__device__ __forceinline__ u64 rp_sort_key(const SortRec &r, u64 p) { return ((u64)r.w0[p] << 8) | (u64)((u32)r.w12[p] >> 24); }
// n <= 8 bytes at p as a little-endian word, zero-padded: one 8-byte load where all 8 lie inside the line
__device__ __forceinline__ u64 rp_word(const u8 *__restrict__ p, u64 n)
{
    if (n < 8) return bfq_repair_word(p, n);
    u64 w;
    __builtin_memcpy(&w, p, 8);
    return w;
}
