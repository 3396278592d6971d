// k_pairs.hip -- interleaved paired FASTQ on the device (include/bfqzip_hip.h, bfq_fastq_deinterleave* / bfq_fastq_interleave*;
// the definition: bfq_pairs.h).  The texts stand on the device with their record index (k_fastq.hip), so both directions
// are a few streaming steps over the index and one copy of the text:
//   k_pairs_cmp     : one lane per couple that is a pair -- records 2k and 2k + 1 of one text (strict split), or record k of
//                     two texts (merge) --, the two keys compared where they lie; the lowest differing pair through one
//                     atomicMin per lane that met one
//   k_pairs_bounds  : orphan mode: v[i] = i where key(i - 1) != key(i), else 0 (one lane per couple (i - 1, i))
//   k_pairs_maxred / k_pairs_maxdown : the run start of every record, an inclusive max-scan of v over the whole file in chunks
//                     of PR_SCAN_CHUNK records: chunk maxima, their scan (the same two kernels, one level up), and the scan
//                     inside each chunk from the chunk's carry -- a run that spans chunks keeps its start through the carry
//   k_pairs_roles   : orphan mode: the output of every record (bfq_pairs_role) and its size in that output's size array;
//                     three exclusive prefix sums (k_scan.hip) place the records
//   k_pairs_psizes  : strict split: the sizes of the even records; ONE prefix sum gives output 1's offsets, and output 2's
//                     follow from the index (the bytes in front of record 2k are those of both outputs in front of pair k).
//                     The merge needs no sum at all: pair k starts at the sum of the two mates' header starts.
//   k_pairs_split / k_pairs_split_roles / k_pairs_merge : every record copied once, 16 lanes per record: bytes up to the
//                     destination's first 16-byte boundary, 16-byte stores, a byte tail (the manner of k_ro_gather).  Strict
//                     split and merge find the source record from the output index: no role or permutation array.
// Every loop ends at a length taken from the index, never at a byte found in the text.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_pairs.h"

#define PR_SCAN_THREADS 256
#define PR_SCAN_ITEMS 16
#define PR_SCAN_CHUNK (PR_SCAN_THREADS * PR_SCAN_ITEMS)          // records per chunk of the max-scan (tests/pairs_model.py names it)

// record i of a text: [hdrStart of i, hdrStart of i + 1) -- the last one ends with the text
__device__ __forceinline__ u64 pr_rec_end(const PrText &t, u64 i) { return i + 1 < t.N ? t.rec[i + 1].hdrStart : t.len; }
__device__ __forceinline__ bool pr_same(const PrText &a, u64 ia, const PrText &b, u64 ib, u32 suffix)
{
    return bfq_pairs_same(a.buf, a.rec[ia].hdrStart, a.rec[ia].hdrLen, b.buf, b.rec[ib].hdrStart, b.rec[ib].hdrLen, suffix);
}

// two: pair k is record k of a and of b; else records 2k and 2k + 1 of a
__global__ __launch_bounds__(256) void k_pairs_cmp(PrText a, PrText b, u32 two, u64 P, u32 suffix, unsigned long long *__restrict__ firstBad)
{
    u64 bad = BFQ_PAIRS_NONE;
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < P; k += (u64)gridDim.x * blockDim.x) {
        const bool same = two ? pr_same(a, k, b, k, suffix) : pr_same(a, 2 * k, a, 2 * k + 1, suffix);
        if (!same && k < bad) bad = k;
    }
    if (bad != BFQ_PAIRS_NONE) atomicMin(firstBad, (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void k_pairs_bounds(PrText a, u32 suffix, u64 *__restrict__ v)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.N; i += (u64)gridDim.x * blockDim.x)
        v[i] = i && !pr_same(a, i - 1, a, i, suffix) ? i : 0;
}

// ---- inclusive max-scan of u64 ----------------------------------------------------------------------------------------------
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
__global__ __launch_bounds__(PR_SCAN_THREADS) void k_pairs_maxred(const u64 *__restrict__ in, u64 n, u64 *__restrict__ maxs)
{
    __shared__ u64 sh[4];
    const u64 base = (u64)blockIdx.x * PR_SCAN_CHUNK;
    u64 m = 0;
#pragma unroll
    for (int k = 0; k < PR_SCAN_ITEMS; k++) {
        const u64 i = base + (u64)k * PR_SCAN_THREADS + threadIdx.x;
        if (i < n) m = pr_max(m, in[i]);
    }
    m = pr_wave_incmax(m, bfq_lane());
    if (bfq_lane() == 63) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) maxs[blockIdx.x] = pr_max(pr_max(sh[0], sh[1]), pr_max(sh[2], sh[3]));
}
// each thread owns PR_SCAN_ITEMS consecutive elements; carryInc: the inclusive scan of the chunk maxima (nullptr: one chunk).
// in == out is allowed: a thread reads its own elements before it writes them.
__global__ __launch_bounds__(PR_SCAN_THREADS) void k_pairs_maxdown(const u64 *in, u64 *out, u64 n, const u64 *__restrict__ carryInc)
{
    __shared__ u64 sh[4];
    const u64 base = (u64)blockIdx.x * PR_SCAN_CHUNK + (u64)threadIdx.x * PR_SCAN_ITEMS;
    const u32 lane = bfq_lane(), w = threadIdx.x >> 6;
    u64 v[PR_SCAN_ITEMS], m = 0;
#pragma unroll
    for (int k = 0; k < PR_SCAN_ITEMS; k++) {
        const u64 i = base + k;
        v[k] = i < n ? in[i] : 0;
        m = pr_max(m, v[k]);
    }
    const u64 inc = pr_wave_incmax(m, lane);
    if (lane == 63) sh[w] = inc;
    u64 run = __shfl_up(inc, 1u);                                   // the lanes before mine in this wave
    if (lane == 0) run = 0;
    __syncthreads();
    for (u32 j = 0; j < w; j++) run = pr_max(run, sh[j]);            // the waves before mine
    if (carryInc && blockIdx.x) run = pr_max(run, carryInc[blockIdx.x - 1]);   // the chunks before mine
#pragma unroll
    for (int k = 0; k < PR_SCAN_ITEMS; k++) {
        const u64 i = base + k;
        run = pr_max(run, v[k]);
        if (i < n) out[i] = run;
    }
}

// ---- roles and sizes -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pairs_roles(PrText a, const u64 *__restrict__ start, u8 *__restrict__ role, u64 *__restrict__ sz0,
                                                     u64 *__restrict__ sz1, u64 *__restrict__ sz2, unsigned long long *__restrict__ cnt)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < a.N; i += (u64)gridDim.x * blockDim.x) {
        const bool last = i + 1 == a.N || start[i + 1] == i + 1;
        const u32 r = bfq_pairs_role(i, start[i], last);
        const u64 n = pr_rec_end(a, i) - a.rec[i].hdrStart;
        role[i] = (u8)r;
        sz0[i] = r == 0 ? n : 0; sz1[i] = r == 1 ? n : 0; sz2[i] = r == 2 ? n : 0;
        if (r == 0) atomicAdd(cnt, 1ull);
        if (r == 1) atomicAdd(cnt + 1, 1ull);
    }
}
__global__ __launch_bounds__(256) void k_pairs_psizes(PrText a, u64 P, u64 *__restrict__ sz)
{
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < P; k += (u64)gridDim.x * blockDim.x)
        sz[k] = a.rec[2 * k + 1].hdrStart - a.rec[2 * k].hdrStart;
}

// ---- the move --------------------------------------------------------------------------------------------------------------
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

// strict split: record j of the text is mate 1 + (j & 1) of pair j / 2; off1[k]: where pair k's first mate starts in output 1
__global__ __launch_bounds__(256) void k_pairs_split(PrText a, const u64 *__restrict__ off1, u8 *__restrict__ o1, u8 *__restrict__ o2)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 j = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < a.N; j += ngrp) {
        const u64 k = j >> 1, s0 = a.rec[j].hdrStart, n = pr_rec_end(a, j) - s0, at1 = off1[k];
        u8 *dst = (j & 1) ? o2 + (a.rec[2 * k].hdrStart - at1) : o1 + at1;
        pr_copy(dst, a.buf + s0, n, sub);
    }
}
__global__ __launch_bounds__(256) void k_pairs_split_roles(PrText a, const u8 *__restrict__ role, const u64 *__restrict__ off0, const u64 *__restrict__ off1,
                                                           const u64 *__restrict__ off2, u8 *__restrict__ o0, u8 *__restrict__ o1, u8 *__restrict__ o2)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 j = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < a.N; j += ngrp) {
        const u64 s0 = a.rec[j].hdrStart, n = pr_rec_end(a, j) - s0;
        const u32 r = role[j];
        u8 *dst = r == 0 ? o0 + off0[j] : r == 1 ? o1 + off1[j] : o2 + off2[j];
        pr_copy(dst, a.buf + s0, n, sub);
    }
}
// merge: output record j is record j / 2 of text 1 + (j & 1); pair k starts where the two mates' records k start, added
__global__ __launch_bounds__(256) void k_pairs_merge(PrText a, PrText b, u8 *__restrict__ out)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 j = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < 2 * a.N; j += ngrp) {
        const u64 k = j >> 1, sa = a.rec[k].hdrStart, sb = b.rec[k].hdrStart, na = pr_rec_end(a, k) - sa;
        if (j & 1) pr_copy(out + sa + sb + na, b.buf + sb, pr_rec_end(b, k) - sb, sub);
        else pr_copy(out + sa + sb, a.buf + sa, na, sub);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// the lowest pair whose keys differ into *d_firstBad (preset to all-ones): records (2k, 2k + 1) of a, or record k of a and b
void bfq_pairs_compare(bfq_ctx *c, const PrText &a, const PrText *b, u64 P, u32 suffix, u64 *d_firstBad)
{
    if (!P) return;
    KLAUNCH(c, K_PAIRS_CMP, 128.0 * (double)P, k_pairs_cmp, bfq_grid(P, 256), 256, a, b ? *b : a, b ? 1u : 0u, P, suffix, (unsigned long long *)d_firstBad);
}

static void pr_maxscan(bfq_ctx *c, const u64 *in, u64 *out, u64 n)
{
    const u64 nb = ceil_div(n, PR_SCAN_CHUNK);
    if (nb <= 1) {
        KLAUNCH(c, K_SCAN, 16.0 * (double)n, k_pairs_maxdown, 1, PR_SCAN_THREADS, in, out, n, (const u64 *)nullptr);
        return;
    }
    const size_t m = c->mark();
    u64 *maxs = c->alloc<u64>(nb), *maxsInc = c->alloc<u64>(nb);
    KLAUNCH(c, K_SCAN, 8.0 * (double)n, k_pairs_maxred, nb, PR_SCAN_THREADS, in, n, maxs);
    pr_maxscan(c, maxs, maxsInc, nb);
    KLAUNCH(c, K_SCAN, 16.0 * (double)n, k_pairs_maxdown, nb, PR_SCAN_THREADS, in, out, n, (const u64 *)maxsInc);
    c->release(m);   // stream-ordered, as in k_scan.hip
}

// orphan mode: start[i] = the record at which the run of record i starts (N entries; start doubles as the bounds' array)
void bfq_pairs_run_starts(bfq_ctx *c, const PrText &a, u32 suffix, u64 *start)
{
    if (!a.N) return;
    KLAUNCH(c, K_PAIRS_CMP, 136.0 * (double)a.N, k_pairs_bounds, bfq_grid(a.N, 256), 256, a, suffix, start);
    pr_maxscan(c, start, start, a.N);
}
// ... the roles, the sizes per output (sz[k][i]: record i's size where it goes to output k, else 0) and d_cnt[0, 2): singles, pairs
void bfq_pairs_roles(bfq_ctx *c, const PrText &a, const u64 *start, u8 *role, u64 *const sz[3], u64 *d_cnt)
{
    if (!a.N) return;
    KLAUNCH(c, K_MISC, 81.0 * (double)a.N, k_pairs_roles, bfq_grid(a.N, 256), 256, a, start, role, sz[0], sz[1], sz[2], (unsigned long long *)d_cnt);
}
void bfq_pairs_pair_sizes(bfq_ctx *c, const PrText &a, u64 P, u64 *sz)
{
    if (!P) return;
    KLAUNCH(c, K_MISC, 72.0 * (double)P, k_pairs_psizes, bfq_grid(P, 256), 256, a, P, sz);
}
void bfq_pairs_split(bfq_ctx *c, const PrText &a, const u64 *off1, u8 *o1, u8 *o2)
{
    if (!a.N) return;
    KLAUNCH(c, K_PAIRS_MOVE, 2.0 * (double)a.len + 44.0 * (double)a.N, k_pairs_split, bfq_grid(a.N, 16), 256, a, off1, o1, o2);
}
void bfq_pairs_split_roles(bfq_ctx *c, const PrText &a, const u8 *role, const u64 *const off[3], u8 *const o[3])
{
    if (!a.N) return;
    KLAUNCH(c, K_PAIRS_MOVE, 2.0 * (double)a.len + 49.0 * (double)a.N, k_pairs_split_roles, bfq_grid(a.N, 16), 256, a, role, off[0], off[1], off[2], o[0], o[1], o[2]);
}
void bfq_pairs_merge(bfq_ctx *c, const PrText &a, const PrText &b, u8 *out)
{
    if (!a.N) return;
    KLAUNCH(c, K_PAIRS_MOVE, 2.0 * (double)(a.len + b.len) + 128.0 * (double)a.N, k_pairs_merge, bfq_grid(2 * a.N, 16), 256, a, b, out);
}
