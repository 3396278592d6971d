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
// The last section holds the repair (bfq_fastq_repair*): mates matched by name wherever they stand, with its own overview.
#include "bfq_pairs_device.h"

#define PR_SCAN_THREADS 256
#define PR_SCAN_ITEMS 16
#define PR_SCAN_CHUNK (PR_SCAN_THREADS * PR_SCAN_ITEMS)          // records per chunk of the max-scan (tests/pairs_model.py names it)

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

void bfq_maxscan_u64(bfq_ctx *c, const u64 *in, u64 *out, u64 n)
{
    const u64 nb = ceil_div(n, PR_SCAN_CHUNK);
    if (nb <= 1) {
        KLAUNCH(c, K_SCAN, 16.0 * (double)n, k_pairs_maxdown, 1, PR_SCAN_THREADS, in, out, n, (const u64 *)nullptr);
        return;
    }
    const size_t m = c->mark();
    u64 *maxs = c->alloc<u64>(nb), *maxsInc = c->alloc<u64>(nb);
    KLAUNCH(c, K_SCAN, 8.0 * (double)n, k_pairs_maxred, nb, PR_SCAN_THREADS, in, n, maxs);
    bfq_maxscan_u64(c, maxs, maxsInc, nb);
    KLAUNCH(c, K_SCAN, 16.0 * (double)n, k_pairs_maxdown, nb, PR_SCAN_THREADS, in, out, n, (const u64 *)maxsInc);
    c->release(m);   // stream-ordered, as in k_scan.hip
}

// orphan mode: start[i] = the record at which the run of record i starts (N entries; start doubles as the bounds' array)
void bfq_pairs_run_starts(bfq_ctx *c, const PrText &a, u32 suffix, u64 *start)
{
    if (!a.N) return;
    KLAUNCH(c, K_PAIRS_CMP, 136.0 * (double)a.N, k_pairs_bounds, bfq_grid(a.N, 256), 256, a, suffix, start);
    bfq_maxscan_u64(c, start, start, a.N);
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

// ==== repair: the mates matched by name across the texts (bfq_fastq_repair*; the definition: bfq_pairs.h) ========================
//   k_repair_hash   : RP_LANES lanes per record: the header's bytes taken in 8-byte chunks, chunk j by lane j mod RP_LANES, once
//                     to find where the key ends (the first blank, tab or CR: a min over the lanes) and once to hash it (the
//                     commutative sum of bfq_repair_hash, added up over the lanes); h[g], the hint and the sort record (the
//                     top hash_bits bits of h where bfq_radix_sort reads its digits, payload g)
//   bfq_radix_sort  : the stable LSD passes of k_radix.hip, ceil(hash_bits / 8) of them: a run of equal sort keys is in global order
//   k_repair_sorted : per sorted position: g and its hint in one word, h, and the position where a run starts (else 0); the
//                     inclusive max-scan above gives the run start of every position
//   k_repair_runs   : the longest run (a max per wave, then one atomicMax) and the smallest global number in a run above
//                     BFQ_REPAIR_RUN_MAX (one atomicMin per such run); the host refuses before anything walks a run
//   k_repair_group  : one lane per sorted position walks its run from its start (at most BFQ_REPAIR_RUN_MAX steps) and counts
//                     the records of its group -- equal h, then equal bytes -- in front of it and in all, by hint; the role
//                     (bfq_repair_role); for an output-2 record a second walk to the output-1 record of its pair, the anchor
//   k_repair_place  : ranks are exclusive scans of the role flags in global order (a pair's rank: its anchor's); every record
//                     writes its size at its rank in its output's size array; three more scans give the offsets
//   k_repair_move   : pr_copy, 16 lanes per record, every record once, from whichever text it lies in
// No loop waits for another workgroup; every loop ends at a length from the index or at BFQ_REPAIR_RUN_MAX.
#define RP_LANES 8u

struct RpTexts { PrText t[3]; u64 n1, n12; };                       // n1: records of text 1; n12: of texts 1 and 2
__device__ __forceinline__ u32 rp_locate(const RpTexts &T, u64 g, u64 *i)
{
    if (g < T.n1) { *i = g; return 1; }
    if (g < T.n12) { *i = g - T.n1; return 2; }
    *i = g - T.n12;
    return 0;
}
// (selects, not an index into the kernel argument: an indexed copy of it would live in scratch)
__device__ __forceinline__ PrText rp_text(const RpTexts &T, u32 k)
{
    PrText r;
    r.buf = k == 1 ? T.t[1].buf : k == 2 ? T.t[2].buf : T.t[0].buf;
    r.rec = k == 1 ? T.t[1].rec : k == 2 ? T.t[2].rec : T.t[0].rec;
    r.len = k == 1 ? T.t[1].len : k == 2 ? T.t[2].len : T.t[0].len;
    r.N = k == 1 ? T.t[1].N : k == 2 ? T.t[2].N : T.t[0].N;
    return r;
}
__device__ __forceinline__ u64 rp_group_min(u64 v)
{
#pragma unroll
    for (u32 d = 1; d < RP_LANES; d <<= 1) { const u64 o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ u64 rp_group_sum(u64 v)
{
#pragma unroll
    for (u32 d = 1; d < RP_LANES; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void k_repair_hash(RpTexts T, u64 N, u32 suffix, u32 hashBits, u64 seed, u64 *__restrict__ h, u8 *__restrict__ hint,
                                                     SortRec out)
{
    const u32 sub = threadIdx.x & (RP_LANES - 1);
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) / RP_LANES;
    for (u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / RP_LANES; g < N; g += ngrp) {      // the lanes of a group share g
        u64 i;
        const u32 src = rp_locate(T, g, &i);
        const PrText tx = rp_text(T, src);
        const u8 *__restrict__ t = tx.buf;
        const u64 s = tx.rec[i].hdrStart, n = tx.rec[i].hdrLen;
        const u64 b = s + 1, m = n ? n - 1 : 0;                  // the bytes behind the '@'
        u64 end = m;
        for (u64 c = sub; 8 * c < m; c += RP_LANES) {
            const u64 len = m - 8 * c < 8 ? m - 8 * c : 8, w = rp_word(t + b + 8 * c, len);
            u64 at = m;
            for (u32 k = 0; k < 8; k++) {
                const u8 ch = (u8)(w >> (8 * k));
                if (k < len && at == m && (ch == ' ' || ch == '\t' || ch == '\r')) at = 8 * c + k;
            }
            if (at < m) { end = at; break; }
        }
        u64 l = rp_group_min(end);
        u32 hi = src;
        if (suffix && l > 2 && t[b + l - 2] == '/' && (t[b + l - 1] == '1' || t[b + l - 1] == '2')) {
            if (!src) hi = t[b + l - 1] == '1' ? 1u : 2u;
            l -= 2;
        }
        u64 acc = 0;
        for (u64 c = sub; 8 * c < l; c += RP_LANES) acc += bfq_repair_chunk(rp_word(t + b + 8 * c, l - 8 * c < 8 ? l - 8 * c : 8), c);
        acc = rp_group_sum(acc);
        if (sub == 0) {
            const u64 hv = bfq_repair_finish(acc, l, seed), key = bfq_repair_sort_key(hv, hashBits);
            h[g] = hv;
            hint[g] = (u8)hi;
            rp_sort_rec(out, g, key);
        }
    }
}

__global__ __launch_bounds__(256) void k_repair_sorted(SortRec sorted, u64 N, const u64 *__restrict__ h, const u8 *__restrict__ hint, u64 *__restrict__ sg,
                                                       u64 *__restrict__ sh, u64 *__restrict__ v)
{
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x) {
        const u64 g = rp_index(sorted.w12[p]);
        sg[p] = g | ((u64)hint[g] << 62);
        sh[p] = h[g];
        v[p] = p && rp_sort_key(sorted, p - 1) != rp_sort_key(sorted, p) ? p : 0;
    }
}

// stat[0]: the longest run; stat[1] (preset to all-ones): the smallest global number in a run above BFQ_REPAIR_RUN_MAX
__global__ __launch_bounds__(256) void k_repair_runs(const u64 *__restrict__ start, const u64 *__restrict__ sg, u64 N, unsigned long long *__restrict__ stat)
{
    u64 longest = 0;
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x) {
        if (p + 1 < N && start[p + 1] != p + 1) continue;          // p does not end its run
        const u64 s = start[p], r = p + 1 - s;
        longest = pr_max(longest, r);
        if (r > BFQ_REPAIR_RUN_MAX) atomicMin(stat + 1, (unsigned long long)(sg[s] & ~(3ull << 62)));   // a run is in global order: its first is its smallest
    }
    longest = pr_wave_incmax(longest, bfq_lane());
    if (bfq_lane() == 63 && longest) atomicMax(stat, (unsigned long long)longest);
}

__device__ __forceinline__ bool rp_same(const RpTexts &T, u64 ga, u64 gb, u32 suffix)
{
    u64 ia, ib;
    const PrText a = rp_text(T, rp_locate(T, ga, &ia)), b = rp_text(T, rp_locate(T, gb, &ib));
    return bfq_pairs_same(a.buf, a.rec[ia].hdrStart, a.rec[ia].hdrLen, b.buf, b.rec[ib].hdrStart, b.rec[ib].hdrLen, suffix);
}

// cnt[0]: groups of more than two records; cnt[1]: runs that hold more than one name.  Every run has at most
// BFQ_REPAIR_RUN_MAX records (k_repair_runs, checked by the host before this launch); the loops are bounded by it all the same.
__global__ __launch_bounds__(256) void k_repair_group(RpTexts T, u64 N, u32 suffix, const u64 *__restrict__ start, const u64 *__restrict__ sg,
                                                      const u64 *__restrict__ sh, u8 *__restrict__ role, u64 *__restrict__ anchor, u8 *__restrict__ f1,
                                                      u8 *__restrict__ f0, unsigned long long *__restrict__ cnt)
{
    const u64 GMASK = ~(3ull << 62);
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x) {
        const u64 s = start[p], me = sg[p], g = me & GMASK, hv = sh[p];
        const u32 hi = (u32)(me >> 62);
        u64 lim = s + BFQ_REPAIR_RUN_MAX < N ? s + BFQ_REPAIR_RUN_MAX : N;
        u32 before[3] = {0, 0, 0}, total[3] = {0, 0, 0};
        bool mixed = false;
        u64 e = s;
        for (; e < lim && start[e] == s; e++) {
            const u64 o = sg[e];
            if (e != p && (sh[e] != hv || !rp_same(T, g, o & GMASK, suffix))) { mixed = true; continue; }
            const u32 oh = (u32)(o >> 62);
            total[oh]++;
            if (e < p) before[oh]++;
        }
        u32 mate = 0;
        const u32 r = bfq_repair_role(hi, before, total, &mate);
        u64 a = g;
        if (r == 2) {                                             // the mate-th record of the group's list L1 (hint 0: L0)
            const u32 list = hi ? 1u : 0u;
            u32 seen = 0;
            for (u64 q = s; q < e; q++) {
                const u64 o = sg[q];
                if ((u32)(o >> 62) != list || (q != p && (sh[q] != hv || !rp_same(T, g, o & GMASK, suffix)))) continue;
                if (seen++ == mate) { a = o & GMASK; break; }
            }
        }
        role[g] = (u8)r;
        anchor[g] = a;
        f1[g] = r == 1; f0[g] = r == 0;
        if (p == s && mixed) atomicAdd(cnt + 1, 1ull);
        if (before[0] + before[1] + before[2] == 0 && total[0] + total[1] + total[2] > 2) atomicAdd(cnt, 1ull);
    }
}

__device__ __forceinline__ u64 rp_size(const RpTexts &T, u64 g)
{
    u64 i;
    const PrText t = rp_text(T, rp_locate(T, g, &i));
    return pr_rec_end(t, i) - t.rec[i].hdrStart;
}
__global__ __launch_bounds__(256) void k_repair_place(RpTexts T, u64 N, const u8 *__restrict__ role, const u64 *__restrict__ anchor,
                                                      const u64 *__restrict__ rank1, const u64 *__restrict__ rank0, u64 *__restrict__ slot, u64 *__restrict__ sz0,
                                                      u64 *__restrict__ sz1, u64 *__restrict__ sz2)
{
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (u64)gridDim.x * blockDim.x) {
        const u32 r = role[g];
        const u64 at = r ? rank1[anchor[g]] : rank0[g];
        slot[g] = at;
        (r == 0 ? sz0 : r == 1 ? sz1 : sz2)[at] = rp_size(T, g);
    }
}
__global__ __launch_bounds__(256) void k_repair_move(RpTexts T, u64 N, const u8 *__restrict__ role, const u64 *__restrict__ slot, const u64 *__restrict__ off0,
                                                     const u64 *__restrict__ off1, const u64 *__restrict__ off2, u8 *__restrict__ o0, u8 *__restrict__ o1,
                                                     u8 *__restrict__ o2)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4;
    for (u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; g < N; g += ngrp) {
        u64 i;
        const PrText t = rp_text(T, rp_locate(T, g, &i));
        const u32 r = role[g];
        const u64 s0 = t.rec[i].hdrStart, n = pr_rec_end(t, i) - s0, at = slot[g];
        u8 *dst = r == 0 ? o0 + off0[at] : r == 1 ? o1 + off1[at] : o2 + off2[at];
        pr_copy(dst, t.buf + s0, n, sub);
    }
}

static RpTexts rp_texts(const PrText t[3])
{
    RpTexts T;
    for (int k = 0; k < 3; k++) T.t[k] = t[k];
    T.n1 = t[1].N; T.n12 = t[1].N + t[2].N;
    return T;
}
// steps 1-3: sg / sh / start (N entries each) of the sorted records; d_stat[0, 2): the longest run, the first record of a run
// that is too long (preset here)
void bfq_repair_sort(bfq_ctx *c, const PrText t[3], u64 N, const bfq_repair_opts &O, u64 *h, u8 *hint, SortRec a, SortRec b, u64 *sg, u64 *sh, u64 *start,
                     u64 *d_stat)
{
    HIP_CHECK(hipMemsetAsync(d_stat, 0, 8, c->stream));
    HIP_CHECK(hipMemsetAsync(d_stat + 1, 0xFF, 8, c->stream));
    if (!N) return;
    const RpTexts T = rp_texts(t);
    KLAUNCH(c, K_PAIRS_CMP, 90.0 * (double)N, k_repair_hash, bfq_grid(N, 256 / RP_LANES), 256, T, N, O.mate_suffix, O.hash_bits, (u64)O.seed, h, hint, a);
    const SortRec sorted = bfq_radix_sort(c, a, b, N, (int)(O.hash_bits + 7) / 8);
    KLAUNCH(c, K_MISC, 53.0 * (double)N, k_repair_sorted, bfq_grid(N, 256), 256, sorted, N, (const u64 *)h, (const u8 *)hint, sg, sh, start);
    bfq_maxscan_u64(c, start, start, N);
    KLAUNCH(c, K_MISC, 16.0 * (double)N, k_repair_runs, bfq_grid(N, 256), 256, (const u64 *)start, (const u64 *)sg, N, (unsigned long long *)d_stat);
}
// step 3's walk: role / anchor / the two role flags per global number; d_cnt[0, 2) zeroed: dup_groups, mixed_runs
void bfq_repair_group(bfq_ctx *c, const PrText t[3], u64 N, u32 suffix, const u64 *start, const u64 *sg, const u64 *sh, u8 *role, u64 *anchor, u8 *f1, u8 *f0,
                      u64 *d_cnt)
{
    if (!N) return;
    KLAUNCH(c, K_PAIRS_CMP, 160.0 * (double)N, k_repair_group, bfq_grid(N, 256), 256, rp_texts(t), N, suffix, start, sg, sh, role, anchor, f1, f0,
            (unsigned long long *)d_cnt);
}
void bfq_repair_place(bfq_ctx *c, const PrText t[3], u64 N, const u8 *role, const u64 *anchor, const u64 *rank1, const u64 *rank0, u64 *slot, u64 *const sz[3])
{
    if (!N) return;
    KLAUNCH(c, K_MISC, 89.0 * (double)N, k_repair_place, bfq_grid(N, 256), 256, rp_texts(t), N, role, anchor, rank1, rank0, slot, sz[0], sz[1], sz[2]);
}
void bfq_repair_move(bfq_ctx *c, const PrText t[3], u64 N, const u8 *role, const u64 *slot, const u64 *const off[3], u8 *const o[3])
{
    if (!N) return;
    KLAUNCH(c, K_PAIRS_MOVE, 2.0 * (double)(t[0].len + t[1].len + t[2].len) + 61.0 * (double)N, k_repair_move, bfq_grid(N, 16), 256, rp_texts(t), N, role, slot,
            off[0], off[1], off[2], o[0], o[1], o[2]);
}
