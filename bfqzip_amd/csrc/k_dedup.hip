// k_dedup.hip -- exact duplicate removal on the device (include/bfqzip_hip.h, bfq_fastq_dedup*; the definition: bfq_dedup.h).
// The one or two texts stand on the device with their record index (k_fastq.hip); unit g is record g of each.
//   k_dedup_hash    : DD_LANES lanes per unit: the sequence line in 8-byte chunks, chunk j by lane j mod DD_LANES (the commutative
//                     sum of bfq_repair_hash, added up over the lanes), the two mates' hashes combined in order; keep = 1: the
//                     quality line the same way for the score; h[g], score[g] and the sort record (the top hash_bits bits of h
//                     where bfq_radix_sort reads its digits, payload g)
//   bfq_radix_sort  : the stable LSD passes of k_radix.hip, ceil(hash_bits / 8) of them: a run of equal sort keys is in global order
//   k_dedup_sorted  : per sorted position: g, h and the position where a run starts (else 0) -- the inclusive max-scan of
//                     k_pairs.hip gives every position's run start --; every run's head = its first position, no proposal
//   k_dedup_runs    : the longest run (a max per wave, then an atomicMax where the wave's is larger than the counter stands)
//   k_dedup_round   : DD_LANES lanes per unresolved position: full hash, lengths, then the bytes against the run's head, 16 bytes
//                     per lane and step (the head's line comes from cache: a whole run reads the same one); equal: rep[p] = head;
//                     else one atomicMin of p on the run's proposal.  The unresolved are counted per wave, one atomicAdd each;
//                     the host reads the counter and stops at 0
//   k_dedup_advance : between rounds: a run with a proposal takes it as its head (and counts as mixed, once)
//   k_dedup_count   : group sizes: a run that never had a proposal is one group of the run's length, written by its last
//                     position; else one atomicAdd per wave and group.  keep = 1: atomicMax of the score per wave and group
//   k_dedup_win     : keep = 1: atomicMin of g among the units that hold their group's maximum, per wave and group
//   k_dedup_flags   : kept[g]; at the heads the duplication levels through LDS counters (groups of one: a register, added once
//                     per wave), the largest group (a max per wave); a few workgroups that stride, so that the counters of a
//                     workgroup reach global memory 2048 times, not once per 256 positions
//   k_dedup_first   : the smallest g among the heads of the largest groups (a group's head is its smallest g)
//   k_dedup_sizes / k_dedup_move : the kept records' sizes in global order -- one exclusive scan (k_scan.hip) per text places
//                     them, and a removed record starts at its place in the text less the kept bytes in front of it --;
//                     pr_copy, 16 lanes per record, every record once
// "Per wave and group": the lanes of a wave that name the same group are found by ballot, reduced, and their first lane issues
// the atomic: a group of 10^5 units in one run is 10^5 / 64 atomics.  A unit alone in its run takes none.
// No loop waits for another workgroup; every loop over bytes ends at a length from the index.  Loops over positions have the
// same trip count for all lanes of a wave: the cross-lane steps run converged.
#include "bfq_pairs_device.h"
#include "bfq_dedup.h"

#define DD_LANES 8u
#define DD_NONE (~0ull)

// (selects, not an index into the kernel argument: an indexed copy of it would live in scratch)
__device__ __forceinline__ PrText dd_text(const DdTexts &T, u32 m)
{
    PrText r;
    r.buf = m ? T.t[1].buf : T.t[0].buf;
    r.rec = m ? T.t[1].rec : T.t[0].rec;
    r.len = m ? T.t[1].len : T.t[0].len;
    r.N = m ? T.t[1].N : T.t[0].N;
    return r;
}
// a counter that only grows, as it stands now: a wave whose value is no larger has nothing to add (47 000 waves on one address)
__device__ __forceinline__ u64 dd_peek(const unsigned long long *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ u64 dd_wave_id() { return ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
__device__ __forceinline__ u64 dd_waves() { return ((u64)gridDim.x * blockDim.x) >> 6; }
__device__ __forceinline__ u64 dd_group_sum(u64 v)
{
#pragma unroll
    for (u32 d = 1; d < DD_LANES; d <<= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ u64 dd_wave_sum(u64 v)
{
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(256) void k_dedup_hash(DdTexts T, u64 N, u32 keep, u32 hashBits, u64 seed, u64 *__restrict__ h, u64 *__restrict__ score, SortRec out)
{
    const u32 lane = bfq_lane(), sub = lane & (DD_LANES - 1);
    for (u64 g0 = dd_wave_id() * (64 / DD_LANES); g0 < N; g0 += dd_waves() * (64 / DD_LANES)) {
        const u64 g = g0 + lane / DD_LANES;
        const bool ok = g < N;
        u64 hv = 0, sc = 0;
        for (u32 m = 0; m < T.nt; m++) {
            const PrText tx = dd_text(T, m);
            const u64 l = ok ? tx.rec[g].len : 0;
            const u8 *__restrict__ seq = tx.buf + (ok ? tx.rec[g].seqStart : 0), *__restrict__ ql = tx.buf + (ok ? tx.rec[g].qualStart : 0);
            u64 acc = 0;
            for (u64 c = sub; 8 * c < l; c += DD_LANES) {
                const u64 n = l - 8 * c < 8 ? l - 8 * c : 8;
                acc += bfq_repair_chunk(rp_word(seq + 8 * c, n), c);
                if (keep) {
                    const u64 w = rp_word(ql + 8 * c, n);          // (the bytes of the padding are 0 and count 0)
#pragma unroll
                    for (u32 k = 0; k < 8; k++) sc += bfq_dedup_qual((u8)(w >> (8 * k)));
                }
            }
            const u64 hk = bfq_repair_finish(dd_group_sum(acc), l, seed);
            hv = m ? bfq_dedup_pair_hash(hv, hk) : hk;
        }
        sc = dd_group_sum(sc);
        if (ok && sub == 0) {
            h[g] = hv;
            if (keep) score[g] = sc;
            rp_sort_rec(out, g, bfq_repair_sort_key(hv, hashBits));
        }
    }
}

__global__ __launch_bounds__(256) void k_dedup_sorted(SortRec sorted, u64 N, const u64 *__restrict__ h, DdGroups G)
{
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x) {
        const u64 g = rp_index(sorted.w12[p]);
        G.sg[p] = g;
        G.sh[p] = h[g];
        G.start[p] = p && rp_sort_key(sorted, p - 1) != rp_sort_key(sorted, p) ? p : 0;
        G.head[p] = p; G.next[p] = DD_NONE; G.rep[p] = DD_NONE; G.mixed[p] = 0;
    }
}

__global__ __launch_bounds__(256) void k_dedup_runs(const u64 *__restrict__ start, u64 N, unsigned long long *__restrict__ stat)
{
    u64 longest = 0;
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x)
        if (p + 1 == N || start[p + 1] == p + 1) longest = pr_max(longest, p + 1 - start[p]);   // p ends its run
    longest = pr_wave_incmax(longest, bfq_lane());
    if (bfq_lane() == 63 && longest > dd_peek(stat + DD_S_MAXRUN)) atomicMax(stat + DD_S_MAXRUN, (unsigned long long)longest);
}

// do the l bytes at a and at b differ?  This lane's share of them: 16-byte steps q = sub, sub + DD_LANES, ... and the bytes
// behind the last whole step.  Reads a[0, l) and b[0, l), nothing else.
__device__ __forceinline__ u32 dd_bytes_differ(const u8 *__restrict__ a, const u8 *__restrict__ b, u64 l, u32 sub)
{
    u32 diff = 0;
    const u64 body = l >> 4;
    for (u64 q = sub; q < body; q += DD_LANES) {
        uint4 x, y;
        __builtin_memcpy(&x, a + 16 * q, 16);
        __builtin_memcpy(&y, b + 16 * q, 16);
        diff |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
    }
    for (u64 j = 16 * body + sub; j < l; j += DD_LANES) diff |= (u32)(a[j] ^ b[j]);
    return diff;
}

__global__ __launch_bounds__(256) void k_dedup_round(DdTexts T, u64 N, DdGroups G, unsigned long long *__restrict__ stat)
{
    const u32 lane = bfq_lane(), sub = lane & (DD_LANES - 1);
    u64 mine = 0;
    for (u64 p0 = dd_wave_id() * (64 / DD_LANES); p0 < N; p0 += dd_waves() * (64 / DD_LANES)) {
        const u64 p = p0 + lane / DD_LANES;
        const bool live = p < N && G.rep[p] == DD_NONE;
        u64 s = 0, hd = 0;
        u32 diff = 0;
        if (live) {
            s = G.start[p]; hd = G.head[s];
            if (hd != p) {
                if (G.sh[p] != G.sh[hd]) diff = 1;
                else {
                    const u64 ga = G.sg[p], gb = G.sg[hd];
                    for (u32 m = 0; m < T.nt; m++) {
                        const PrText tx = dd_text(T, m);
                        const u64 la = tx.rec[ga].len, lb = tx.rec[gb].len;
                        if (la != lb) diff = 1;
                        else diff |= dd_bytes_differ(tx.buf + tx.rec[ga].seqStart, tx.buf + tx.rec[gb].seqStart, la, sub);
                    }
                }
            }
        }
#pragma unroll
        for (u32 d = 1; d < DD_LANES; d <<= 1) diff |= __shfl_xor(diff, d);
        if (live && sub == 0) {
            if (!diff) G.rep[p] = hd;
            else { atomicMin((unsigned long long *)&G.next[s], (unsigned long long)p); mine++; }
        }
    }
    mine = dd_wave_sum(mine);
    if (lane == 0 && mine) atomicAdd(stat + DD_S_UNRES, (unsigned long long)mine);
}

__global__ __launch_bounds__(256) void k_dedup_advance(u64 N, DdGroups G, unsigned long long *__restrict__ stat)
{
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x) {
        if (G.start[p] != p || G.next[p] == DD_NONE) continue;
        G.head[p] = G.next[p]; G.next[p] = DD_NONE;
        if (!G.mixed[p]) { G.mixed[p] = 1; atomicAdd(stat + DD_S_MIXED, 1ull); }
    }
}

// the smallest global number in a run that still holds unresolved positions (a run is in global order: its first is its smallest)
__global__ __launch_bounds__(256) void k_dedup_first_bad(u64 N, DdGroups G, unsigned long long *__restrict__ firstBad)
{
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x)
        if (G.rep[p] == DD_NONE) atomicMin(firstBad, (unsigned long long)G.sg[G.start[p]]);
}

// One atomic per wave and key: among the lanes that are `on`, those with equal keys are reduced -- OP 0: counted, 1: the largest
// val, 2: the smallest val -- and their first lane applies the result to arr[key].  Called by all 64 lanes.
template <int OP> __device__ __forceinline__ void dd_wave_atomic(unsigned long long *__restrict__ arr, bool on, u64 key, u64 val, u32 lane)
{
    u64 todo = __ballot(on);
    while (todo) {
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const u64 k = bfq_readlane64(key, lead);
        const bool in = on && key == k;
        const u64 m = __ballot(in);
        u64 r;
        if (OP == 0) r = (u64)__popcll(m);
        else if (__popcll(m) == 1) r = bfq_readlane64(val, lead);
        else {
            r = in ? val : OP == 1 ? 0ull : DD_NONE;
#pragma unroll
            for (u32 d = 1; d < 64; d <<= 1) {
                const u64 o = __shfl_xor(r, d);
                r = OP == 1 ? (o > r ? o : r) : (o < r ? o : r);
            }
        }
        if ((int)lane == lead) {
            if (OP == 0) atomicAdd(arr + k, (unsigned long long)r);
            else if (OP == 1) atomicMax(arr + k, (unsigned long long)r);
            else atomicMin(arr + k, (unsigned long long)r);
        }
        todo &= ~m;
    }
}
// p is the only position of its run
__device__ __forceinline__ bool dd_alone(const DdGroups &G, u64 p, u64 N) { return G.start[p] == p && (p + 1 == N || G.start[p + 1] == p + 1); }

__global__ __launch_bounds__(256) void k_dedup_count(u64 N, u32 keep, DdGroups G, const u64 *__restrict__ score, unsigned long long *__restrict__ gsize,
                                                     unsigned long long *__restrict__ best)
{
    const u32 lane = bfq_lane();
    for (u64 p0 = dd_wave_id() * 64; p0 < N; p0 += dd_waves() * 64) {
        const u64 p = p0 + lane;
        const bool ok = p < N;
        u64 s = 0, hd = 0, sc = 0;
        bool pure = false, alone = false;
        if (ok) {
            s = G.start[p]; hd = G.rep[p];
            pure = !G.mixed[s];
            alone = dd_alone(G, p, N);
            if (pure && (p + 1 == N || G.start[p + 1] == p + 1)) gsize[s] = p + 1 - s;       // one group: the run's length, by its last position
            if (keep && !alone) sc = score[G.sg[p]];
        }
        dd_wave_atomic<0>(gsize, ok && !pure, hd, 0, lane);
        if (keep) dd_wave_atomic<1>(best, ok && !alone, hd, sc, lane);
    }
}

__global__ __launch_bounds__(256) void k_dedup_win(u64 N, DdGroups G, const u64 *__restrict__ score, const u64 *__restrict__ best, unsigned long long *__restrict__ win)
{
    const u32 lane = bfq_lane();
    for (u64 p0 = dd_wave_id() * 64; p0 < N; p0 += dd_waves() * 64) {
        const u64 p = p0 + lane;
        u64 hd = 0, g = 0;
        bool holds = false;
        if (p < N && !dd_alone(G, p, N)) {
            hd = G.rep[p]; g = G.sg[p];
            holds = score[g] == best[hd];
        }
        dd_wave_atomic<2>(win, holds, hd, g, lane);
    }
}

__global__ __launch_bounds__(256) void k_dedup_flags(u64 N, u32 keep, DdGroups G, const u64 *__restrict__ gsize, const u64 *__restrict__ win, u8 *__restrict__ kept,
                                                     unsigned long long *__restrict__ stat)
{
    __shared__ unsigned long long lg[32], lu[32];
    const u32 lane = bfq_lane();
    if (threadIdx.x < 32) lg[threadIdx.x] = lu[threadIdx.x] = 0;
    __syncthreads();
    u64 nk = 0, big = 0, ones = 0;
    for (u64 p0 = dd_wave_id() * 64; p0 < N; p0 += dd_waves() * 64) {
        const u64 p = p0 + lane;
        if (p >= N) continue;
        const u64 g = G.sg[p], hd = G.rep[p];
        const bool k = keep ? dd_alone(G, p, N) || win[hd] == g : hd == p;
        kept[g] = k;
        nk += k;
        if (hd != p) continue;                                     // the heads: one per group
        const u64 n = gsize[p];
        if (n == 1) { ones++; continue; }                          // (most groups: counted in a register, added once per wave)
        const u32 l = bfq_dedup_level(n);
        atomicAdd(&lg[l], 1ull);
        atomicAdd(&lu[l], (unsigned long long)n);
        big = pr_max(big, n);
    }
    nk = dd_wave_sum(nk);
    ones = dd_wave_sum(ones);
    big = pr_wave_incmax(pr_max(big, ones ? 1 : 0), lane);
    if (lane == 0 && nk) atomicAdd(stat + DD_S_KEPT, (unsigned long long)nk);
    if (lane == 0 && ones) { atomicAdd(&lg[0], (unsigned long long)ones); atomicAdd(&lu[0], (unsigned long long)ones); }
    if (lane == 63 && big > dd_peek(stat + DD_S_MAXGROUP)) atomicMax(stat + DD_S_MAXGROUP, (unsigned long long)big);
    __syncthreads();
    if (threadIdx.x < 32 && lg[threadIdx.x]) {
        atomicAdd(stat + DD_S_LGROUPS + threadIdx.x, lg[threadIdx.x]);
        atomicAdd(stat + DD_S_LUNITS + threadIdx.x, lu[threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void k_dedup_first(u64 N, DdGroups G, const u64 *__restrict__ gsize, unsigned long long *__restrict__ stat)
{
    const u64 big = stat[DD_S_MAXGROUP];
    u64 first = DD_NONE;
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < N; p += (u64)gridDim.x * blockDim.x)
        if (G.rep[p] == p && gsize[p] == big && G.sg[p] < first) first = G.sg[p];
    if (first != DD_NONE) atomicMin(stat + DD_S_FIRST, (unsigned long long)first);
}

__global__ __launch_bounds__(256) void k_dedup_sizes(DdTexts T, u64 N, const u8 *__restrict__ kept, u64 *__restrict__ sz0, u64 *__restrict__ sz1)
{
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < N; g += (u64)gridDim.x * blockDim.x) {
        const bool k = kept[g];
        sz0[g] = k ? pr_rec_end(T.t[0], g) - T.t[0].rec[g].hdrStart : 0;
        if (T.nt == 2) sz1[g] = k ? pr_rec_end(T.t[1], g) - T.t[1].rec[g].hdrStart : 0;
    }
}
// record j: unit j / nt of text j % nt.  off[g]: the kept bytes of the text in front of unit g; a removed record starts at
// its place in the text less those.  A null output is not written.
__global__ __launch_bounds__(256) void k_dedup_move(DdTexts T, u64 N, const u8 *__restrict__ kept, const u64 *__restrict__ off0, const u64 *__restrict__ off1,
                                                    u8 *__restrict__ o0, u8 *__restrict__ o1, u8 *__restrict__ d0, u8 *__restrict__ d1)
{
    const u32 sub = threadIdx.x & 15u;
    const u64 ngrp = ((u64)gridDim.x * blockDim.x) >> 4, R = (u64)T.nt * N;
    for (u64 j = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 4; j < R; j += ngrp) {
        const u32 m = T.nt == 2 ? (u32)(j & 1) : 0u;
        const u64 g = T.nt == 2 ? j >> 1 : j;
        const PrText t = dd_text(T, m);
        const u64 s0 = t.rec[g].hdrStart, n = pr_rec_end(t, g) - s0, at = m ? off1[g] : off0[g];
        const bool k = kept[g];
        u8 *base = k ? (m ? o1 : o0) : (m ? d1 : d0);
        if (!base) continue;
        u8 *dst = base + (k ? at : s0 - at);
        pr_copy(dst, t.buf + s0, n, sub);
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// the grid of a kernel whose waves each end in atomics on one address: few workgroups that stride, not one per 256 positions
static unsigned dd_grid_few(u64 N) { const unsigned g = bfq_grid(N, 256); return g > 2048u ? 2048u : g; }
// steps 1 and 2: G.sg / sh / start of the sorted units, every run's head its first position; d_stat[0, DD_S_NUM) preset
void bfq_dedup_sort(bfq_ctx *c, const DdTexts &T, u64 N, const bfq_dedup_opts &O, u64 *h, u64 *score, SortRec a, SortRec b, const DdGroups &G, u64 *d_stat)
{
    HIP_CHECK(hipMemsetAsync(d_stat, 0, 8 * DD_S_NUM, c->stream));
    HIP_CHECK(hipMemsetAsync(d_stat + DD_S_FIRST, 0xFF, 8, c->stream));
    if (!N) return;
    const double bytes = (double)(T.t[0].len + (T.nt == 2 ? T.t[1].len : 0));
    KLAUNCH(c, K_PAIRS_CMP, (O.keep ? 0.8 : 0.4) * bytes + 60.0 * (double)N, k_dedup_hash, bfq_grid(N, 256 / DD_LANES), 256, T, N, O.keep, O.hash_bits, (u64)O.seed,
            h, score, a);
    const SortRec sorted = bfq_radix_sort(c, a, b, N, (int)(O.hash_bits + 7) / 8);
    KLAUNCH(c, K_MISC, 69.0 * (double)N, k_dedup_sorted, bfq_grid(N, 256), 256, sorted, N, (const u64 *)h, G);
    bfq_maxscan_u64(c, G.start, G.start, N);
    KLAUNCH(c, K_MISC, 8.0 * (double)N, k_dedup_runs, dd_grid_few(N), 256, (const u64 *)G.start, N, (unsigned long long *)d_stat);
}
// step 3, one round (every round but the first takes the proposals of the one before); returns how many positions are unresolved
u64 bfq_dedup_round(bfq_ctx *c, const DdTexts &T, u64 N, const DdGroups &G, u64 *d_stat, bool first)
{
    if (!first) KLAUNCH(c, K_MISC, 16.0 * (double)N, k_dedup_advance, bfq_grid(N, 256), 256, N, G, (unsigned long long *)d_stat);
    HIP_CHECK(hipMemsetAsync(d_stat + DD_S_UNRES, 0, 8, c->stream));
    const double bytes = (double)(T.t[0].len + (T.nt == 2 ? T.t[1].len : 0));
    KLAUNCH(c, K_PAIRS_CMP, 0.4 * bytes + 48.0 * (double)N, k_dedup_round, bfq_grid(N, 256 / DD_LANES), 256, T, N, G, (unsigned long long *)d_stat);
    u64 left = 0;
    HIP_CHECK(hipMemcpyAsync(&left, d_stat + DD_S_UNRES, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    return left;
}
void bfq_dedup_first_bad(bfq_ctx *c, u64 N, const DdGroups &G, u64 *d_firstBad)
{
    KLAUNCH(c, K_MISC, 8.0 * (double)N, k_dedup_first_bad, bfq_grid(N, 256), 256, N, G, (unsigned long long *)d_firstBad);
}
// step 4: kept[g] in global order and the statistics in d_stat; gsize / best / win: N entries each (best and win: keep = 1)
void bfq_dedup_winners(bfq_ctx *c, u64 N, u32 keep, const DdGroups &G, const u64 *score, u64 *gsize, u64 *best, u64 *win, u8 *kept, u64 *d_stat)
{
    if (!N) return;
    HIP_CHECK(hipMemsetAsync(gsize, 0, 8 * N, c->stream));
    if (keep) {
        HIP_CHECK(hipMemsetAsync(best, 0, 8 * N, c->stream));
        HIP_CHECK(hipMemsetAsync(win, 0xFF, 8 * N, c->stream));
    }
    KLAUNCH(c, K_MISC, 40.0 * (double)N, k_dedup_count, bfq_grid(N, 256), 256, N, keep, G, score, (unsigned long long *)gsize, (unsigned long long *)best);
    if (keep) KLAUNCH(c, K_MISC, 40.0 * (double)N, k_dedup_win, bfq_grid(N, 256), 256, N, G, score, (const u64 *)best, (unsigned long long *)win);
    KLAUNCH(c, K_MISC, 33.0 * (double)N, k_dedup_flags, dd_grid_few(N), 256, N, keep, G, (const u64 *)gsize, (const u64 *)win, kept, (unsigned long long *)d_stat);
    KLAUNCH(c, K_MISC, 24.0 * (double)N, k_dedup_first, bfq_grid(N, 256), 256, N, G, (const u64 *)gsize, (unsigned long long *)d_stat);
}
void bfq_dedup_sizes(bfq_ctx *c, const DdTexts &T, u64 N, const u8 *kept, u64 *const sz[2])
{
    if (!N) return;
    KLAUNCH(c, K_MISC, (1.0 + 52.0 * T.nt) * (double)N, k_dedup_sizes, bfq_grid(N, 256), 256, T, N, kept, sz[0], sz[1]);
}
void bfq_dedup_move(bfq_ctx *c, const DdTexts &T, u64 N, const u8 *kept, const u64 *const off[2], u8 *const out[2], u8 *const dup[2])
{
    if (!N) return;
    const double bytes = (double)(T.t[0].len + (T.nt == 2 ? T.t[1].len : 0));
    KLAUNCH(c, K_PAIRS_MOVE, 2.0 * bytes + 53.0 * (double)T.nt * (double)N, k_dedup_move, bfq_grid((u64)T.nt * N, 16), 256, T, N, kept, off[0], off[1], out[0], out[1],
            dup[0], dup[1]);
}
