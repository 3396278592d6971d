// k_kmers.hip -- the k-mer spectrum of one or two FASTQ texts (include/bfqzip_hip.h, bfq_fastq_kmers; bfq_kmers.hip drives
// the kernels and sizes the memory; bfq_kmers.h holds the constants).
//
// The texts are on the device with their record indexes (k_fastq.hip: one FqRec per record, nothing gathered).
//
// Extraction (k_km_hist, k_km_count, k_km_emit: one walk, three uses).  A read belongs to a group of KM_GROUP = 16 lanes; a lane
// owns a stretch of KM_STARTS = 16 consecutive start positions, the group 256 per step, so a 150-base read takes one step and a
// long read as many as it needs: no lane walks a read.  The bytes of a stretch (16 + k - 1 <= 46) come from four aligned
// 16-byte loads; the loop over the 64 loaded bytes is unrolled, so every byte is taken from its register by a constant index
// and the lane's offset into them is a predicate.  Every byte shifts one 2-bit code into the forward value and one into the
// reverse complement, and counts the valid bases that end at it: the window that ends at a byte is valid when that count has
// reached k.  No window is built from scratch.
//   k_km_hist  : once per text: the valid and the skipped windows, the reads shorter than k, and the histogram over the top 12
//                bits of the k-mer in 4096 LDS counters, flushed with one 64-bit global atomic per bin that is not zero
//   k_km_count : per value range and text: the windows of every read whose k-mer lies in the range (one 32-bit count per read;
//                bfq_exscan_u32 turns them into the reads' places)
//   k_km_emit  : the same walk; the lanes of a group that emit at a byte are ranked by one ballot, so a read's records fill
//                [place, place + count) without a counter in memory.  The order inside that span is the walk's, which the sort
//                does not care about.
// A sort record (12 bytes, the suffix sort's: bfq_common.h) carries 40 bits where bfq_radix_sort() reads its digits and 56
// bits of payload.  2k <= 40: the k-mer is the key.  Above: first the lowBits = 2k - 40 low bits are the key and the top 40
// ride in the payload; k_km_rekey swaps them after the low round.  In the final layout of both
//   k-mer = key40 << lowBits | (w1 & 0xFFFFFF), source (0: A, 1: B) = bit 0 of w2.
//
// Runs of equal k-mers in the sorted records (k_km_seg_count, k_km_seg_heads).  A workgroup takes KM_SEG_CHUNK = 2048 rows, a
// thread 8 consecutive ones; a row is a head when its k-mer differs from the row's before it.  Per chunk the heads and the rows
// of B are counted, both counts are scanned, and the second kernel writes for head number j its row and the number of B rows
// before it as one 64-bit word; entry nRuns holds (n, all B rows).  A run of any length is two neighbouring entries: cA and cB
// are two subtractions by whoever handles the run (k_km_stats), however many chunks it spans, and no row of it costs an atomic.
//   k_km_stats : KM_RUN_CHUNK = 1024 runs per workgroup and step: the histograms, joint and trans in 32-bit LDS counters (a run
//                adds 1 to each; a range has less than 2^32 rows), one 64-bit global atomic per bin and workgroup at the end;
//                the scalar sums in lane registers, reduced per wave; the listed runs of each chunk counted
//   k_km_list  : (a list was asked for) the listed runs placed by the scan of those counts behind what the ranges before
//                wrote, while they lie below the cap
//   k_km_advance : n_listed += the listed runs of this range (the next range's list starts there)
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_kmers.h"

typedef unsigned long long ull;

#define KM_THREADS 256
#define KM_FLUSH_BATCHES 1000                           // batches of reads between two flushes of k_km_hist's LDS counters
static_assert((u64)KM_FLUSH_BATCHES * KM_BATCH * BFQ_MAX_READ_LEN < (1ull << 32), "32-bit LDS counters would wrap");
static_assert(KM_BATCH % (KM_THREADS / KM_GROUP) == 0 && KM_GROUP == 16 && KM_STARTS + 31 - 1 + 15 <= 64, "a stretch fits four 16-byte loads");
static_assert(KM_SEG_CHUNK == 8 * KM_THREADS && KM_RUN_CHUNK == 4 * KM_THREADS, "rows and runs per thread");
static_assert(sizeof(bfq_kmer_entry) == 16 && sizeof(FqRec) == 32, "16-byte list entries");

// The windows that start at positions [s0, s0 + n) of the sequence line at seq, n <= KM_STARTS: f(has, x) at every one of the
// 64 loaded bytes, by all lanes that came here: has = a valid window of this stretch ends at the byte, x = its k-mer.
// Returns the number of valid windows.
template <class F> __device__ __forceinline__ u32 km_stretch(const u8 *__restrict__ seq, u32 s0, u32 n, u32 k, bool canonical, F f)
{
    const uintptr_t ad = (uintptr_t)(seq + s0);
    const uint4 *__restrict__ q = (const uint4 *)(ad & ~(uintptr_t)15);
    const int mis = (int)(ad & 15);
    const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];       // (the texts are padded by 64 bytes: bfq_text_slot_bytes)
    const u32 w[16] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w, v3.x, v3.y, v3.z, v3.w};
    const int need = (int)(n + k - 1);
    const u64 mask = (1ull << (2 * k)) - 1;
    const u32 top = 2 * (k - 1);
    u64 fwd = 0, rc = 0;
    u32 run = 0, valid = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const u32 b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
        const int t = j - mis;                                    // byte t of the stretch
        const bool in = t >= 0 && t < need;
        const bool ok = b == 'A' || b == 'C' || b == 'G' || b == 'T';
        const u32 code = ((b >> 1) & 3u) ^ ((b >> 2) & 1u);       // A 0, C 1, G 2, T 3
        if (in) {
            fwd = ((fwd << 2) | code) & mask;
            rc = (rc >> 2) | ((u64)(3u - code) << top);
            run = ok ? run + 1 : 0;
        }
        const bool has = in && t >= (int)k - 1 && run >= k;
        valid += has ? 1u : 0u;
        f(has, canonical && rc < fwd ? rc : fwd);
    }
    return valid;
}

// the reads of batch bt that belong to this lane's group, their windows stretch by stretch: body(i, rec, s0, n) for every
// stretch of read i (a read shorter than k: once with n = 0, by all lanes of the group)
template <class F> __device__ __forceinline__ void km_batch(const KmText &T, u64 bt, u32 k, F body)
{
    const u32 g = threadIdx.x / KM_GROUP, gl = threadIdx.x % KM_GROUP;
    for (u32 r = g; r < KM_BATCH; r += KM_THREADS / KM_GROUP) {
        const u64 i = bt * KM_BATCH + r;
        if (i >= T.N) break;
        const FqRec rec = T.rec[i];
        if (rec.len < k) { body(i, rec, 0u, 0u); continue; }
        const u32 nw = rec.len - k + 1;
        for (u32 s0 = gl * KM_STARTS; s0 < nw; s0 += KM_GROUP * KM_STARTS) body(i, rec, s0, nw - s0 < KM_STARTS ? nw - s0 : (u32)KM_STARTS);
    }
}

__device__ __forceinline__ u64 km_wave_sum(u64 v)
{
    for (int o = 32; o; o >>= 1) v += (u64)__shfl_xor((ull)v, o);
    return v;
}

// scal[0, 3): reads shorter than k, valid windows, skipped windows
__global__ __launch_bounds__(KM_THREADS) void k_km_hist(KmText T, u32 k, u32 canonical, u64 nbatches, ull *__restrict__ hist, ull *__restrict__ scal)
{
    __shared__ u32 sh[KM_BINS];
    for (u32 t = threadIdx.x; t < KM_BINS; t += KM_THREADS) sh[t] = 0;
    __syncthreads();
    const u32 shift = 2 * k - KM_TOP_BITS;
    u64 nShort = 0, nWin = 0, nSkip = 0;                          // per lane
    u32 since = 0;
    for (u64 bt = blockIdx.x; bt < nbatches; bt += gridDim.x) {
        km_batch(T, bt, k, [&](u64, const FqRec &rec, u32 s0, u32 n) {
            if (!n) { nShort += threadIdx.x % KM_GROUP == 0 ? 1 : 0; return; }
            const u32 v = km_stretch(T.buf + rec.seqStart, s0, n, k, canonical != 0, [&](bool has, u64 x) {
                if (has) atomicAdd(&sh[(u32)(x >> shift)], 1u);
            });
            nWin += v; nSkip += n - v;
        });
        if (++since == KM_FLUSH_BATCHES) {                        // (the same for the whole workgroup)
            since = 0;
            __syncthreads();
            for (u32 t = threadIdx.x; t < KM_BINS; t += KM_THREADS) {
                const u32 v = sh[t];
                if (v) { atomicAdd(&hist[t], (ull)v); sh[t] = 0; }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < KM_BINS; t += KM_THREADS) {
        const u32 v = sh[t];
        if (v) atomicAdd(&hist[t], (ull)v);
    }
    nShort = km_wave_sum(nShort); nWin = km_wave_sum(nWin); nSkip = km_wave_sum(nSkip);
    if (bfq_lane() == 0) {
        if (nShort) atomicAdd(&scal[0], (ull)nShort);
        if (nWin) atomicAdd(&scal[1], (ull)nWin);
        if (nSkip) atomicAdd(&scal[2], (ull)nSkip);
    }
}

// cnt[i] = the windows of read i whose k-mer's bin lies in [binLo, binHi)
__global__ __launch_bounds__(KM_THREADS) void k_km_count(KmText T, u32 k, u32 canonical, u32 binLo, u32 binHi, u64 nbatches, u32 *__restrict__ cnt)
{
    const u32 shift = 2 * k - KM_TOP_BITS, gl = threadIdx.x % KM_GROUP;
    for (u64 bt = blockIdx.x; bt < nbatches; bt += gridDim.x) {
        const u32 g = threadIdx.x / KM_GROUP;
        for (u32 r = g; r < KM_BATCH; r += KM_THREADS / KM_GROUP) {
            const u64 i = bt * KM_BATCH + r;
            if (i >= T.N) break;
            const FqRec rec = T.rec[i];
            u32 mine = 0;
            if (rec.len >= k) {
                const u32 nw = rec.len - k + 1;
                for (u32 s0 = gl * KM_STARTS; s0 < nw; s0 += KM_GROUP * KM_STARTS)
                    km_stretch(T.buf + rec.seqStart, s0, nw - s0 < KM_STARTS ? nw - s0 : (u32)KM_STARTS, k, canonical != 0, [&](bool has, u64 x) {
                        const u32 bin = (u32)(x >> shift);
                        mine += has && bin >= binLo && bin < binHi ? 1u : 0u;
                    });
            }
            for (int o = KM_GROUP / 2; o; o >>= 1) mine += (u32)__shfl_xor((int)mine, o, KM_GROUP);   // (all 16 lanes are here)
            if (gl == 0) cnt[i] = mine;
        }
    }
}

// one record per window in range, read i's at [off[i], off[i] + cnt[i])
__global__ __launch_bounds__(KM_THREADS) void k_km_emit(KmText T, u32 k, u32 canonical, u32 binLo, u32 binHi, u32 lowBits, u32 src, u64 nbatches,
                                                        const u64 *__restrict__ off, u32 *__restrict__ w0, u64 *__restrict__ w12)
{
    const u32 shift = 2 * k - KM_TOP_BITS, lane = bfq_lane();
    const u64 gmask = 0xFFFFull << (lane & ~15u), below = ((1ull << lane) - 1) & gmask;
    u64 at = 0;                                                   // the next free place of the read (the same in every lane of the group that is still walking)
    u64 cur = ~0ull;
    for (u64 bt = blockIdx.x; bt < nbatches; bt += gridDim.x)
        km_batch(T, bt, k, [&](u64 i, const FqRec &rec, u32 s0, u32 n) {
            if (!n) return;
            if (i != cur) { cur = i; at = off[i]; }
            km_stretch(T.buf + rec.seqStart, s0, n, k, canonical != 0, [&](bool has, u64 x) {
                const u32 bin = (u32)(x >> shift);
                const bool emit = has && bin >= binLo && bin < binHi;
                const u64 m = __ballot(emit);                     // (lanes of the group that have left the read are not in it, and emit nothing more)
                if (emit) {
                    const u64 slot = at + (u64)__popcll(m & below);
                    u32 a;
                    u64 bc;
                    km_record(x, src, lowBits, &a, &bc);
                    w0[slot] = a;
                    w12[slot] = bc;
                }
                at += (u64)__popcll(m & gmask);
            });
        });
}

// after the low round: the top 40 bits become the key, the low bits ride in the payload
__global__ __launch_bounds__(256) void k_km_rekey(u32 *__restrict__ w0, u64 *__restrict__ w12, u64 n)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 a = w0[i];
        const u64 bc = w12[i];
        const u32 w1 = (u32)bc, w2 = (u32)(bc >> 32);
        const u64 lo = (u64)a << 8 | (w1 >> 24);
        const u64 hi40 = (u64)(w1 & 0xFFFFFFu) << 16 | (w2 >> 16);
        w0[i] = (u32)(hi40 >> 8);
        w12[i] = (u64)(w2 & 1u) << 32 | (u64)((u32)(hi40 & 0xFFu) << 24 | (u32)lo);
    }
}

// the 8 rows of a thread: bit j of *heads = row first + j starts a run, bit j of *bs = it is B's; rows at or beyond n: neither
__device__ __forceinline__ void km_rows8(const u32 *__restrict__ w0, const u64 *__restrict__ w12, u64 first, u64 n, u32 lowBits, u32 *heads, u32 *bs)
{
    u32 h = 0, b = 0;
    if (first < n) {
        u64 prev = first ? km_kmer(w0[first - 1], w12[first - 1], lowBits) : ~0ull;   // (no k-mer is all ones: 2k <= 62)
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u64 i = first + j;
            if (i < n) {
                const u64 bc = w12[i];
                const u64 x = km_kmer(w0[i], bc, lowBits);
                h |= (x != prev ? 1u : 0u) << j;
                b |= ((u32)(bc >> 32) & 1u) << j;
                prev = x;
            }
        }
    }
    *heads = h; *bs = b;
}

__global__ __launch_bounds__(KM_THREADS) void k_km_seg_count(const u32 *__restrict__ w0, const u64 *__restrict__ w12, u64 n, u32 lowBits, u64 nchunks,
                                                             u32 *__restrict__ cntH, u32 *__restrict__ cntB)
{
    __shared__ u32 sh[4];
    for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        u32 h, b, th, tb;
        km_rows8(w0, w12, ch * KM_SEG_CHUNK + 8ull * threadIdx.x, n, lowBits, &h, &b);
        bfq_block_exscan32(__popc(h), sh, &th);
        bfq_block_exscan32(__popc(b), sh, &tb);
        if (threadIdx.x == 0) { cntH[ch] = th; cntB[ch] = tb; }
    }
}

// heads[j] = row of head j | the B rows before it << 32; heads[number of heads] = n | all B rows << 32
__global__ __launch_bounds__(KM_THREADS) void k_km_seg_heads(const u32 *__restrict__ w0, const u64 *__restrict__ w12, u64 n, u32 lowBits, u64 nchunks,
                                                             const u64 *__restrict__ offH, const u64 *__restrict__ offB, u64 *__restrict__ heads)
{
    __shared__ u32 sh[4];
    for (u64 ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const u64 first = ch * KM_SEG_CHUNK + 8ull * threadIdx.x;
        u32 h, b, th, tb;
        km_rows8(w0, w12, first, n, lowBits, &h, &b);
        u64 at = offH[ch] + bfq_block_exscan32(__popc(h), sh, &th);
        u64 pb = offB[ch] + bfq_block_exscan32(__popc(b), sh, &tb);
#pragma unroll
        for (u32 j = 0; j < 8; j++) {
            const u64 i = first + j;
            if (i >= n) break;
            if (h >> j & 1u) heads[at++] = i | pb << 32;
            pb += b >> j & 1u;
            if (i == n - 1) heads[at] = n | pb << 32;
        }
    }
}

#define KM_ST_HA 0
#define KM_ST_HB 256
#define KM_ST_JOINT 512
#define KM_ST_TRANS 768
#define KM_ST_N 777
static_assert(offsetof(bfq_kmer_report, hist_b) == offsetof(bfq_kmer_report, hist_a) + 8 * KM_ST_HB &&
              offsetof(bfq_kmer_report, joint) == offsetof(bfq_kmer_report, hist_a) + 8 * KM_ST_JOINT &&
              offsetof(bfq_kmer_report, trans) == offsetof(bfq_kmer_report, hist_a) + 8 * KM_ST_TRANS &&
              offsetof(bfq_kmer_report, reserved) == offsetof(bfq_kmer_report, hist_a) + 8 * KM_ST_N,
              "the LDS counters mirror the report's arrays");

__device__ __forceinline__ void km_run_counts(const u64 *__restrict__ heads, u64 j, u32 *ca, u32 *cb)
{
    const u64 a = heads[j], b = heads[j + 1];
    const u32 len = (u32)b - (u32)a;                              // (rows and B rows below 2^32: KM_MAX_PART)
    *cb = (u32)(b >> 32) - (u32)(a >> 32);
    *ca = len - *cb;
}
__device__ __forceinline__ u32 km_class(u32 c, u32 solid) { return c == 0 ? 0u : c < solid ? 1u : 2u; }
__device__ __forceinline__ bool km_listed(u32 ca, u32 cb, u32 solid)
{
    const u32 x = km_class(ca, solid), y = km_class(cb, solid);
    return (x == 2 && y == 0) || (x == 0 && y == 2);
}

// listCnt[ch] for every ch < nchunksMax (the chunks beyond the runs: 0)
__global__ __launch_bounds__(KM_THREADS) void k_km_stats(const u64 *__restrict__ heads, const u64 *__restrict__ d_nRuns, u32 solid, u64 nchunksMax,
                                                         bfq_kmer_report *rep, u32 *__restrict__ listCnt)
{
    __shared__ u32 cnt[KM_ST_N];
    __shared__ u32 shList;
    const u64 nRuns = *d_nRuns;
    for (u32 t = threadIdx.x; t < KM_ST_N; t += KM_THREADS) cnt[t] = 0;
    if (threadIdx.x == 0) shList = 0;
    __syncthreads();
    u64 dA = 0, dB = 0, both = 0, onlyA = 0, onlyB = 0, occA = 0, occB = 0, changed = 0;   // per lane
    for (u64 ch = blockIdx.x; ch < nchunksMax; ch += gridDim.x) {
        u32 listed = 0;
#pragma unroll
        for (u32 r = 0; r < KM_RUN_CHUNK / KM_THREADS; r++) {
            const u64 j = ch * KM_RUN_CHUNK + r * KM_THREADS + threadIdx.x;
            if (j >= nRuns) continue;
            u32 ca, cb;
            km_run_counts(heads, j, &ca, &cb);
            if (ca) { dA++; atomicAdd(&cnt[KM_ST_HA + (ca < 255 ? ca : 255u)], 1u); }
            if (cb) { dB++; atomicAdd(&cnt[KM_ST_HB + (cb < 255 ? cb : 255u)], 1u); }
            atomicAdd(&cnt[KM_ST_JOINT + 16 * (ca < 15 ? ca : 15u) + (cb < 15 ? cb : 15u)], 1u);
            atomicAdd(&cnt[KM_ST_TRANS + 3 * km_class(ca, solid) + km_class(cb, solid)], 1u);
            both += ca && cb ? 1 : 0;
            if (!cb) { onlyA++; occA += ca; }
            if (!ca) { onlyB++; occB += cb; }
            changed += ca != cb ? 1 : 0;
            listed += km_listed(ca, cb, solid) ? 1u : 0u;
        }
        for (int o = 32; o; o >>= 1) listed += (u32)__shfl_xor((int)listed, o);
        if (bfq_lane() == 0 && listed) atomicAdd(&shList, listed);
        __syncthreads();
        if (threadIdx.x == 0) { listCnt[ch] = shList; shList = 0; }
        __syncthreads();
    }
    ull *dst = (ull *)rep->hist_a;
    for (u32 t = threadIdx.x; t < KM_ST_N; t += KM_THREADS)
        if (cnt[t]) atomicAdd(dst + t, (ull)cnt[t]);
    dA = km_wave_sum(dA); dB = km_wave_sum(dB); both = km_wave_sum(both); onlyA = km_wave_sum(onlyA); onlyB = km_wave_sum(onlyB);
    occA = km_wave_sum(occA); occB = km_wave_sum(occB); changed = km_wave_sum(changed);
    if (bfq_lane() == 0) {
        if (dA) atomicAdd((ull *)&rep->distinct_a, (ull)dA);
        if (dB) atomicAdd((ull *)&rep->distinct_b, (ull)dB);
        if (both) atomicAdd((ull *)&rep->distinct_both, (ull)both);
        if (onlyA) atomicAdd((ull *)&rep->only_a, (ull)onlyA);
        if (onlyB) atomicAdd((ull *)&rep->only_b, (ull)onlyB);
        if (occA) atomicAdd((ull *)&rep->occ_only_a, (ull)occA);
        if (occB) atomicAdd((ull *)&rep->occ_only_b, (ull)occB);
        if (changed) atomicAdd((ull *)&rep->distinct_changed, (ull)changed);
    }
}

// the listed runs in ascending order behind the rep->n_listed entries of the ranges before, while below cap
__global__ __launch_bounds__(KM_THREADS) void k_km_list(const u64 *__restrict__ heads, const u64 *__restrict__ d_nRuns, const u32 *__restrict__ w0,
                                                        const u64 *__restrict__ w12, u32 lowBits, u32 solid, const u64 *__restrict__ listOff,
                                                        const bfq_kmer_report *rep, u64 cap, bfq_kmer_entry *__restrict__ out)
{
    __shared__ u32 sh[4];
    const u64 nRuns = *d_nRuns, base = rep->n_listed;
    for (u64 ch = blockIdx.x; ch * KM_RUN_CHUNK < nRuns; ch += gridDim.x) {
        const u64 first = ch * KM_RUN_CHUNK + 4ull * threadIdx.x;
        u32 ca[4], cb[4], flags = 0, tot;
#pragma unroll
        for (u32 r = 0; r < 4; r++) {
            ca[r] = cb[r] = 0;
            if (first + r < nRuns) {
                km_run_counts(heads, first + r, &ca[r], &cb[r]);
                flags |= (km_listed(ca[r], cb[r], solid) ? 1u : 0u) << r;
            }
        }
        u64 at = base + listOff[ch] + bfq_block_exscan32(__popc(flags), sh, &tot);
#pragma unroll
        for (u32 r = 0; r < 4; r++)
            if (flags >> r & 1u) {
                if (at < cap) {
                    const u64 row = heads[first + r] & 0xFFFFFFFFull;
                    ulonglong2 e;
                    e.x = km_kmer(w0[row], w12[row], lowBits);
                    e.y = (ull)ca[r] | (ull)cb[r] << 32;          // count_a, count_b
                    *(ulonglong2 *)(out + at) = e;
                }
                at++;
            }
    }
}

__global__ void k_km_advance(bfq_kmer_report *rep, const u64 *__restrict__ d_listed) { rep->n_listed += *d_listed; }

// ---- launchers ------------------------------------------------------------------------------------------------------------
static unsigned km_grid(u64 items) { return (unsigned)std::min<u64>(std::max<u64>(items, 1), 2048); }   // 8 workgroups per CU; the rest by stride

void bfq_kmers_hist(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u64 bases, u64 *d_hist, u64 *d_scal)
{
    if (!T.N) return;
    const u64 nb = ceil_div(T.N, KM_BATCH);
    KLAUNCH(c, K_KM_HIST, (double)bases + 32.0 * (double)T.N, k_km_hist, km_grid(nb), KM_THREADS, T, k, canonical, nb, (ull *)d_hist, (ull *)d_scal);
}
void bfq_kmers_count(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u32 binLo, u32 binHi, u64 bases, u32 *cnt)
{
    if (!T.N) return;
    const u64 nb = ceil_div(T.N, KM_BATCH);
    KLAUNCH(c, K_KM_COUNT, (double)bases + 36.0 * (double)T.N, k_km_count, km_grid(nb), KM_THREADS, T, k, canonical, binLo, binHi, nb, cnt);
}
void bfq_kmers_emit(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u32 binLo, u32 binHi, u32 src, u64 bases, u64 records, const u64 *off, SortRec out)
{
    if (!T.N) return;
    const u64 nb = ceil_div(T.N, KM_BATCH);
    KLAUNCH(c, K_KM_EMIT, (double)bases + 40.0 * (double)T.N + 12.0 * (double)records, k_km_emit, km_grid(nb), KM_THREADS, T, k, canonical, binLo, binHi,
            km_low_bits(k), src, nb, off, out.w0, out.w12);
}
SortRec bfq_kmers_sort(bfq_ctx *c, SortRec a, SortRec b, u64 n, u32 k)
{
    const u32 low = km_low_bits(k);
    if (!low) return bfq_radix_sort(c, a, b, n, (int)(2 * k + 7) / 8);
    const SortRec r = bfq_radix_sort(c, a, b, n, (int)(low + 7) / 8);
    KLAUNCH(c, K_KM_REKEY, 24.0 * (double)n, k_km_rekey, bfq_grid(n, 256 * 8), 256, r.w0, r.w12, n);
    return bfq_radix_sort(c, r, r.w0 == a.w0 ? b : a, n, BFQ_KEY_PASSES);
}
size_t bfq_kmers_seg_bytes(u64 n)
{
    const u64 nch = ceil_div(n, KM_SEG_CHUNK), nrc = ceil_div(n, KM_RUN_CHUNK);
    return 2 * bfq_align256(4 * nch) + 2 * bfq_align256(8 * (nch + 1)) + 2 * bfq_scan_bytes(nch) + bfq_align256(4 * nrc) + bfq_align256(8 * (nrc + 1)) +
           bfq_scan_bytes(nrc) + 4 * 256;
}
// the runs of the sorted records S (n rows; `heads` has room for n + 1 words) into *d_rep; the listed ones to d_list
void bfq_kmers_runs(bfq_ctx *c, SortRec S, u64 n, u32 k, u32 solid, u64 *heads, bfq_kmer_report *d_rep, bfq_kmer_entry *d_list, u64 capList)
{
    const u32 low = km_low_bits(k);
    const u64 nch = ceil_div(n, KM_SEG_CHUNK), nrc = ceil_div(n, KM_RUN_CHUNK);
    const size_t m = c->mark();
    u32 *cntH = c->alloc<u32>(nch), *cntB = c->alloc<u32>(nch);
    u64 *offH = c->alloc<u64>(nch + 1), *offB = c->alloc<u64>(nch + 1);
    u32 *listCnt = c->alloc<u32>(nrc);
    u64 *listOff = c->alloc<u64>(nrc + 1);
    u64 *d_nRuns = c->alloc<u64>(1), *d_nB = c->alloc<u64>(1), *d_listed = c->alloc<u64>(1);
    KLAUNCH(c, K_KM_SEG, 12.0 * (double)n, k_km_seg_count, km_grid(nch), KM_THREADS, S.w0, S.w12, n, low, nch, cntH, cntB);
    bfq_exscan_u32(c, cntH, offH, nch, d_nRuns);
    bfq_exscan_u32(c, cntB, offB, nch, d_nB);
    KLAUNCH(c, K_KM_SEG, 20.0 * (double)n, k_km_seg_heads, km_grid(nch), KM_THREADS, S.w0, S.w12, n, low, nch, offH, offB, heads);
    KLAUNCH(c, K_KM_STATS, 8.0 * (double)n, k_km_stats, km_grid(nrc), KM_THREADS, heads, d_nRuns, solid, nrc, d_rep, listCnt);
    bfq_exscan_u32(c, listCnt, listOff, nrc, d_listed);
    if (capList) KLAUNCH(c, K_KM_STATS, 8.0 * (double)n, k_km_list, km_grid(nrc), KM_THREADS, heads, d_nRuns, S.w0, S.w12, low, solid, listOff, d_rep, capList, d_list);
    KLAUNCH(c, K_MISC, 16.0, k_km_advance, 1, 1, d_rep, d_listed);
    c->release(m);
}
