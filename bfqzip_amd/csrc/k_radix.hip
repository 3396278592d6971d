// k_radix.hip -- stable LSD radix sort of the suffix records on their 40-bit key (the first 16
// symbols, two per 5-bit group: bfq_common.h), 8-bit digits, 5 passes.
//
// This is the sort at the heart of the eBWT construction that replaces
// `gsufsort --bwt --qs` (call site BFQzip.py:184): one record per read suffix.  A record is
// 12 bytes in three 32-bit arrays (bfq_common.h): the histogram pass reads only the word that
// holds the pass's digit (4 B/row), the scatter moves 12 B/row each way.  Per pass:
//   k_radix_hist    : per-workgroup digit counts (per-wave LDS histograms)
//   exclusive scan  : digit-major table -> global offsets (k_scan.hip)
//   k_radix_scatter : wave-level match ranking (ballots), per-wave LDS digit counters +
//                     prefix across waves, then each of the three words staged through LDS
//                     in tile-sorted order and written out in coalesced runs.
// HBM-bound integer work: per pass 4 B/row (hist) + 12 B read + 12 B written.
//
// The suffix sort's first pass can GENERATE its records instead of reading them (k_radix_scatter<1, true>, KeySrc given to
// bfq_radix_sort): row i of the unsorted input is text position i, so the record is computed from the byte text and the
// packed text (2 + 0.51 B/row in) and the 12 B/row array k_build_keys would write, and this pass read back, never exists.
// Its digit counts come from k_build_keys' counting form (k_text.hip).  That pass moves about 14.5 B/row, not 24.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_keyrec.h"

#ifndef RS_THREADS
#define RS_THREADS 256
#endif
#define RS_WAVES (RS_THREADS / 64)
#define RS_OCC (1024 / RS_THREADS)                  // workgroups per CU (16 waves); 512-thread tiles measured 40 % slower
#define RS_ROUNDS 12                                // items per thread
#define RS_TILE (RS_THREADS * RS_ROUNDS)            // 3072 records per tile
#define GEN_PAD 16                                  // bytes before a tile's text in LDS (the generating pass): keeps the 16-byte stores aligned
static_assert(RS_TILE / 16 <= RS_THREADS && (RS_TILE + 20) / BFQ_SYMS_PER_WORD + 2 <= RS_THREADS, "one text load per thread and array");
static_assert(2 * (GEN_PAD + RS_TILE) + 8 * ((RS_TILE + 20) / BFQ_SYMS_PER_WORD + 2) <= 8 * RS_TILE && RS_TILE + 20 < 4096, "the tile's text fits the staging buffer");
static_assert(RS_TILE == BFQ_RS_TILE, "bfq_radix_block_elems() counts in scatter tiles");

template <class T>
__global__ __launch_bounds__(RS_THREADS) void k_radix_hist(const T *__restrict__ dw, u64 n, int shift,
                                                           u32 *__restrict__ hist, u64 nblocks, u64 blockElems)
{
    __shared__ u32 wh[RS_WAVES][256];
    u32 w = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < RS_WAVES * 256; i += RS_THREADS) (&wh[0][0])[i] = 0;
    __syncthreads();
    u64 base = (u64)blockIdx.x * blockElems;
    u64 end = base + blockElems;
    if (end > n) end = n;
    // 16 bytes per lane and load (4 or 2 records); the block base is a multiple of 4 records
    constexpr int V = 16 / sizeof(T);
    u64 i = base + (u64)threadIdx.x * V;
    for (; i + V <= end; i += (u64)RS_THREADS * V) {
        uint4 x = *(const uint4 *)(dw + i);
        if (sizeof(T) == 4) {
            atomicAdd(&wh[w][(x.x >> shift) & 255u], 1u); atomicAdd(&wh[w][(x.y >> shift) & 255u], 1u);
            atomicAdd(&wh[w][(x.z >> shift) & 255u], 1u); atomicAdd(&wh[w][(x.w >> shift) & 255u], 1u);
        } else {                                                  // digit in the low word of each u64
            atomicAdd(&wh[w][(x.x >> shift) & 255u], 1u); atomicAdd(&wh[w][(x.z >> shift) & 255u], 1u);
        }
    }
    for (; i < end; i++) {                                        // at most V-1 records of the last block
        u32 d = (u32)(dw[i] >> shift) & 255u;
        atomicAdd(&wh[w][d], 1u);
    }
    __syncthreads();
    u32 d = threadIdx.x;
    if (d < 256) {
        u32 t = 0;
#pragma unroll
        for (int k = 0; k < RS_WAVES; k++) t += wh[k][d];
        hist[(u64)d * nblocks + blockIdx.x] = t;
    }
}

// DW = which word carries the digit of this pass (0: w0, 1: w1)
// GEN = the generating first pass: row i of the input is text position i, and its record is made in registers from the
// byte text and the packed text (bfq_keyrec.h) instead of being loaded -- `in` is not read, the unsorted record array
// never exists.  Everything after the load stage is the same code, and the tile order (wave, round, lane) is the same,
// so the pass is stable on text order and writes what the streamed pass 0 writes from k_build_keys' records.
// Loads of the generating form: slot s of a tile is position tbase + s, so the tile's text is one span -- 3072 + 1 bytes each
// of T8 and Q8 (16-byte loads, one per thread and array) and the ~148 packed words its windows touch (one per thread) --
// staged in LDS, in the buffer the sorted records are staged in afterwards, and read from there row by row: 3 global
// loads per thread and tile instead of 24, and no registers held for loads in flight (per-row global loads -- a byte each
// from T8 / Q8 and two packed words -- compiled to 120 bytes of scratch at this occupancy).  Word index and symbol offset
// come from one 64-bit division per tile and a 32-bit multiply per row.
template <int DW, bool GEN>
__global__ __launch_bounds__(RS_THREADS, RS_OCC) void k_radix_scatter(SortRec in, SortRec out, u64 n, int shift,
                                                              const u64 *__restrict__ blockOff, u64 nblocks, u32 tilesPerBlock,
                                                              KeySrc src)
{
    __shared__ __attribute__((aligned(16))) u64 stage[RS_TILE];   // w0, then the (w1,w2) pair of the records (GEN: first the tile's text)
    __shared__ u8 dig[RS_TILE];             // digit of every tile-sorted slot
    __shared__ u32 wcnt[RS_WAVES][256];     // per-wave digit counters -> exclusive prefix across waves
    __shared__ u32 lstart[256];             // first tile-sorted slot of each digit
    __shared__ u64 gbase[256];              // global output cursor of each digit for this workgroup
    __shared__ u32 shscan[RS_WAVES];

    const u32 tid = threadIdx.x, lane = bfq_lane(), w = tid >> 6;
    const u64 ltmask = bfq_lanemask_lt();
    const u64 blk = blockIdx.x;
    if (tid < 256) gbase[tid] = blockOff[(u64)tid * nblocks + blk];

    for (u32 t = 0; t < tilesPerBlock; t++) {
        u64 tbase = (blk * tilesPerBlock + t) * RS_TILE;
        if (tbase >= n) break;                                   // uniform
        u32 cnt = (n - tbase < (u64)RS_TILE) ? (u32)(n - tbase) : (u32)RS_TILE;
        // GEN: the thread index is made opaque to the compiler once per tile and everything that depends on it alone (lane, wave,
        // slot numbers, LDS addresses) is derived again: otherwise all of it is kept in registers across the tiles and, with the
        // key arithmetic added, spilled
        u32 tid0 = tid;
        if (GEN) asm volatile("" : "+v"(tid0));
        const u32 ln = GEN ? (tid0 & 63u) : lane, wv = GEN ? (tid0 >> 6) : w;
        const u64 ltm = GEN ? ((1ull << ln) - 1ull) : ltmask;
        const u32 slot0 = wv * (RS_ROUNDS * 64) + ln;                // the thread's first slot in tile order

        for (int i = tid0; i < RS_WAVES * 256; i += RS_THREADS) (&wcnt[0][0])[i] = 0;
        // GEN: the tile's text goes through LDS, in the staging buffer, which is free until the ranking is done: byte GEN_PAD + j
        // of tL / qL is position tbase + j (so byte GEN_PAD - 1 is the position before the tile), wL[k] is packed word wb + k
        u8 *const tL = (u8 *)stage, *const qL = tL + GEN_PAD + RS_TILE;
        const u64 *const wL = (const u64 *)(qL + GEN_PAD + RS_TILE);
        const u64 wb = tbase / BFQ_SYMS_PER_WORD;                    // (uniform) the tile's first position: packed word, symbol offset
        const u32 ob = (u32)(tbase - wb * BFQ_SYMS_PER_WORD);
        if (GEN) {
            // 16 bytes per lane and load (tbase is a multiple of 16, the arrays are allocated in multiples of 16 bytes past n)
            if (tid0 < RS_TILE / 16 && 16 * tid0 < cnt) {
                *(uint4 *)(tL + GEN_PAD + 16 * tid0) = *(const uint4 *)(src.T8 + tbase + 16 * tid0);
                *(uint4 *)(qL + GEN_PAD + 16 * tid0) = *(const uint4 *)(src.Q8 + tbase + 16 * tid0);
            }
            if (tid0 == RS_THREADS - 1 && tbase) { tL[GEN_PAD - 1] = src.T8[tbase - 1]; qL[GEN_PAD - 1] = src.Q8[tbase - 1]; }
            // the packed words the tile's windows span: those of its positions and one more
            const u64 sb = wb / BFQ_T3_PER_SEC;
            const u32 rb = (u32)(wb - sb * BFQ_T3_PER_SEC);
            const u32 nw = bfq_div21_small(ob + cnt - 1) + 2;
            if (tid0 < nw) {
                const u32 e = rb + tid0, es = bfq_div6_small(e);     // sectors past the tile's first
                ((u64 *)wL)[tid0] = src.text3[sb * 8 + es * 8 + (e - es * BFQ_T3_PER_SEC)];
            }
        }
        __syncthreads();

        // tile order = (wave, round, lane): wave w owns slots [w*1024, w*1024+1024)
        u32 a0[RS_ROUNDS], a1[RS_ROUNDS], a2[GEN ? 1 : RS_ROUNDS];
        u32 pk[RS_ROUNDS];                                       // digit << 16 | rank, later digit << 16 | tile slot
        // unconditional loads (slots past the end of the last tile re-read its last record), padding selected afterwards:
        // all 24 loads of a lane are in flight together
        const u32 lastSlot = cnt - 1;
        if (GEN) {
#pragma unroll
            for (int r = 0; r < RS_ROUNDS; r++) {
                const u32 slot = slot0 + r * 64;
                const u32 s = slot < lastSlot ? slot : lastSlot;
                const u32 dq = bfq_div21_small(ob + s);              // packed words past the tile's first
                u64 x12;
                bfq_keyrec(wL[dq], wL[dq + 1], ob + s - dq * BFQ_SYMS_PER_WORD, tbase + s, tL[GEN_PAD - 1 + s], qL[GEN_PAD - 1 + s], &a0[r], &x12);
                a1[r] = (u32)x12;                                    // (w2 = the position's low word is made again where it is staged)
                if (slot >= cnt) { a0[r] = 0xFFFFFFFFu; a1[r] = 0xFFFFFFFFu; }   // padding, as below
                __builtin_amdgcn_sched_barrier(0);                   // one row after the other: interleaved, their intermediate values spill
            }
        } else {
#pragma unroll
            for (int r = 0; r < RS_ROUNDS; r++) {
                const u32 slot = slot0 + r * 64;
                const u64 row = tbase + (slot < lastSlot ? slot : lastSlot);
                a0[r] = in.w0[row];
                const u64 x12 = in.w12[row];
                a1[r] = (u32)x12;
                a2[r] = (u32)(x12 >> 32);
            }
        }
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; r++) {
            const u32 slot = slot0 + r * 64;
            if (!GEN && slot >= cnt) { a0[r] = 0xFFFFFFFFu; a1[r] = 0xFFFFFFFFu; a2[r] = 0u; }   // padding sorts last (digit 255, tile end)
        }
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; r++) {
            u32 d = ((DW ? a1[r] : a0[r]) >> shift) & 255u;
            u64 peers = ~0ull;
#pragma unroll
            for (int b = 0; b < 8; b++) {
                bool bit = (d >> b) & 1u;
                u64 bal = __ballot(bit);
                peers &= bit ? bal : ~bal;
            }
            u32 before = (u32)__popcll(peers & ltm);
            u32 c0 = wcnt[wv][d];
            pk[r] = (d << 16) | (c0 + before);
            bfq_wave_sync();
            if (before == 0) wcnt[wv][d] = c0 + (u32)__popcll(peers);
            bfq_wave_sync();
        }
        __syncthreads();

        // per digit (thread = digit): prefix across waves, then across digits
        u32 tot = 0;
        if (tid0 < 256) {
#pragma unroll
            for (int k = 0; k < RS_WAVES; k++) { u32 ck = wcnt[k][tid0]; wcnt[k][tid0] = tot; tot += ck; }
        }
        {                                                        // exclusive scan of tot over the workgroup
            u32 inc = GEN ? bfq_wave_incscan32_bp(tot, ln) : bfq_wave_incscan32_bp(tot);
            if (ln == 63) shscan[wv] = inc;
            __syncthreads();
            u32 base = 0;
#pragma unroll
            for (int k = 0; k < RS_WAVES; k++) base += (k < (int)wv) ? shscan[k] : 0u;
            if (tid0 < 256) lstart[tid0] = base + inc - tot;
        }
        __syncthreads();

#pragma unroll
        for (int r = 0; r < RS_ROUNDS; r++) {
            u32 d = pk[r] >> 16;
            u32 p = lstart[d] + wcnt[wv][d] + (pk[r] & 0xFFFFu);
            pk[r] = p;
            stage[p] = (u64)a0[r];
            dig[p] = (u8)d;
        }
        __syncthreads();
        u64 dst[RS_ROUNDS];
#pragma unroll
        for (int q = 0; q < RS_ROUNDS; q++) {
            u32 j = q * RS_THREADS + tid0;
            u32 d = dig[j];
            dst[q] = gbase[d] + (u64)(j - lstart[d]);
            if (j < cnt) out.w0[dst[q]] = (u32)stage[j];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RS_ROUNDS; r++) stage[pk[r]] = ((u64)(GEN ? (u32)tbase + slot0 + r * 64 : a2[r]) << 32) | a1[r];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RS_ROUNDS; q++) {
            u32 j = q * RS_THREADS + tid0;
            if (j < cnt) out.w12[dst[q]] = stage[j];
        }
        __syncthreads();
        if (tid0 < 256) gbase[tid0] += tot;
        // next iteration starts with a barrier after zeroing wcnt
    }
}

// skey digits: 0 in w1 (bits 24..31), 1..4 in w0.  The records start in `in`; `tmp` is the other ping-pong buffer.
// Returns the buffer that holds the result: `in` for an even number of passes, `tmp` for an odd one.
// gen: pass 0 generates the records of text positions 0 .. n - 1 from (T8, Q8, text3) and never reads `in`, which only
// takes its turn as a ping-pong buffer from pass 1 on (the byte text may lie there: it is dead by then); needs hist0 and n >= 2.
SortRec bfq_radix_sort(bfq_ctx *c, SortRec in, SortRec tmp, u64 n, int passes, const u32 *hist0, const KeySrc *gen)
{
    if (gen && (!hist0 || n < 2 || passes < 1)) throw BfqError{BFQ_E_ARG, "bfq_radix_sort: a generating first pass needs its counts and two rows"};
    if (n < 2) {
        if (n == 1 && (passes & 1)) {
            HIP_CHECK(hipMemcpyAsync(tmp.w0, in.w0, 4, hipMemcpyDeviceToDevice, c->stream));
            HIP_CHECK(hipMemcpyAsync(tmp.w12, in.w12, 8, hipMemcpyDeviceToDevice, c->stream));
        }
        return (passes & 1) ? tmp : in;
    }
    const u64 be = bfq_radix_block_elems(n);
    const u32 tpb = (u32)(be / RS_TILE);
    u64 nb = ceil_div(n, be);
    size_t m = c->mark();
    u32 *hist = c->alloc<u32>(256 * nb);
    u64 *off = c->alloc<u64>(256 * nb);
    SortRec out = tmp;
    for (int pass = 0; pass < passes; pass++) {
        const int dw = pass == 0 ? 1 : 0;
        const int shift = pass == 0 ? 24 : 8 * (pass - 1);
        const bool have = (pass == 0 && hist0);            // pass 0's counts were made by k_build_keys
        if (!have && dw)
            KLAUNCH(c, K_RADIX_HIST, 8.0 * (double)n, k_radix_hist<u64>, nb, RS_THREADS, (const u64 *)in.w12, n, shift, hist, nb, be);
        else if (!have)
            KLAUNCH(c, K_RADIX_HIST, 4.0 * (double)n, k_radix_hist<u32>, nb, RS_THREADS, (const u32 *)in.w0, n, shift, hist, nb, be);
        bfq_exscan_u32(c, have ? hist0 : hist, off, 256 * nb, nullptr);
        if (pass == 0 && gen)                              // 1 + 1 + 0.51 B/row of text in, 12 B/row of records out
            KLAUNCH(c, K_RADIX_SCATTER, 14.51 * (double)n, (k_radix_scatter<1, true>), nb, RS_THREADS, in, out, n, shift, (const u64 *)off, nb, tpb, *gen);
        else if (dw)
            KLAUNCH(c, K_RADIX_SCATTER, 24.0 * (double)n, (k_radix_scatter<1, false>), nb, RS_THREADS, in, out, n, shift, (const u64 *)off, nb, tpb, KeySrc{});
        else
            KLAUNCH(c, K_RADIX_SCATTER, 24.0 * (double)n, (k_radix_scatter<0, false>), nb, RS_THREADS, in, out, n, shift, (const u64 *)off, nb, tpb, KeySrc{});
        SortRec t = in; in = out; out = t;
    }
    c->release(m);
    return in;
}
