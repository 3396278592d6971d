// k_posbin.hip -- steps 3-4 of the fused path without LF table and walks: the rows go back to text order by a two-level
// radix partition on the text position every row still carries in its sort record (geometry: bfq_posbin.h).
//
//   k_posbin_l1   : row order -> level-1 bins.  Reads the record's (w1, w2) words (position, eBWT symbol, quality) and the
//                   row's two edit bytes k_cluster left (replacement symbol, smoothed quality), writes 8-byte records
//                   (position of the SYMBOL = suffix position - 1, final symbol code, final quality -- binned when B = 1).
//   k_posbin_l2   : level-1 bins -> windows of BFQ_PB_W positions, 4-byte records.
//   k_posbin_apply: one workgroup per window: the records are placed by position in two LDS byte arrays, the terminator
//                   slots are dropped (the reads go out back to back: the read index at the window's first position
//                   comes from a binary search in roff[i] + i, the terminators inside the window from the records)
//                   and the window is written out in one piece.
//
// Bin sizes are exact (every position occurs once), so there is no counting pass: a workgroup ranks a tile's records by bin
// in LDS, takes one atomicAdd per non-empty bin on the bin's global cursor and writes the runs through LDS staging.  Order
// inside a bin is free.  Every store is checked against the bin's capacity: rows that do not form a permutation of the
// positions are counted in errInvert instead of being written anywhere.
#include <type_traits>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_posbin.h"

#define PB_THREADS 256
#define PB_ROUNDS 4                                 // rounds of 4 consecutive records per thread
#define PB_ITEMS (PB_ROUNDS * 4)
#define PB_TILE (PB_THREADS * PB_ITEMS)             // 4096 records per tile: a divisor of every bin size
#define PB_CUR_STRIDE 16                            // level-1 cursors: one per 64-byte line (every tile adds to every one of them)
static_assert(BFQ_PB_W % PB_TILE == 0, "a tile lies inside one level-1 bin");
static_assert(BFQ_PB_MAX_BINS == 2 * PB_THREADS, "two bins per thread in the tile scan");

// LEVEL 1: in = the sorted records' (w1, w2) words, out = u64 records; LEVEL 2: in = level 1's records, out = u32 records
template <int LEVEL>
__global__ __launch_bounds__(PB_THREADS) void k_posbin_part(const u64 *__restrict__ in, const u8 *__restrict__ repl, const u8 *__restrict__ editQual,
                                                             int B, u64 n, int shiftIn, int shiftOut, u32 *__restrict__ cursor, u32 curStride,
                                                             void *__restrict__ outv, u64 ntiles, DevCounters *cnt)
{
    typedef typename std::conditional<LEVEL == 1, u64, u32>::type OutT;
    __shared__ OutT stage[PB_TILE];
    __shared__ u16 sbin[PB_TILE];
    __shared__ u32 lcnt[BFQ_PB_MAX_BINS], lstart[BFQ_PB_MAX_BINS], gb[BFQ_PB_MAX_BINS];
    __shared__ u32 sh[4];
    OutT *out = (OutT *)outv;
    const u32 tid = threadIdx.x;

    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 tbase = tile * PB_TILE;
        const u64 binBase = LEVEL == 1 ? 0ull : (tbase >> shiftIn) << (shiftIn - shiftOut);
        lcnt[tid] = 0; lcnt[tid + PB_THREADS] = 0;
        __syncthreads();

        u64 v[PB_ITEMS];
        u32 lb[PB_ITEMS], rk[PB_ITEMS];
        // the arrays are padded by 16 entries and more: a vector load that starts inside them stays inside them
#pragma unroll
        for (int r = 0; r < PB_ROUNDS; r++) {
            const u64 j = tbase + (u64)(r * PB_THREADS + tid) * 4;
            uint4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
            u32 rp4 = 0, eq4 = 0;
            if (j < n) {
                a = *(const uint4 *)(in + j); b = *(const uint4 *)(in + j + 2);
                if (LEVEL == 1) { rp4 = *(const u32 *)(repl + j); eq4 = *(const u32 *)(editQual + j); }
            }
            const u64 x[4] = {((u64)a.y << 32) | a.x, ((u64)a.w << 32) | a.z, ((u64)b.y << 32) | b.x, ((u64)b.w << 32) | b.z};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                u64 val = x[k];
                if (LEVEL == 1) {
                    const u64 pay = bfq_rec_pay((u32)x[k], (u32)(x[k] >> 32));
                    const u64 p = bfq_val_pos(pay);                     // the row's suffix starts at p: its eBWT symbol is text[p - 1]
                    const u32 rp = (rp4 >> (8 * k)) & 0xFFu;
                    const u32 code = rp ? bfq_base_code((u8)rp) : bfq_val_code(pay);
                    u32 q = (eq4 >> (8 * k)) & 0xFFu;
                    if (B) q = bfq_bin8(q);
                    val = bfq_pack_val(p ? p - 1 : n - 1, code & 7u, q);
                }
                const u64 pos = bfq_val_pos(val);
                const u64 l = (pos >> shiftOut) - binBase;            // (a bin below binBase wraps to a huge value)
                const bool live = j + k < n;
                const bool ok = live && pos < n && l < (u64)BFQ_PB_MAX_BINS;
                if (live && !ok) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
                v[r * 4 + k] = val;
                lb[r * 4 + k] = ok ? (u32)l : 0xFFFFu;
                rk[r * 4 + k] = ok ? atomicAdd(&lcnt[l], 1u) : 0u;
            }
        }
        __syncthreads();

        // thread t: bins 2 t and 2 t + 1 -- where they start in the staged tile, and their runs' places in the global bins
        const u32 c0 = lcnt[2 * tid], c1 = lcnt[2 * tid + 1];
        u32 total;
        const u32 ex = bfq_block_exscan32(c0 + c1, sh, &total);
        lstart[2 * tid] = ex; lstart[2 * tid + 1] = ex + c0;
        if (c0) gb[2 * tid] = atomicAdd(&cursor[(binBase + 2 * tid) * curStride], c0);
        if (c1) gb[2 * tid + 1] = atomicAdd(&cursor[(binBase + 2 * tid + 1) * curStride], c1);
        __syncthreads();

#pragma unroll
        for (int i = 0; i < PB_ITEMS; i++) {
            if (lb[i] == 0xFFFFu) continue;
            const u32 slot = lstart[lb[i]] + rk[i];
            stage[slot] = LEVEL == 1 ? (OutT)v[i] : (OutT)bfq_posbin_rec4(v[i]);
            sbin[slot] = (u16)lb[i];
        }
        __syncthreads();

        for (u32 i = tid; i < total; i += PB_THREADS) {
            const u32 l = sbin[i];
            const u64 g = binBase + l;
            const u64 off = (u64)gb[l] + (i - lstart[l]);
            if (off < bfq_posbin_cap(n, shiftOut, g)) out[(g << shiftOut) + off] = stage[i];
            else atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
        }
        __syncthreads();
    }
}

#define PA_THREADS 512
#define PA_CHUNK (BFQ_PB_W / PA_THREADS)            // 64 window positions per thread in the compaction
static_assert(PA_CHUNK == 64, "16 words per thread and array");

// bytes [a, a + len) of an LDS array go to g[a, a + len); g is 16-byte aligned: whole 16-byte pieces as one store,
// the ragged first and last piece byte by byte -- nothing outside the range is touched
__device__ __forceinline__ void pb_flush(const u8 *lds, u32 a, u32 len, u8 *g)
{
    const u32 end = a + len, pieces = (end + 15) >> 4;
    for (u32 k = threadIdx.x; k < pieces; k += PA_THREADS) {
        const u32 lo = k << 4;
        if (lo >= a && lo + 16 <= end) *(uint4 *)(g + lo) = *(const uint4 *)(lds + lo);
        else for (u32 i = (lo > a ? lo : a); i < lo + 16 && i < end; i++) g[i] = lds[i];
    }
}

// (two workgroups per CU -- 64 KiB of LDS each -- are four waves per SIMD: 128 VGPRs)
__global__ __launch_bounds__(PA_THREADS, 4) void k_posbin_apply(const u32 *__restrict__ rec, u64 n, const u64 *__restrict__ roff, u64 N,
                                                             u8 *__restrict__ outSym, u8 *__restrict__ outQual, u64 nwin)
{
    __shared__ __attribute__((aligned(16))) u8 ls[BFQ_PB_W + 32];
    __shared__ __attribute__((aligned(16))) u8 lq[BFQ_PB_W + 32];
    __shared__ u32 sh[PA_THREADS / 64];
    __shared__ u64 shBefore;
    const u32 tid = threadIdx.x, lane = bfq_lane(), w = tid >> 6;

    for (u64 win = blockIdx.x; win < nwin; win += gridDim.x) {
        const u64 q0 = win << BFQ_PB_WSHIFT;
        const u32 cnt = (u32)bfq_posbin_cap(n, BFQ_PB_WSHIFT, win);
        if (tid == 0) shBefore = bfq_posbin_reads_before(roff, N, q0);
        // placement (the record array is padded: a vector load that starts inside it stays inside it)
        for (u32 k = tid * 4; k < cnt; k += PA_THREADS * 4) {
            const uint4 r4 = *(const uint4 *)(rec + q0 + k);
            const u32 r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (k + i >= cnt) break;
                const u32 idx = r[i] & (BFQ_PB_W - 1u), code = (r[i] >> BFQ_PB_WSHIFT) & 7u, q = (r[i] >> (BFQ_PB_WSHIFT + 3)) & 0xFFu;
                if (idx >= cnt) continue;
                ls[idx] = code ? bfq_code_sym(code) : (u8)0; lq[idx] = (u8)q;
            }
        }
        __syncthreads();
        {
            // drop the terminator slots: every thread takes its 64 positions into registers, counts its terminators, and
            // after the scan (whose barriers separate all reads from all writes) puts its symbols back, moved down
            u32 s[PA_CHUNK / 4], q[PA_CHUNK / 4];
            const u32 c0 = tid * PA_CHUNK;
            u32 mine = 0;
#pragma unroll
            for (int i = 0; i < PA_CHUNK / 4; i++) {
                s[i] = *(const u32 *)(ls + c0 + 4 * i); q[i] = *(const u32 *)(lq + c0 + 4 * i);
#pragma unroll
                for (int b = 0; b < 4; b++) mine += (c0 + 4 * i + b < cnt && ((s[i] >> (8 * b)) & 0xFFu) == 0u) ? 1u : 0u;
            }
            const u32 inc = bfq_wave_incscan32(mine);
            if (lane == 63) sh[w] = inc;
            __syncthreads();
            u32 before = inc - mine, terms = 0;
#pragma unroll
            for (int k = 0; k < PA_THREADS / 64; k++) { const u32 t = sh[k]; before += k < (int)w ? t : 0u; terms += t; }
            const u64 o0 = q0 - shBefore;                           // where the window's first symbol goes
            const u32 len = cnt - terms;
            const u32 bS = (u32)(((uintptr_t)outSym + o0) & 15u), bQ = (u32)(((uintptr_t)outQual + o0) & 15u);
            __syncthreads();
            u32 pos = c0 - before;
#pragma unroll
            for (int i = 0; i < PA_CHUNK / 4; i++) {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const u32 sy = (s[i] >> (8 * b)) & 0xFFu;
                    if (c0 + 4 * i + b < cnt && sy) { ls[bS + pos] = (u8)sy; lq[bQ + pos] = (u8)(q[i] >> (8 * b)); pos++; }
                }
            }
            __syncthreads();
            pb_flush(ls, bS, len, outSym + o0 - bS);
            pb_flush(lq, bQ, len, outQual + o0 - bQ);
        }
        __syncthreads();
    }
}

// the arena bytes bfq_posbins() takes beside what the caller holds (level-1 records, cursors)
size_t bfq_posbins_need(u64 n)
{
    const int s1 = bfq_posbin_shift(n);
    if (s1 < 0) return ~(size_t)0;
    return 8 * (n + 16) + 4 * (bfq_posbin_bins(n, s1) * PB_CUR_STRIDE + bfq_posbin_bins(n, BFQ_PB_WSHIFT) + 64) + 1024;
}

// w12: the sorted records' (w1, w2) words in row order (n + 16 entries) -- dead after level 1, level 2's records go there;
// repl / editQual: one byte per row (0 / the row's quality where k_cluster changed nothing)
void bfq_posbins(bfq_ctx *c, u64 *w12, const u8 *repl, const u8 *editQual, u64 n, const u64 *d_roff, u64 N, int B, u8 *outSym, u8 *outQual)
{
    if (!n) return;
    const int s1 = bfq_posbin_shift(n);
    if (s1 < 0) throw BfqError{BFQ_E_ARG, "too many rows for the position bins"};
    const size_t mk = c->mark();
    const u64 nb1 = bfq_posbin_bins(n, s1), nwin = bfq_posbin_bins(n, BFQ_PB_WSHIFT), ntiles = ceil_div(n, PB_TILE);
    u64 *rec8 = c->alloc<u64>(n + 16);
    u32 *cur = c->alloc<u32>(nb1 * PB_CUR_STRIDE + nwin + 64), *cur2 = cur + nb1 * PB_CUR_STRIDE;
    u32 *rec4 = (u32 *)w12;
    HIP_CHECK(hipMemsetAsync(cur, 0, 4 * (nb1 * PB_CUR_STRIDE + nwin), c->stream));
    const unsigned grid = (unsigned)(ntiles > BFQ_MAX_GRID ? BFQ_MAX_GRID : ntiles);
    KLAUNCH(c, K_POSBIN_L1, 18.0 * (double)n, k_posbin_part<1>, grid, PB_THREADS, (const u64 *)w12, repl, editQual, B, n, 0, s1, cur,
            (u32)PB_CUR_STRIDE, (void *)rec8, ntiles, c->d_cnt);
    KLAUNCH(c, K_POSBIN_L2, 12.0 * (double)n, k_posbin_part<2>, grid, PB_THREADS, (const u64 *)rec8, (const u8 *)nullptr, (const u8 *)nullptr, 0, n, s1,
            (int)BFQ_PB_WSHIFT, cur2, 1u, (void *)rec4, ntiles, c->d_cnt);
    const unsigned agrid = (unsigned)(nwin > BFQ_MAX_GRID ? BFQ_MAX_GRID : nwin);
    KLAUNCH(c, K_POSBIN_APPLY, 4.0 * (double)n + 2.0 * (double)(n - N), k_posbin_apply, agrid, PA_THREADS, (const u32 *)rec4, n, d_roff, N, outSym, outQual, nwin);
    c->release(mk);
}
