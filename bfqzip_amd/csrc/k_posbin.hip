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
// positions are counted in errInvert instead of being written anywhere.  Level 1, whose bins lie far apart, writes whole
// 64-byte chunks instead of the tile's runs (k_posbin_l1_wc below; BFQ_POSBIN_WC=0: the runs, for A/B runs).
//
// Sparse form (the default; BFQ_POSBIN_SPARSE=0: every row travels as described above).  The result is the input with edits
// applied and the input lies in device memory in the outputs' layout, so level 1 sends a row only if its final (symbol,
// quality) differs from a default k_posbin_apply works out by itself: the input, or -- M = 2, most qualities smoothed -- the
// input base with the constant quality (bfq_posbin.h; chosen on the device, no host synchronisation).  Bins and windows
// then fill partially: level 2 reads a bin's head and tail regions only and skips the tiles in the gap, k_posbin_apply starts
// from the default, lays the window's records over it and takes the terminators from the read offsets.  What is lost: bins
// are not exactly filled any more, so the check after level 1 is "sent = landed, no bin above its capacity", not "a permutation".
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

// level 1's record of a row: x = the sorted record's (w1, w2) words, rp / q = the row's edit bytes
__device__ __forceinline__ u64 pb_l1_value(u64 x, u32 rp, u32 q, int B, u64 n)
{
    const u64 pay = bfq_rec_pay((u32)x, (u32)(x >> 32));
    const u64 p = bfq_val_pos(pay);                                 // the row's suffix starts at p: its eBWT symbol is text[p - 1]
    const u32 code = rp ? bfq_base_code((u8)rp) : bfq_val_code(pay);
    if (B) q = bfq_bin8(q);
    return bfq_pack_val(p ? p - 1 : n - 1, code & 7u, q);
}

// LEVEL 1: in = the sorted records' (w1, w2) words, out = u64 records; LEVEL 2: in = level 1's records, out = u32 records.
// A tile's records into registers: v = the record, lb = its bin relative to binBase (0xFFFF: not to be written, counted in
// errInvert where it is a live row), rk = its rank among the tile's records of that bin (lcnt: zeroed, a barrier ago)
// SPARSE (level 2): the tile is slots [t0, t0 + PB_TILE) of a level-1 bin filled to head / tail: what lies in its gap is no row
template <int LEVEL, bool SPARSE>
__device__ __forceinline__ void pb_load_rank(const u64 *__restrict__ in, const u8 *__restrict__ repl, const u8 *__restrict__ editQual, int B, u64 n,
                                             u64 tbase, u64 binBase, int shiftOut, u32 *lcnt, DevCounters *cnt, u64 (&v)[PB_ITEMS],
                                             u32 (&lb)[PB_ITEMS], u32 (&rk)[PB_ITEMS], u64 cap1 = 0, u64 head = 0, u64 tail = 0, u64 t0 = 0)
{
    const u32 tid = threadIdx.x;
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
            const u64 val = LEVEL == 1 ? pb_l1_value(x[k], (rp4 >> (8 * k)) & 0xFFu, (eq4 >> (8 * k)) & 0xFFu, B, n) : x[k];
            const u64 pos = bfq_val_pos(val);
            const u64 l = (pos >> shiftOut) - binBase;            // (a bin below binBase wraps to a huge value)
            const bool live = j + k < n && (!SPARSE || bfq_posbin_live(cap1, head, tail, t0 + (j + k - tbase)));
            const bool ok = live && pos < n && l < (u64)BFQ_PB_MAX_BINS;
            if (live && !ok) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
            v[r * 4 + k] = val;
            lb[r * 4 + k] = ok ? (u32)l : 0xFFFFu;
            rk[r * 4 + k] = ok ? atomicAdd(&lcnt[l], 1u) : 0u;
        }
    }
}

// per-tile runs at the bin's cursor (level 1: BFQ_POSBIN_WC=0).  SPARSE (level 2 behind the sparse level 1): cur1 = level 1's
// cursors; a tile that lies wholly in its bin's gap is skipped without a load, and the windows fill partially -- their
// cursors hold the counts afterwards.
template <int LEVEL, bool SPARSE>
__global__ __launch_bounds__(PB_THREADS) void k_posbin_part(const u64 *__restrict__ in, const u8 *__restrict__ repl, const u8 *__restrict__ editQual,
                                                             int B, u64 n, int shiftIn, int shiftOut, u32 *__restrict__ cursor, u32 curStride,
                                                             void *__restrict__ outv, u64 ntiles, DevCounters *cnt, const u32 *__restrict__ cur1)
{
    static_assert(!SPARSE || LEVEL == 2, "level 1's sparse form is k_posbin_l1_wc");
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
        u64 cap1 = 0, head = 0, tail = 0, t0 = 0;
        if (SPARSE) {
            const u64 g1 = tbase >> shiftIn;
            cap1 = bfq_posbin_cap(n, shiftIn, g1); head = cur1[g1 * PB_CUR_STRIDE]; tail = cur1[g1 * PB_CUR_STRIDE + 1]; t0 = tbase - (g1 << shiftIn);
            if (bfq_posbin_gap_tile(cap1, head, tail, t0, PB_TILE)) continue;          // (the same for the whole workgroup)
        }
        lcnt[tid] = 0; lcnt[tid + PB_THREADS] = 0;
        __syncthreads();

        u64 v[PB_ITEMS];
        u32 lb[PB_ITEMS], rk[PB_ITEMS];
        pb_load_rank<LEVEL, SPARSE>(in, repl, editQual, B, n, tbase, binBase, shiftOut, lcnt, cnt, v, lb, rk, cap1, head, tail, t0);
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

// Level 1 in whole 64-byte chunks (the default; geometry and cursors: bfq_posbin.h).  The workgroup -- 512 threads, one per
// bin, 8 records per thread and tile -- keeps every bin's incomplete tail (below C = 8 records) in LDS from tile to tile:
// left[t * PB_LS + b] is the tail's t-th record of bin b, thread b holds its length in a register.  Per tile a bin's sequence
// is its tail followed by the tile's records in rank order; the whole chunks of it are claimed on the head cursor and written
// by groups of C consecutive lanes, the rest is the new tail.  When the workgroup is done, the tails go to the ends of their
// bins through the downward tail cursor.  The next tile's loads are issued before this tile's LDS work.
// (Level 2 keeps the runs: its windows lie close together and whole chunks gained nothing there -- DESIGN section 4.)
#define PW_THREADS 512
#define PW_ROUNDS (PB_TILE / PW_THREADS / 4)
#define PW_ITEMS (PW_ROUNDS * 4)
#define PW_C 8                                      // records per chunk (bfq_posbin_chunk(1))
#define PB_LS (BFQ_PB_MAX_BINS + 1)                 // (odd stride: a chunk's lanes read its tail records from different banks)
#define PW_MAXCHUNKS ((PB_TILE + BFQ_PB_MAX_BINS * (PW_C - 1)) / PW_C)
static_assert(BFQ_PB_MAX_BINS == PW_THREADS && PW_C * 8 == BFQ_PB_CHUNK_BYTES && PW_THREADS % PW_C == 0, "one bin per thread, a chunk by C consecutive lanes");

struct PwRaw { uint4 a[PW_ROUNDS], b[PW_ROUNDS]; u32 rp4[PW_ROUNDS], eq4[PW_ROUNDS]; };
__device__ __forceinline__ void pw_load(const u64 *__restrict__ in, const u8 *__restrict__ repl, const u8 *__restrict__ editQual, u64 n, u64 tbase, PwRaw &raw)
{
    // the arrays are padded by 16 entries and more: a vector load that starts inside them stays inside them
#pragma unroll
    for (int r = 0; r < PW_ROUNDS; r++) {
        const u64 j = tbase + (u64)(r * PW_THREADS + threadIdx.x) * 4;
        raw.a[r] = raw.b[r] = uint4{0, 0, 0, 0}; raw.rp4[r] = raw.eq4[r] = 0;
        if (j < n) { raw.a[r] = *(const uint4 *)(in + j); raw.b[r] = *(const uint4 *)(in + j + 2); raw.rp4[r] = *(const u32 *)(repl + j); raw.eq4[r] = *(const u32 *)(editQual + j); }
    }
}
// exclusive scan over the 512 threads; sh holds 8 entries; two barriers
__device__ __forceinline__ u32 pw_block_exscan32(u32 v, u32 *sh, u32 *total)
{
    const u32 lane = bfq_lane(), w = threadIdx.x >> 6;
    const u32 inc = bfq_wave_incscan32(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < PW_THREADS / 64; k++) { const u32 t = sh[k]; base += k < w ? t : 0u; tot += t; }
    *total = tot;
    __syncthreads();
    return base + inc - v;
}
__device__ __forceinline__ void pw_tail_out(const u64 *left, u32 b, u32 nl, u64 n, int shiftOut, u32 *tailCur, u64 *out, DevCounters *cnt)
{
    if (!nl) return;
    const u64 cap = bfq_posbin_cap(n, shiftOut, b);
    const u64 s = atomicAdd(tailCur, nl);
    for (u32 t = 0; t < nl; t++) {
        if (s + t < cap) out[((u64)b << shiftOut) + bfq_posbin_tail_slot(cap, s + t)] = left[t * PB_LS + b];
        else atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
    }
}

// SPARSE: the row is sent iff its final (code, quality) differs from the default at its position (bfq_posbin.h), which the row
// knows from its own payload: the eBWT symbol and its quality as the input had them
__device__ __forceinline__ bool pb_l1_send(u64 x, u64 val, int pol, int B, u32 dqConst)
{
    const u64 pay = bfq_rec_pay((u32)x, (u32)(x >> 32));
    const u32 oc = bfq_val_code(pay);
    const u32 dq = pol == BFQ_PB_CONST ? dqConst : bfq_posbin_default_qual(BFQ_PB_KEEP, B, bfq_val_qual(pay), 0u);
    return oc != 0u && (bfq_val_code(val) != oc || bfq_val_qual(val) != dq);
}

// (two workgroups per CU -- 72 KiB of LDS each -- are four waves per SIMD: 128 VGPRs)
// SPARSE: rows that match the default take no rank, no staging slot and no cursor claim, so the bins fill partially (heads
// still go up in whole chunks, tails down from the end).  Every workgroup works the polarity out for itself from the
// smoothing counter, which is final when k_cluster and k_big_* are done; workgroup 0 leaves it (+ 1) in cnt->pbPolarity for
// k_posbin_apply and the host.  The rows sent are counted, one atomic per workgroup.
template <bool SPARSE>
__global__ __launch_bounds__(PW_THREADS, 4) void k_posbin_l1_wc(const u64 *__restrict__ in, const u8 *__restrict__ repl, const u8 *__restrict__ editQual, int B, u64 n,
                                                                int shiftOut, u32 *__restrict__ cursor, u64 *__restrict__ out, u64 ntiles, DevCounters *cnt,
                                                                int M, int polForce, u32 vq, u64 bases)
{
    constexpr u32 C = PW_C;
    int pol = BFQ_PB_KEEP;
    u32 dqConst = 0;
    u64 sentWg = 0;                                 // (thread 0's copy counts)
    if (SPARSE) {
        pol = bfq_posbin_polarity(M, polForce, cnt->stats[6], bases);
        dqConst = bfq_posbin_default_qual(BFQ_PB_CONST, B, 0u, vq);
        if (blockIdx.x == 0 && threadIdx.x == 0) cnt->pbPolarity = (u64)pol + 1;
    }
    __shared__ u64 stage[PB_TILE];
    __shared__ u64 left[(C - 1) * PB_LS];
    // per bin and tile: lcnt = records; pk0 = start in the staged tile | first chunk << 16; pk1 = tail carried in | whole chunks << 16;
    // gb = what the head cursor gave; cbin = the bin of every chunk
    __shared__ u32 lcnt[BFQ_PB_MAX_BINS], pk0[BFQ_PB_MAX_BINS], pk1[BFQ_PB_MAX_BINS], gb[BFQ_PB_MAX_BINS];
    __shared__ u16 cbin[PW_MAXCHUNKS];
    __shared__ u32 sh[PW_THREADS / 64];
    const u32 tid = threadIdx.x;
    u32 *const head = cursor + (u64)tid * PB_CUR_STRIDE, *const tail = head + 1;     // bin tid's cursors: one 64-byte line
    u32 nl = 0;                                     // tail of bin tid
    PwRaw raw;
    if (blockIdx.x < ntiles) pw_load(in, repl, editQual, n, (u64)blockIdx.x * PB_TILE, raw);

    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 tbase = tile * PB_TILE;
        lcnt[tid] = 0;
        __syncthreads();

        u64 v[PW_ITEMS];
        u32 lb[PW_ITEMS], rk[PW_ITEMS];
#pragma unroll
        for (int r = 0; r < PW_ROUNDS; r++) {
            const u64 j = tbase + (u64)(r * PW_THREADS + tid) * 4;
            const uint4 a = raw.a[r], b = raw.b[r];
            const u64 x[4] = {((u64)a.y << 32) | a.x, ((u64)a.w << 32) | a.z, ((u64)b.y << 32) | b.x, ((u64)b.w << 32) | b.z};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const u64 val = pb_l1_value(x[k], (raw.rp4[r] >> (8 * k)) & 0xFFu, (raw.eq4[r] >> (8 * k)) & 0xFFu, B, n);
                const u64 pos = bfq_val_pos(val);
                const u64 l = pos >> shiftOut;
                const bool live = j + k < n;
                const bool ok = live && pos < n && l < (u64)BFQ_PB_MAX_BINS;
                if (live && !ok) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
                const bool send = ok && (!SPARSE || pb_l1_send(x[k], val, pol, B, dqConst));
                v[r * 4 + k] = val;
                lb[r * 4 + k] = send ? (u32)l : 0xFFFFu;
                rk[r * 4 + k] = send ? atomicAdd(&lcnt[l], 1u) : 0u;
            }
        }
        if (tile + gridDim.x < ntiles) pw_load(in, repl, editQual, n, (tile + gridDim.x) * PB_TILE, raw);
        __syncthreads();

        // thread b: where bin b starts in the staged tile, its whole chunks and their place in the global bin
        const u32 c = lcnt[tid];
        const u32 h = bfq_posbin_head_claim(nl, c, C), f = h / C;
        u32 totals;                                 // (records: at most 4096, chunks: fewer -- one scan for both)
        const u32 ex = pw_block_exscan32(c | (f << 16), sh, &totals);
        const u32 nchunks = totals >> 16;
        sentWg += totals & 0xFFFFu;
        pk0[tid] = ex; pk1[tid] = nl | (f << 16);
        if (f) gb[tid] = atomicAdd(head, h);
        __syncthreads();

        // every chunk has exactly one tile record that names its bin: the one that opens it or, in a chunk the tail opens, rank 0
#pragma unroll
        for (int i = 0; i < PW_ITEMS; i++) {
            if (lb[i] == 0xFFFFu) continue;
            const u32 p0 = pk0[lb[i]], p1 = pk1[lb[i]];
            stage[(p0 & 0xFFFFu) + rk[i]] = v[i];
            const u32 ci = (p1 & 0xFFFFu) + rk[i], ch = ci / C;
            if (ch < (p1 >> 16) && (ci % C == 0 || rk[i] == 0)) cbin[(p0 >> 16) + ch] = (u16)lb[i];
        }
        __syncthreads();

        for (u32 e = tid; e < nchunks * C; e += PW_THREADS) {
            const u32 ch = e / C, l = cbin[ch];
            const u32 p0 = pk0[l], carried = pk1[l] & 0xFFFFu;
            const u32 ci = (ch - (p0 >> 16)) * C + e % C;
            const u64 rec = ci < carried ? left[ci * PB_LS + l] : stage[(p0 & 0xFFFFu) + ci - carried];
            const u64 off = (u64)gb[l] + ci;
            if (off < bfq_posbin_cap(n, shiftOut, l)) out[((u64)l << shiftOut) + off] = rec;
            else atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
        }
        __syncthreads();

        // the new tail: what a bin without a whole chunk carried stays where it is, the tile's records follow it
        {
            const u32 r = bfq_posbin_tail_kept(nl, c, C);
            const u32 s0 = (ex & 0xFFFFu) + h - nl;                     // stage index of the new tail's slot 0
            for (u32 t = f ? 0u : nl; t < r; t++) left[t * PB_LS + tid] = stage[s0 + t];
            nl = r;
        }
    }
    pw_tail_out(left, tid, nl, n, shiftOut, tail, out, cnt);
    if (SPARSE && tid == 0 && sentWg) atomicAdd((unsigned long long *)&cnt->pbSent, (unsigned long long)sentWg);
}

// after level 1: head and tail regions tile every bin exactly (stores beyond a bin's capacity were dropped and counted
// where they were tried; two regions that overlap inside it show here)
// sparse (one workgroup): the bins are not exactly filled any more, so what can be told is "sent = landed, no overlap": no
// bin holds more than its capacity, and heads and tails add up to the rows level 1 counted as sent
__global__ void k_posbin_check(const u32 *__restrict__ cursor, u64 nbins, u64 n, int shift, int sparse, DevCounters *cnt)
{
    if (!sparse) {
        const u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x;
        if (b < nbins && (u64)cursor[b * PB_CUR_STRIDE] + cursor[b * PB_CUR_STRIDE + 1] != bfq_posbin_cap(n, shift, b)) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
        return;
    }
    __shared__ unsigned long long landed;
    if (threadIdx.x == 0) landed = 0;
    __syncthreads();
    u64 mine = 0;
    for (u64 b = threadIdx.x; b < nbins; b += blockDim.x) {
        const u64 ht = (u64)cursor[b * PB_CUR_STRIDE] + cursor[b * PB_CUR_STRIDE + 1];
        if (ht > bfq_posbin_cap(n, shift, b)) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
        mine += ht;
    }
    if (mine) atomicAdd(&landed, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0 && landed != cnt->pbSent) atomicAdd((unsigned long long *)&cnt->errInvert, 1ull);
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

// bytes [a, a + len) of an LDS array come from g[a, a + len), every byte through f (f4: four bytes of a word at once).  vec: g is
// 16-byte aligned -- whole pieces as one load; the ragged ends, and everything when the input is aligned otherwise than the
// output, byte by byte: no load leaves the range (the caller's arrays are exact-size)
template <class F, class F4>
__device__ __forceinline__ void pb_fill(u8 *lds, u32 a, u32 len, const u8 *g, bool vec, F f, F4 f4)
{
    const u32 end = a + len;
    if (!vec) {
        for (u32 i = a + threadIdx.x; i < end; i += PA_THREADS) lds[i] = f(g[i]);
        return;
    }
    const u32 pieces = (end + 15) >> 4;
    for (u32 k = threadIdx.x; k < pieces; k += PA_THREADS) {
        const u32 lo = k << 4;
        if (lo >= a && lo + 16 <= end) {
            uint4 x = *(const uint4 *)(g + lo);
            x.x = f4(x.x); x.y = f4(x.y); x.z = f4(x.z); x.w = f4(x.w);
            *(uint4 *)(lds + lo) = x;
        } else for (u32 i = (lo > a ? lo : a); i < lo + 16 && i < end; i++) lds[i] = f(g[i]);
    }
}
__device__ __forceinline__ u32 pb_bin8x4(u32 w) { return bfq_bin8(w & 0xFFu) | (bfq_bin8((w >> 8) & 0xFFu) << 8) | (bfq_bin8((w >> 16) & 0xFFu) << 16) | (bfq_bin8(w >> 24) << 24); }

// The sparse form of the last stage: the window's packed output range [o0, o0 + len) starts as the default -- the input's
// bases, and its qualities (KEEP) or the constant (CONST: no quality is read), binned when B = 1 -- and the window's records,
// as many as its level-2 cursor counted, are laid over it.  No record stands for a terminator any more: the window's
// terminators come from the read offsets, as a bitmap with per-word prefix counts (bfq_posbin.h; one 64-bit word per thread),
// and a record's packed slot is its window position minus the terminators before it.  A record that names a position
// outside the window, a terminator's position or no base is counted in errInvert, not followed.
// (two workgroups per CU -- 70 KiB of LDS each)
__global__ __launch_bounds__(PA_THREADS, 4) void k_posbin_apply_sparse(const u32 *__restrict__ rec, const u32 *__restrict__ wcur, u64 n, const u64 *__restrict__ roff,
                                                                    u64 N, const u8 *inSym, const u8 *inQual, int B, u32 vq, u8 *outSym, u8 *outQual, u64 nwin,
                                                                    DevCounters *cnt)
{
    __shared__ __attribute__((aligned(16))) u8 ls[BFQ_PB_W + 32];
    __shared__ __attribute__((aligned(16))) u8 lq[BFQ_PB_W + 32];
    __shared__ u64 bm[PA_THREADS];
    __shared__ u32 pre[PA_THREADS];
    __shared__ u32 sh[PA_THREADS / 64];
    __shared__ u64 shBefore;
    static_assert(PA_THREADS * 64 == BFQ_PB_W, "one bitmap word per thread");
    const u32 tid = threadIdx.x, lane = bfq_lane(), w = tid >> 6;
    const int pol = cnt->pbPolarity == (u64)BFQ_PB_CONST + 1 ? BFQ_PB_CONST : BFQ_PB_KEEP;
    const u32 dqConst = bfq_posbin_default_qual(BFQ_PB_CONST, B, 0u, vq);

    for (u64 win = blockIdx.x; win < nwin; win += gridDim.x) {
        const u64 q0 = win << BFQ_PB_WSHIFT;
        const u32 cap = (u32)bfq_posbin_cap(n, BFQ_PB_WSHIFT, win);
        if (tid == 0) shBefore = bfq_posbin_reads_before(roff, N, q0);
        bm[tid] = 0;
        __syncthreads();
        const u64 rb = shBefore;                                    // the reads from rb on end at q0 or behind it
        for (u64 i = rb + tid; i < N; i += PA_THREADS) {
            const u64 t = roff[i + 1] + i;
            if (t >= q0 + cap) break;
            const u32 d = (u32)(t - q0);
            atomicOr((unsigned long long *)&bm[d >> 6], 1ull << (d & 63u));
        }
        __syncthreads();
        const u32 mine = (u32)bfq_popc64(bm[tid]);
        const u32 inc = bfq_wave_incscan32(mine);
        if (lane == 63) sh[w] = inc;
        __syncthreads();
        u32 before = inc - mine, terms = 0;
#pragma unroll
        for (int k = 0; k < PA_THREADS / 64; k++) { const u32 t = sh[k]; before += k < (int)w ? t : 0u; terms += t; }
        pre[tid] = before;
        const u64 o0 = q0 - rb;                                     // where the window's first symbol goes
        const u32 len = cap - terms;
        const u32 bS = (u32)(((uintptr_t)outSym + o0) & 15u), bQ = (u32)(((uintptr_t)outQual + o0) & 15u);
        pb_fill(ls, bS, len, inSym + o0 - bS, (((uintptr_t)inSym + o0) & 15u) == bS, [](u8 x) { return x; }, [](u32 x) { return x; });
        if (pol == BFQ_PB_CONST) {
            const u32 c4 = dqConst * 0x01010101u;                   // (whole pieces: the slack around the range is the array's own)
            for (u32 k = tid; k < (bQ + len + 15) >> 4; k += PA_THREADS) *(uint4 *)(lq + (k << 4)) = uint4{c4, c4, c4, c4};
        } else if (B) pb_fill(lq, bQ, len, inQual + o0 - bQ, (((uintptr_t)inQual + o0) & 15u) == bQ, [](u8 x) { return (u8)bfq_bin8(x); }, [](u32 x) { return pb_bin8x4(x); });
        else pb_fill(lq, bQ, len, inQual + o0 - bQ, (((uintptr_t)inQual + o0) & 15u) == bQ, [](u8 x) { return x; }, [](u32 x) { return x; });
        __syncthreads();

        // the records over the default (the record array is padded: a vector load that starts inside it stays inside it)
        u32 nrec = wcur[win], bad = 0;
        if (nrec > cap) nrec = cap;                                 // (what went beyond was dropped and counted by level 2)
        for (u32 k = tid * 4; k < nrec; k += PA_THREADS * 4) {
            const uint4 r4 = *(const uint4 *)(rec + q0 + k);
            const u32 r[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (k + i >= nrec) break;
                const u32 idx = r[i] & (BFQ_PB_W - 1u), code = (r[i] >> BFQ_PB_WSHIFT) & 7u, q = (r[i] >> (BFQ_PB_WSHIFT + 3)) & 0xFFu;
                if (idx >= cap || code == 0u || code > 5u || bfq_posbin_is_term(bm, idx)) { bad++; continue; }
                const u32 slot = idx - bfq_posbin_term_rank(bm, pre, idx);
                ls[bS + slot] = bfq_code_sym(code); lq[bQ + slot] = (u8)q;
            }
        }
        if (bad) atomicAdd((unsigned long long *)&cnt->errInvert, (unsigned long long)bad);
        __syncthreads();
        pb_flush(ls, bS, len, outSym + o0 - bS);
        pb_flush(lq, bQ, len, outQual + o0 - bQ);
        __syncthreads();
    }
}

// workgroups of `kernel` that run at once (at most one per tile)
static unsigned pb_resident(bfq_ctx *c, const void *kernel, int threads, u64 ntiles)
{
    int perCu = 0, cus = 0;
    HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, threads, 0));
    HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const u64 g = (u64)(perCu > 0 ? perCu : 1) * (u64)(cus > 0 ? cus : 1);
    return (unsigned)(ntiles < g ? ntiles : g);
}

// the arena bytes bfq_posbins() takes beside what the caller holds (level-1 records, cursors)
size_t bfq_posbins_need(u64 n)
{
    const int s1 = bfq_posbin_shift(n);
    if (s1 < 0) return ~(size_t)0;
    return 8 * (n + 16) + 4 * (bfq_posbin_bins(n, s1) * PB_CUR_STRIDE + bfq_posbin_bins(n, BFQ_PB_WSHIFT) + 64) + 1024;
}

// w12: the sorted records' (w1, w2) words in row order (n + 16 entries) -- dead after level 1, level 2's records go there;
// repl / editQual: one byte per row (0 / the row's quality where k_cluster changed nothing); inSym / inQual: the call's inputs,
// laid out like the outputs (the sparse form's defaults; may be the outputs themselves)
void bfq_posbins(bfq_ctx *c, u64 *w12, const u8 *repl, const u8 *editQual, u64 n, const u64 *d_roff, u64 N, int B, const u8 *inSym, const u8 *inQual,
                 u8 *outSym, u8 *outQual)
{
    if (!n) return;
    const int s1 = bfq_posbin_shift(n);
    if (s1 < 0) throw BfqError{BFQ_E_ARG, "too many rows for the position bins"};
    // BFQ_POSBIN_SPARSE=0: every row travels, as before; BFQ_POSBIN_WC=0 is the dense per-tile-run path as a whole
    const bool sparse = c->env.posBinWc && c->env.posBinSparse;
    const int force = c->env.posBinPolarity;
    if (sparse && force == BFQ_PB_CONST && c->P.M != 2) throw BfqError{BFQ_E_ARG, "BFQ_POSBIN_POLARITY=const needs M = 2"};
    const size_t mk = c->mark();
    const u64 nb1 = bfq_posbin_bins(n, s1), nwin = bfq_posbin_bins(n, BFQ_PB_WSHIFT), ntiles = ceil_div(n, PB_TILE);
    u64 *rec8 = c->alloc<u64>(n + 16);
    // level 1: head and tail cursor of a bin share its 64-byte line
    u32 *cur = c->alloc<u32>(nb1 * PB_CUR_STRIDE + nwin + 64), *cur2 = cur + nb1 * PB_CUR_STRIDE;
    u32 *rec4 = (u32 *)w12;
    HIP_CHECK(hipMemsetAsync(cur, 0, 4 * (nb1 * PB_CUR_STRIDE + nwin), c->stream));
    const unsigned grid = (unsigned)(ntiles > BFQ_MAX_GRID ? BFQ_MAX_GRID : ntiles);
    const unsigned agrid = (unsigned)(nwin > BFQ_MAX_GRID ? BFQ_MAX_GRID : nwin);
    const u32 vq = (u32)c->P.v & 0xFFu;
    // The algorithmic bytes handed to the profiler stay the dense bound (36 bytes per row) in the sparse form too: how many rows
    // were sent is known on the device only, and reading it back here would cost a synchronisation.
    if (c->env.posBinWc) {
        // whole chunks are aligned when the array is: bin bases and head claims are multiples of the chunk
        if ((uintptr_t)rec8 & (BFQ_PB_CHUNK_BYTES - 1)) throw BfqError{BFQ_E_ARG, "position bins: record array not 64-byte aligned"};
        // as many workgroups as run at once: a workgroup's tails are written once, at its end
        const auto l1 = sparse ? k_posbin_l1_wc<true> : k_posbin_l1_wc<false>;
        KLAUNCH(c, K_POSBIN_L1, 18.0 * (double)n, l1, pb_resident(c, (const void *)l1, PW_THREADS, ntiles), PW_THREADS, (const u64 *)w12, repl,
                editQual, B, n, s1, cur, rec8, ntiles, c->d_cnt, c->P.M, force, vq, n - N);
        if (sparse) KLAUNCH(c, K_POSBIN_CHECK, 8.0 * (double)nb1, k_posbin_check, 1, BFQ_PB_MAX_BINS, (const u32 *)cur, nb1, n, s1, 1, c->d_cnt);
        else KLAUNCH(c, K_POSBIN_CHECK, 8.0 * (double)nb1, k_posbin_check, bfq_grid(nb1, 256), 256, (const u32 *)cur, nb1, n, s1, 0, c->d_cnt);
    } else {
        const auto l1 = k_posbin_part<1, false>;
        KLAUNCH(c, K_POSBIN_L1, 18.0 * (double)n, l1, grid, PB_THREADS, (const u64 *)w12, repl, editQual, B, n, 0, s1, cur,
                (u32)PB_CUR_STRIDE, (void *)rec8, ntiles, c->d_cnt, (const u32 *)nullptr);
    }
    const auto l2 = sparse ? k_posbin_part<2, true> : k_posbin_part<2, false>;
    KLAUNCH(c, K_POSBIN_L2, 12.0 * (double)n, l2, grid, PB_THREADS, (const u64 *)rec8, (const u8 *)nullptr, (const u8 *)nullptr, 0, n, s1,
            (int)BFQ_PB_WSHIFT, cur2, 1u, (void *)rec4, ntiles, c->d_cnt, (const u32 *)cur);
    if (sparse) KLAUNCH(c, K_POSBIN_APPLY, 4.0 * (double)n + 2.0 * (double)(n - N), k_posbin_apply_sparse, agrid, PA_THREADS, (const u32 *)rec4, (const u32 *)cur2, n,
                        d_roff, N, inSym, inQual, B, vq, outSym, outQual, nwin, c->d_cnt);
    else KLAUNCH(c, K_POSBIN_APPLY, 4.0 * (double)n + 2.0 * (double)(n - N), k_posbin_apply, agrid, PA_THREADS, (const u32 *)rec4, n, d_roff, N, outSym, outQual, nwin);
    c->release(mk);
}
