// partition_wc.hip -- what whole 64-byte chunks are worth to a radix partition into bins of known size (the position bins of
// k_posbin.hip, with nothing but the partition left): n 8-byte records that hold a pseudo-random permutation of [0, n)
// go into 270 bins of 2^23 positions (level 1), and level 1's output goes as 4-byte records into the 512 windows of 2^14
// positions of every bin (level 2) -- each level in two forms:
//   runs  : a 4096-record tile is ranked by bin in LDS, one atomicAdd per non-empty bin on the bin's cursor, the runs are
//           written where the cursor stands (runs of ~15 and ~8 records that begin and end anywhere in a sector)
//   chunks: the workgroup carries every bin's incomplete tail in LDS from tile to tile and writes whole aligned 64-byte
//           chunks only (8 x 8 B, 16 x 4 B; -DC2=8: 32-byte chunks at level 2); what is left at the end goes to the bins'
//           ends through a second, downward cursor.  Level 2 gives a workgroup a contiguous range of tiles.  As many
//           workgroups as run at once; the next tile's loads are issued before this tile's LDS work.
// -DTHREADS=512 runs both forms with eight waves per workgroup (8 records per thread, one bin per thread).
// Every run is checked (each slot holds a record of its bin, head + tail cursors = bin sizes) before its time is printed.
//   hipcc -O3 --offload-arch=gfx950 partition_wc.hip -o partition_wc && ./partition_wc [log2 of the bin size, default 23]
// (24: 4.53 G records, the benchmark's size; 36 + 36 + 18 GB of buffers.  Numbers: profiles/r6_posbin_sectors/README.md)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>
typedef unsigned long long u64;
typedef unsigned int u32;
typedef unsigned short u16;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

#ifndef THREADS
#define THREADS 256                                 // -DTHREADS=512: eight waves per workgroup, 8 records per thread
#endif
#define NW (THREADS / 64)
#define ITEMS (4096 / THREADS)
#define BPT (MAXB / THREADS)                        // bins a thread owns in the per-bin steps: BPT * tid + k
#define TILE (THREADS * ITEMS)
#define MAXB 512
#define LS (MAXB + 1)
#define NB1 270
#ifndef C2
#define C2 16
#endif

__device__ __forceinline__ u32 block_exscan(u32 v, u32 *sh, u32 *total)
{
    const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u32 inc = v;
    for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += t; }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    u32 base = 0, tot = 0;
#pragma unroll
    for (u32 k = 0; k < NW; k++) { const u32 t = sh[k]; base += k < w ? t : 0u; tot += t; }
    *total = tot;
    __syncthreads();
    return base + inc - v;
}

__device__ __forceinline__ u64 bin_cap(u64 n, int shift, u64 b)
{
    const u64 lo = b << shift;
    return lo >= n ? 0 : (n - lo < (1ull << shift) ? n - lo : (1ull << shift));
}

// the tile's records (load_tile), their bins relative to binBase and their ranks inside those (rank_tile)
struct Raw { uint4 a[ITEMS / 4], b[ITEMS / 4]; };
__device__ __forceinline__ void load_tile(const u64 *__restrict__ in, u64 n, u64 tbase, Raw &raw)
{
#pragma unroll
    for (int r = 0; r < ITEMS / 4; r++) {
        const u64 j = tbase + (u64)(r * THREADS + threadIdx.x) * 4;
        raw.a[r] = raw.b[r] = uint4{0, 0, 0, 0};
        if (j < n) { raw.a[r] = *(const uint4 *)(in + j); raw.b[r] = *(const uint4 *)(in + j + 2); }      // (the arrays are padded)
    }
}
__device__ __forceinline__ void rank_tile(const Raw &raw, u64 n, u64 tbase, u64 binBase, int shiftOut, u32 *lcnt, u64 (&v)[ITEMS], u32 (&lb)[ITEMS], u32 (&rk)[ITEMS])
{
#pragma unroll
    for (int r = 0; r < ITEMS / 4; r++) {
        const u64 j = tbase + (u64)(r * THREADS + threadIdx.x) * 4;
        const uint4 a = raw.a[r], b = raw.b[r];
        const u64 x[4] = {((u64)a.y << 32) | a.x, ((u64)a.w << 32) | a.z, ((u64)b.y << 32) | b.x, ((u64)b.w << 32) | b.z};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const u64 l = (x[k] >> shiftOut) - binBase;
            const bool ok = j + k < n && x[k] < n && l < (u64)MAXB;
            v[r * 4 + k] = x[k];
            lb[r * 4 + k] = ok ? (u32)l : 0xFFFFu;
            rk[r * 4 + k] = ok ? atomicAdd(&lcnt[l], 1u) : 0u;
        }
    }
}

template <int LEVEL>
__global__ __launch_bounds__(THREADS) void k_runs(const u64 *__restrict__ in, u64 n, int shiftIn, int shiftOut, u32 *__restrict__ cursor, u32 stride,
                                                  void *__restrict__ outv, u64 ntiles, u32 *err)
{
    typedef typename std::conditional<LEVEL == 1, u64, u32>::type OutT;
    __shared__ OutT stage[TILE];
    __shared__ u16 sbin[TILE];
    __shared__ u32 lcnt[MAXB], lstart[MAXB], gb[MAXB], sh[NW];
    OutT *out = (OutT *)outv;
    const u32 tid = threadIdx.x;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const u64 tbase = tile * TILE, binBase = LEVEL == 1 ? 0ull : (tbase >> shiftIn) << (shiftIn - shiftOut);
        for (u32 k = 0; k < BPT; k++) lcnt[tid + k * THREADS] = 0;
        __syncthreads();
        u64 v[ITEMS]; u32 lb[ITEMS], rk[ITEMS];
        Raw raw;
        load_tile(in, n, tbase, raw);
        rank_tile(raw, n, tbase, binBase, shiftOut, lcnt, v, lb, rk);
        __syncthreads();
        u32 c[BPT], sum = 0, total;
        for (u32 k = 0; k < BPT; k++) { c[k] = lcnt[BPT * tid + k]; sum += c[k]; }
        u32 ex = block_exscan(sum, sh, &total);
        for (u32 k = 0; k < BPT; k++) {
            const u32 b = BPT * tid + k;
            lstart[b] = ex; ex += c[k];
            if (c[k]) gb[b] = atomicAdd(&cursor[(binBase + b) * stride], c[k]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (lb[i] == 0xFFFFu) continue;
            const u32 slot = lstart[lb[i]] + rk[i];
            stage[slot] = (OutT)v[i]; sbin[slot] = (u16)lb[i];
        }
        __syncthreads();
        for (u32 i = tid; i < total; i += THREADS) {
            const u32 l = sbin[i];
            const u64 g = binBase + l, off = (u64)gb[l] + (i - lstart[l]);
            if (off < bin_cap(n, shiftOut, g)) out[(g << shiftOut) + off] = stage[i]; else atomicAdd(err, 1u);
        }
        __syncthreads();
    }
}

template <typename OutT, int C>
__device__ __forceinline__ void tails_out(const OutT *left, u32 b, u32 &nl, u64 g, u64 n, int shiftOut, u32 *tailCur, OutT *out, u32 *err)
{
    if (!nl) return;
    const u64 cap = bin_cap(n, shiftOut, g), s = atomicAdd(tailCur, nl);
    for (u32 t = 0; t < nl; t++) {
        if (s + t < cap) out[(g << shiftOut) + cap - 1 - (s + t)] = left[t * LS + b]; else atomicAdd(err, 1u);
    }
    nl = 0;
}

template <int LEVEL, int C>
__global__ __launch_bounds__(THREADS) void k_chunks(const u64 *__restrict__ in, u64 n, int shiftIn, int shiftOut, u32 *__restrict__ head, u32 *__restrict__ tail,
                                                    u32 stride, void *__restrict__ outv, u64 ntiles, u64 tilesPerWg, u32 *err)
{
    typedef typename std::conditional<LEVEL == 1, u64, u32>::type OutT;
    __shared__ OutT stage[TILE];
    __shared__ OutT left[(C - 1) * LS];
    __shared__ u32 lcnt[MAXB], pk0[MAXB], pk1[MAXB], gb[MAXB], sh[NW];
    __shared__ u16 cbin[(TILE + MAXB * (C - 1)) / C];
    OutT *out = (OutT *)outv;
    const u32 tid = threadIdx.x;
    const u64 first = LEVEL == 1 ? (u64)blockIdx.x : (u64)blockIdx.x * tilesPerWg;
    const u64 last = LEVEL == 1 ? ntiles : (first + tilesPerWg < ntiles ? first + tilesPerWg : ntiles);
    const u64 step = LEVEL == 1 ? (u64)gridDim.x : 1ull;
    u32 nl[BPT];                                    // the tails of this thread's bins
    for (u32 k = 0; k < BPT; k++) nl[k] = 0;
    u64 curBase = 0;
    Raw raw;
    if (first < last) load_tile(in, n, first * TILE, raw);
    for (u64 tile = first; tile < last; tile += step) {
        const u64 tbase = tile * TILE, binBase = LEVEL == 1 ? 0ull : (tbase >> shiftIn) << (shiftIn - shiftOut);
        if (LEVEL == 2 && binBase != curBase)
            for (u32 k = 0; k < BPT; k++) tails_out<OutT, C>(left, BPT * tid + k, nl[k], curBase + BPT * tid + k, n, shiftOut, &tail[(curBase + BPT * tid + k) * stride], out, err);
        curBase = binBase;
        for (u32 k = 0; k < BPT; k++) lcnt[tid + k * THREADS] = 0;
        __syncthreads();
        u64 v[ITEMS]; u32 lb[ITEMS], rk[ITEMS];
        rank_tile(raw, n, tbase, binBase, shiftOut, lcnt, v, lb, rk);
        if (tile + step < last) load_tile(in, n, (tile + step) * TILE, raw);        // the next tile's loads fly during this tile's LDS work
        __syncthreads();
        u32 c[BPT], h[BPT], sum = 0, totals;
        for (u32 k = 0; k < BPT; k++) { c[k] = lcnt[BPT * tid + k]; h[k] = (nl[k] + c[k]) / C * C; sum += c[k] | ((h[k] / C) << 16); }
        const u32 ex0 = block_exscan(sum, sh, &totals);
        const u32 nchunks = totals >> 16;
        u32 ex = ex0;
        for (u32 k = 0; k < BPT; k++) {
            const u32 b = BPT * tid + k;
            pk0[b] = ex; pk1[b] = nl[k] | ((h[k] / C) << 16);
            ex += c[k] | ((h[k] / C) << 16);
            if (h[k]) gb[b] = atomicAdd(&head[(binBase + b) * stride], h[k]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ITEMS; i++) {
            if (lb[i] == 0xFFFFu) continue;
            const u32 p0 = pk0[lb[i]], p1 = pk1[lb[i]];
            stage[(p0 & 0xFFFFu) + rk[i]] = (OutT)v[i];
            const u32 ci = (p1 & 0xFFFFu) + rk[i], ch = ci / C;
            if (ch < (p1 >> 16) && (ci % C == 0 || rk[i] == 0)) cbin[(p0 >> 16) + ch] = (u16)lb[i];
        }
        __syncthreads();
        for (u32 e = tid; e < nchunks * C; e += THREADS) {
            const u32 ch = e / C, l = cbin[ch];
            const u32 p0 = pk0[l], n0 = pk1[l] & 0xFFFFu;
            const u32 ci = (ch - (p0 >> 16)) * C + e % C;
            const OutT rec = ci < n0 ? left[ci * LS + l] : stage[(p0 & 0xFFFFu) + ci - n0];
            const u64 g = binBase + l, off = (u64)gb[l] + ci;
            if (off < bin_cap(n, shiftOut, g)) out[(g << shiftOut) + off] = rec; else atomicAdd(err, 1u);
        }
        __syncthreads();
        ex = ex0;
        for (u32 k = 0; k < BPT; k++) {
            const u32 b = BPT * tid + k, r = (nl[k] + c[k]) % C, s0 = (ex & 0xFFFFu) + h[k] - nl[k];
            for (u32 t = h[k] ? 0u : nl[k]; t < r; t++) left[t * LS + b] = stage[s0 + t];
            nl[k] = r;
            ex += c[k];
        }
    }
    for (u32 k = 0; k < BPT; k++) tails_out<OutT, C>(left, BPT * tid + k, nl[k], curBase + BPT * tid + k, n, shiftOut, &tail[(curBase + BPT * tid + k) * stride], out, err);
}

// in[i] = a pseudo-random permutation of [0, n): a four-round Feistel network on 2 * half bits, walked until it lands below n
__device__ __forceinline__ u64 feistel(u64 x, int half)
{
    const u32 mask = (1u << half) - 1u;
    u32 L = (u32)(x >> half), R = (u32)x & mask;
    for (u32 r = 0; r < 4; r++) {
        u32 F = R * 0x9E3779B1u + (r + 1) * 0x85EBCA6Bu;
        F ^= F >> 15; F *= 0x2C1B3C6Du; F ^= F >> 12;
        const u32 t = L ^ (F & mask);
        L = R; R = t;
    }
    return ((u64)L << half) | R;
}
__global__ void k_init(u64 *in, u64 n, int half)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        u64 x = i;
        do x = feistel(x, half); while (x >= n);
        in[i] = x;
    }
}
// every slot holds a record of its bin (level 2's records keep the low 32 bits of the position)
template <typename OutT>
__global__ void k_verify(const OutT *out, u64 n, int shift, u32 *err)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 want = i >> shift, got = sizeof(OutT) == 8 ? (u64)out[i] >> shift : (((u64)out[i] ^ i) & 0xFFFFFFFFull) >> shift;
        if (sizeof(OutT) == 8 ? got != want : got != 0) atomicAdd(err, 1u);
    }
}
__global__ void k_cursors(const u32 *head, const u32 *tail, u32 stride, u64 nbins, u64 n, int shift, u32 *err)
{
    const u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nbins && (u64)head[b * stride] + (tail ? tail[b * stride] : 0u) != bin_cap(n, shift, b)) atomicAdd(err, 1u);
}

int main(int argc, char **argv)
{
    const int s1 = argc > 1 ? atoi(argv[1]) : 23, s2 = s1 - 9;
    const u64 n = (u64)NB1 << s1, ntiles = n / TILE, nwin = n >> s2;
    u64 *in, *rec8; u32 *rec4, *cur, *err;
    CK(hipMalloc(&in, 8 * (n + 16))); CK(hipMalloc(&rec8, 8 * (n + 16))); CK(hipMalloc(&rec4, 4 * (n + 16)));
    CK(hipMalloc(&cur, 4 * (2 * nwin + 16 * NB1))); CK(hipMalloc(&err, 4));
    CK(hipMemset(err, 0, 4));
    k_init<<<1u << 16, 256>>>(in, n, (s1 + 10) / 2);               // (n < 2^(s1 + 9))
    int cus = 0, o1 = 0, o2 = 0, p1 = 0, p2 = 0;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o1, k_chunks<1, 8>, THREADS, 0));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&o2, k_chunks<2, C2>, THREADS, 0));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p1, k_runs<1>, THREADS, 0));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&p2, k_runs<2>, THREADS, 0));
    printf("n = %llu records, %d bins of 2^%d, %llu windows of 2^%d; %d CUs; workgroups per CU: runs %d / %d, chunks %d / %d (level-2 chunk: %d records)\n",
           n, NB1, s1, nwin, s2, cus, p1, p2, o1, o2, C2);
    const unsigned gridRuns = (unsigned)(ntiles > (1u << 19) ? (1u << 19) : ntiles), g1 = (unsigned)(cus * o1), g2 = (unsigned)(cus * o2);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    u32 herr = 0;
    for (int form = 0; form < 2; form++) {
        for (int level = 1; level <= 2; level++) {
            float best = 1e30f;
            for (int rep = 0; rep < 3; rep++) {
                float ms = 0;
                CK(hipMemset(cur, 0, 4 * (2 * nwin + 16 * NB1)));
                u32 *cur2 = cur + 16 * NB1;
                CK(hipEventRecord(e0));
                if (form == 0 && level == 1) k_runs<1><<<gridRuns, THREADS>>>(in, n, 0, s1, cur, 16, rec8, ntiles, err);
                if (form == 0 && level == 2) k_runs<2><<<gridRuns, THREADS>>>(rec8, n, s1, s2, cur2, 1, rec4, ntiles, err);
                if (form == 1 && level == 1) k_chunks<1, 8><<<g1, THREADS>>>(in, n, 0, s1, cur, cur + 1, 16, rec8, ntiles, 0, err);
                if (form == 1 && level == 2) k_chunks<2, C2><<<g2, THREADS>>>(rec8, n, s1, s2, cur2, cur2 + nwin, 1, rec4, ntiles, (ntiles + g2 - 1) / g2, err);
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
                if (ms < best) best = ms;
                if (level == 1) { k_verify<u64><<<1u << 16, 256>>>(rec8, n, s1, err); k_cursors<<<2, 256>>>(cur, form ? cur + 1 : nullptr, 16, NB1, n, s1, err); }
                else { k_verify<u32><<<1u << 16, 256>>>(rec4, n, s2, err); k_cursors<<<(unsigned)((nwin + 255) / 256), 256>>>(cur2, form ? cur2 + nwin : nullptr, 1, nwin, n, s2, err); }
                CK(hipMemcpy(&herr, err, 4, hipMemcpyDeviceToHost));
                if (herr) { printf("level %d, %s: %u records or cursors wrong\n", level, form ? "chunks" : "runs", herr); return 1; }
            }
            const double bytes = level == 1 ? 16.0 * n : 12.0 * n;
            printf("level %d (%d-byte records, %s), %-6s: %8.2f ms  %5.2f TB/s of %2.0f B per record\n", level, level == 1 ? 8 : 4,
                   level == 1 ? "270 bins" : "512 windows per bin", form ? "chunks" : "runs", best, bytes / best / 1e9, bytes / n);
        }
    }
    return 0;
}
