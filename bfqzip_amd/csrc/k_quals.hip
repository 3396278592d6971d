// k_quals.hip -- the BFQQUAL1 container: read-order quality lines (OUT.fq.qs) coded by their place in the read.  Opt-in
// (bfq_quals_compress, bfq_fastq_job.qual_codec, parallel.py --quals, `bsc q`); include/bfqzip_hip.h states the format,
// tests/quals_model.py states it again in Python, and this file produces the same bytes.
//
// Why a container of its own: BFQRANS2 sees the k bytes in front of a value inside an arbitrary 8192-byte segment.  What
// dedicated quality coders condition on -- where in the read the value stands, how noisy the read has been so far, a coarse
// view of the values two and three places back -- is computed per read with no dependency between reads, so the project's
// shape stays: a static model counted on a sample, stored rows, one rANS stream per segment, one lane per segment.
//
//   k_ql_present   which byte values occur                       k_ql_lens      line lengths and the longest line
//   k_ql_segfirst  first read of every 1024-value window (the rule of BFQDNAC1)
//   k_ql_count     a lane per sampled segment walks its reads forwards: (context at the highest rung, rank) pairs into the
//                  table through a per-workgroup LDS cache of the hot pairs (exact sums)
//   host           the rung (choose_order's estimator over the nested rungs), the rows normalised to 2^12
//   k_ql_encode    a lane per segment, last value to first.  delta is a forward prefix: on entering a read from its end the
//                  lane sums the read's |differences| forwards with 8-byte loads, then walks back subtracting
//   k_ql_pack      the segments' streams closed up behind the header (a wavefront per segment)
//   k_ql_decode    a lane per segment, forwards; a row of cumulative u16 padded to a multiple of 8 entries arrives in 16-byte
//                  loads and the symbol is the number of entries <= slot, counted in registers
//   k_ql_newlines  the line ends, from lens
#include <vector>
#include <functional>
#include <string.h>
#include "bfq_internal.h"
#include "bfq_device.h"

#define QL_S 1024u
#define QL_SCALE 12u
#define QL_L (1u << 23)
#define QL_HDR 72u
#define QL_MAXLINE 65535u
#define QL_MAX_TABLE (1u << 22)
#define QL_CACHE 4096u
#define QL_NOFIT (~0ull)

// log2 of (M, P, D, E) at rung 0..3
static const u32 ql_rung[4][4] = {{0, 0, 0, 0}, {2, 2, 1, 0}, {3, 3, 2, 0}, {3, 4, 2, 1}};
struct QlPar { u32 A, lM, lP, lD, lE, W; };
static QlPar ql_par(u32 A, u32 rung, u32 maxlen)
{
    const u32 W = (maxlen + 15u) / 16u;
    return QlPar{A, ql_rung[rung][0], ql_rung[rung][1], ql_rung[rung][2], ql_rung[rung][3], W ? W : 1u};
}
static u64 ql_rows(u32 rung, u32 A) { return (u64)A << (ql_rung[rung][0] + ql_rung[rung][1] + ql_rung[rung][2] + ql_rung[rung][3]); }
static u32 ql_sample_step(u64 nvals) { const u64 s = nvals >> 24; return s < 1 ? 1u : s > 64 ? 64u : (u32)s; }
static void ql_put32(u8 *p, u32 v) { p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24); }
static void ql_put64(u8 *p, u64 v) { ql_put32(p, (u32)v); ql_put32(p + 4, (u32)(v >> 32)); }
static u32 ql_get32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }
static u64 ql_get64(const u8 *p) { return (u64)ql_get32(p) | ((u64)ql_get32(p + 4) << 32); }

// the row of a value: q1 the rank before it, m8 = max(q2, q3) 8 / A, e = (q2 == q3), p16 = min(15, j / W), delta = the sum
// of the read's |differences| in front of q1
__host__ __device__ static inline u32 ql_ctx(const QlPar &P, u32 q1, u32 m8, u32 e, u32 p16, u32 delta)
{
    const u32 d4 = (delta >= 8u ? 1u : 0u) + (delta >= 32u ? 1u : 0u) + (delta >= 128u ? 1u : 0u);
    const u32 m = m8 >> (3u - P.lM), p = p16 >> (4u - P.lP), d = d4 >> (2u - P.lD), ee = P.lE ? e : 0u;
    return ((((((p << P.lD) | d) << P.lE) | ee) << P.lM) | m) * P.A + q1;
}
__device__ __forceinline__ u32 ql_absdiff(u32 a, u32 b) { return a > b ? a - b : b - a; }
// eight bytes at p, of which `avail` exist (the last read of a stream ends at the buffer's end)
__device__ __forceinline__ u64 ql_load8(const u8 *p, u64 avail)
{
    u64 w = 0;
    if (avail >= 8) __builtin_memcpy(&w, p, 8);
    else for (u32 t = 0; t < (u32)avail; t++) w |= (u64)p[t] << (8u * t);
    return w;
}

__global__ __launch_bounds__(256) void k_ql_present(const u8 *__restrict__ in, u64 n, u32 *__restrict__ present)
{
    __shared__ u32 sh[256];
    sh[threadIdx.x] = 0;
    __syncthreads();
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) sh[in[i]] = 1;
    __syncthreads();
    if (sh[threadIdx.x]) present[threadIdx.x] = 1;
}
__global__ __launch_bounds__(256) void k_ql_lens(const u64 *__restrict__ lineEnd, u64 nreads, u32 *__restrict__ lens, u32 *__restrict__ maxlen)
{
    __shared__ u32 smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    u32 mx = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nreads; i += (u64)gridDim.x * blockDim.x) {
        const u64 s = i ? lineEnd[i - 1] + 1 : 0, len = lineEnd[i] - s;
        const u32 l = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)len;
        lens[i] = l;
        mx = l > mx ? l : mx;
    }
    if (mx) atomicMax(&smax, mx);
    __syncthreads();
    if (threadIdx.x == 0 && smax) atomicMax(maxlen, smax);
}
__global__ __launch_bounds__(256) void k_ql_lenmax(const u32 *__restrict__ lens, u64 nreads, u32 *__restrict__ maxlen)
{
    __shared__ u32 smax;
    if (threadIdx.x == 0) smax = 0;
    __syncthreads();
    u32 mx = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nreads; i += (u64)gridDim.x * blockDim.x) mx = lens[i] > mx ? lens[i] : mx;
    if (mx) atomicMax(&smax, mx);
    __syncthreads();
    if (threadIdx.x == 0 && smax) atomicMax(maxlen, smax);
}
// segFirst[g], g = 0..nseg: the first read whose first value has an index >= g S (nreads when there is none)
__global__ __launch_bounds__(256) void k_ql_segfirst(const u64 *__restrict__ boff, u64 nreads, u64 nseg, u64 *__restrict__ segFirst)
{
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g <= nseg; g += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = nreads;
        const u64 want = g * QL_S;
        while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (boff[mid] >= want) hi = mid; else lo = mid + 1; }
        segFirst[g] = lo;
    }
}

struct QlIn {
    const u8 *in;           // the raw stream: value j of read r is in[boff[r] + r + j]
    u64 n;
    const u64 *boff;        // [nreads + 1]
    const u64 *segFirst;    // [nseg + 1]
    u64 nseg;
};

// the direct-mapped LDS cache of k_cdc_count: the first pair to claim a slot counts there, everything else in the table
__device__ __forceinline__ void ql_add(u32 *tag, u32 *cnt, u32 *__restrict__ gcnt, u32 key, u32 v)
{
    const u32 slot = key & (QL_CACHE - 1u);
    u32 t = tag[slot];
    if (t == 0xFFFFFFFFu) { const u32 old = atomicCAS(&tag[slot], 0xFFFFFFFFu, key); t = (old == 0xFFFFFFFFu) ? key : old; }
    if (t == key) atomicAdd(&cnt[slot], v);
    else atomicAdd(&gcnt[key], v);
}
__global__ __launch_bounds__(256) void k_ql_count(QlIn I, const u8 *__restrict__ map, QlPar P, u32 step, u32 *__restrict__ cnt)
{
    __shared__ u8 smap[256], m8tab[64];
    __shared__ u32 ctag[QL_CACHE], ccnt[QL_CACHE];
    for (u32 t = threadIdx.x; t < 256; t += blockDim.x) smap[t] = map[t];
    for (u32 t = threadIdx.x; t < 64; t += blockDim.x) m8tab[t] = (u8)(t * 8u / P.A > 7u ? 7u : t * 8u / P.A);
    for (u32 j = threadIdx.x; j < QL_CACHE; j += blockDim.x) { ctag[j] = 0xFFFFFFFFu; ccnt[j] = 0; }
    __syncthreads();
    for (u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) * step; g < I.nseg; g += (u64)gridDim.x * blockDim.x * step) {
        const u64 ra = I.segFirst[g], rb = I.segFirst[g + 1];
        u32 lastKey = 0xFFFFFFFFu, run = 0;
        for (u64 r = ra; r < rb; r++) {
            const u64 rs = I.boff[r];
            const u32 l = (u32)(I.boff[r + 1] - rs);
            const u8 *src = I.in + rs + r;
            const u64 lim = I.n - (rs + r);
            u32 q1 = 0, q2 = 0, q3 = 0, delta = 0, pj = 0, rem = 0;
            for (u32 c0 = 0; c0 < l; c0 += 8) {
                const u64 w = ql_load8(src + c0, lim - c0);
#pragma unroll
                for (u32 u = 0; u < 8; u++) {
                    if (c0 + u < l) {
                        const u32 s = smap[(u8)(w >> (8u * u))];
                        const u32 key = ql_ctx(P, q1, m8tab[q2 > q3 ? q2 : q3], q2 == q3 ? 1u : 0u, pj, delta) * P.A + s;
                        if (key == lastKey) run++;
                        else { if (run) ql_add(ctag, ccnt, cnt, lastKey, run); lastKey = key; run = 1; }
                        if (c0 + u) delta += ql_absdiff(s, q1);
                        q3 = q2; q2 = q1; q1 = s;
                        if (++rem == P.W) { rem = 0; pj = pj < 15u ? pj + 1u : 15u; }
                    }
                }
            }
        }
        if (run) ql_add(ctag, ccnt, cnt, lastKey, run);
    }
    __syncthreads();
    for (u32 j = threadIdx.x; j < QL_CACHE; j += blockDim.x)
        if (ccnt[j]) atomicAdd(&cnt[ctag[j]], ccnt[j]);
}

// rank of value idx of the read whose bytes [c0, c0 + 8) are `hi` and [c0 - 8, c0) are `lo` (c0 - 8 <= idx < c0 + 8)
__device__ __forceinline__ u32 ql_at(const u8 *smap, u64 hi, u64 lo, u32 c0, u32 idx)
{
    return idx >= c0 ? smap[(u8)(hi >> (8u * (idx - c0)))] : smap[(u8)(lo >> (8u * (idx + 8u - c0)))];
}
// scratch: the stream of segment g ends at byte 2 (values up to and including g's) + 16 (g + 1): two bytes per value (a value
// costs at most 12 bits) and 16 per segment, so no two segments' slots meet
__device__ __forceinline__ u64 ql_slot_end(u64 valsEnd, u64 g) { return 2ull * valsEnd + 16ull * (g + 1ull); }

// One lane per segment, last value to first.  fc[row * A + rank] = frequency | cumulative << 16; emitted bytes are collected
// eight at a time towards lower addresses of the lane's slot.
__global__ __launch_bounds__(256) void k_ql_encode(QlIn I, const u8 *__restrict__ map, QlPar P, const u32 *__restrict__ fc,
                                                   u8 *__restrict__ scratch, u32 *__restrict__ segBytes)
{
    __shared__ u8 smap[256], m8tab[64];
    for (u32 t = threadIdx.x; t < 256; t += blockDim.x) smap[t] = map[t];
    for (u32 t = threadIdx.x; t < 64; t += blockDim.x) m8tab[t] = (u8)(t * 8u / P.A > 7u ? 7u : t * 8u / P.A);
    __syncthreads();
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < I.nseg; g += (u64)gridDim.x * blockDim.x) {
        const u64 ra = I.segFirst[g], rb = I.segFirst[g + 1];
        const u64 b1 = I.boff[rb];
        if (b1 == I.boff[ra]) { segBytes[g] = 0; continue; }
        u8 *const slotEnd = scratch + ql_slot_end(b1, g);
        u8 *q = slotEnd;
        u64 acc = 0;
        u32 nacc = 0, x = QL_L;
        for (u64 r = rb; r-- > ra;) {
            const u64 rs = I.boff[r];
            const u32 l = (u32)(I.boff[r + 1] - rs);
            if (!l) continue;
            const u8 *src = I.in + rs + r;
            const u64 lim = I.n - (rs + r);
            u32 D = 0;                                             // the read's sum of |differences|, forwards
            {
                u32 pr = 0;
                for (u32 c = 0; c < l; c += 8) {
                    const u64 w = ql_load8(src + c, lim - c);
#pragma unroll
                    for (u32 u = 0; u < 8; u++)
                        if (c + u < l) { const u32 s = smap[(u8)(w >> (8u * u))]; if (c + u) D += ql_absdiff(s, pr); pr = s; }
                }
            }
            u32 c0 = (l - 1u) & ~7u;
            u64 hi = ql_load8(src + c0, lim - c0), lo = c0 ? ql_load8(src + c0 - 8, 8) : 0ull;
            const u32 jl = l - 1u;
            u32 s0 = ql_at(smap, hi, lo, c0, jl);
            u32 s1 = jl >= 1u ? ql_at(smap, hi, lo, c0, jl - 1u) : 0u;
            u32 s2 = jl >= 2u ? ql_at(smap, hi, lo, c0, jl - 2u) : 0u;
            u32 s3 = jl >= 3u ? ql_at(smap, hi, lo, c0, jl - 3u) : 0u;
            u32 delta = D - (jl >= 1u ? ql_absdiff(s0, s1) : 0u);  // the differences in front of q1
            u32 pq = jl / P.W, rem = jl - pq * P.W;
            for (;;) {
#pragma unroll
                for (int u = 7; u >= 0; u--) {
                    const u32 j = c0 + (u32)u;
                    if (j < l) {
                        const u32 row = ql_ctx(P, s1, m8tab[s2 > s3 ? s2 : s3], s2 == s3 ? 1u : 0u, pq < 15u ? pq : 15u, delta);
                        const u32 t = fc[(u64)row * P.A + s0];
                        const u32 f = t & 0xFFFFu, cm = t >> 16;
                        const u32 xmax = ((QL_L >> QL_SCALE) << 8) * f;
                        while (x >= xmax) {
                            acc = (acc << 8) | (x & 0xFFu); x >>= 8;
                            if (++nacc == 8) { q -= 8; __builtin_memcpy(q, &acc, 8); nacc = 0; }
                        }
                        const u32 dv = x / f;
                        x = (dv << QL_SCALE) + (x - dv * f) + cm;
                        // the window one place down
                        if (j >= 2u) delta -= ql_absdiff(s1, s2);
                        s0 = s1; s1 = s2; s2 = s3;
                        const u64 wsrc = u >= 4 ? hi : lo;                  // value j - 4: four places down the 16-byte window
                        const u32 wsh = 8u * (u32)(u >= 4 ? u - 4 : u + 4);
                        s3 = j >= 4u ? smap[(u8)(wsrc >> wsh)] : 0u;
                        if (rem == 0) { pq--; rem = P.W - 1u; } else rem--;
                    }
                }
                if (c0 == 0) break;
                c0 -= 8; hi = lo; lo = c0 ? ql_load8(src + c0 - 8, 8) : 0ull;
            }
        }
        while (nacc) { nacc--; *--q = (u8)(acc >> (8u * nacc)); }   // the oldest of the pending bytes first
        q -= 4;
        q[0] = (u8)x; q[1] = (u8)(x >> 8); q[2] = (u8)(x >> 16); q[3] = (u8)(x >> 24);
        segBytes[g] = (u32)(slotEnd - q);
    }
}
// one wavefront per segment: its stream from the end of its scratch slot to its place in the payload; bytes beyond `cap` are
// not written (the host sees the total)
__global__ __launch_bounds__(256) void k_ql_pack(QlIn I, const u8 *__restrict__ scratch, const u32 *__restrict__ segBytes,
                                                 const u64 *__restrict__ off, u8 *__restrict__ out, u64 cap)
{
    const u32 lane = bfq_lane();
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; g < I.nseg; g += nwaves) {
        const u32 bytes = segBytes[g];
        if (!bytes) continue;
        const u8 *src = scratch + ql_slot_end(I.boff[I.segFirst[g + 1]], g) - bytes;
        const u64 o = off[g];
        for (u32 j = lane; j < bytes; j += 64) if (o + j < cap) out[o + j] = src[j];
    }
}

// One lane per segment, forwards.  cum: rows of `nld` 16-byte groups of cumulative frequencies, padded with 2^12 (no slot
// reaches it): the symbol is the number of entries <= slot, less one; its share ends at the smallest entry above the slot.
// Every payload byte read lies inside the segment's share, every value written inside its read.
__global__ __launch_bounds__(256) void k_ql_decode(QlIn I, const u8 *__restrict__ pay, const u64 *__restrict__ off, const u32 *__restrict__ segBytes,
                                                   const u8 *__restrict__ alphabet, QlPar P, const u16 *__restrict__ cum, u32 nld,
                                                   u8 *__restrict__ out, u32 *__restrict__ bad)
{
    __shared__ u8 salpha[64], m8tab[64];
    for (u32 t = threadIdx.x; t < 64; t += blockDim.x) {
        salpha[t] = alphabet[t];
        m8tab[t] = (u8)(t * 8u / P.A > 7u ? 7u : t * 8u / P.A);
    }
    __syncthreads();
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < I.nseg; g += (u64)gridDim.x * blockDim.x) {
        const u64 ra = I.segFirst[g], rb = I.segFirst[g + 1];
        const u32 nbytes = segBytes[g];
        if (I.boff[rb] == I.boff[ra]) { if (nbytes) atomicAdd(bad, 1u); continue; }
        if (nbytes < 4) { atomicAdd(bad, 1u); continue; }
        const u8 *q = pay + off[g];
        u32 x = (u32)q[0] | ((u32)q[1] << 8) | ((u32)q[2] << 16) | ((u32)q[3] << 24);
        if (x < QL_L) { atomicAdd(bad, 1u); continue; }             // an encoder's final state is never below the renormalisation bound
        u32 used = 4, ni = 0;
        u64 ib = 0;
        bool ok = true;
        for (u64 r = ra; r < rb && ok; r++) {
            const u64 rs = I.boff[r];
            const u32 l = (u32)(I.boff[r + 1] - rs);
            u8 *dst = out + rs + r;
            u32 q1 = 0, q2 = 0, q3 = 0, delta = 0, pj = 0, rem = 0;
            for (u32 j = 0; j < l; j++) {
                const u32 row = ql_ctx(P, q1, m8tab[q2 > q3 ? q2 : q3], q2 == q3 ? 1u : 0u, pj, delta);
                const uint4 *rp = (const uint4 *)(cum + (u64)row * (8u * nld));
                const u32 slot = x & ((1u << QL_SCALE) - 1u);
                u32 cnt = 0, c0 = 0, nx = 1u << QL_SCALE;
                for (u32 k = 0; k < nld; k++) {
                    const uint4 v = rp[k];
                    const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int t = 0; t < 8; t++) {
                        const u32 en = (t & 1) ? w[t >> 1] >> 16 : w[t >> 1] & 0xFFFFu;
                        const bool le = en <= slot;
                        cnt += le ? 1u : 0u;
                        c0 = le && en > c0 ? en : c0;
                        nx = !le && en < nx ? en : nx;
                    }
                }
                const u32 s = cnt - 1u, f = nx - c0;               // (entry 0 of a row is 0: cnt >= 1)
                x = f * (x >> QL_SCALE) + slot - c0;
                while (x < QL_L) {
                    if (used >= nbytes) { ok = false; break; }      // a refill past the segment's share: damaged
                    if (ni == 0) {
                        ib = 0;
                        if (used + 8 <= nbytes) { __builtin_memcpy(&ib, q + used, 8); ni = 8; }
                        else { ni = nbytes - used; for (u32 t = 0; t < ni; t++) ib |= (u64)q[used + t] << (8u * t); }
                    }
                    x = (x << 8) | (u32)(ib & 0xFFu); ib >>= 8; ni--; used++;
                }
                if (!ok) break;
                dst[j] = salpha[s];
                if (j) delta += ql_absdiff(s, q1);
                q3 = q2; q2 = q1; q1 = s;
                if (++rem == P.W) { rem = 0; pj = pj < 15u ? pj + 1u : 15u; }
            }
        }
        if (used != nbytes) ok = false;                            // ... and a share not consumed exactly
        if (!ok) atomicAdd(bad, 1u);
    }
}
__global__ __launch_bounds__(256) void k_ql_newlines(const u64 *__restrict__ boff, u64 nreads, u8 *__restrict__ out)
{
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < nreads; r += (u64)gridDim.x * blockDim.x) out[boff[r + 1] + r] = '\n';
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// (tests/cxx/emu_quals.cpp compiles everything from "#define QL_S" down to the line above for the host and runs it single-threaded)
// arena when it has room, an allocation of its own otherwise (the fused job and the restore run the codec in what they have left)
struct QlMem {
    bfq_ctx *c;
    std::vector<void *> own;
    explicit QlMem(bfq_ctx *c) : c(c) {}
    ~QlMem() { for (void *p : own) (void)hipFree(p); }
    template <typename Tp> Tp *get(u64 count)
    {
        const u64 bytes = count * sizeof(Tp) + 256;
        if (c->ws.room() >= bytes + 512) return c->alloc<Tp>(count);
        void *p = nullptr;
        if (!bfq_dev_malloc(c, &p, bytes)) throw BfqError{BFQ_E_NOMEM, "stream codec: no device memory for the quality model"};
        own.push_back(p);
        return (Tp *)p;
    }
};

// arena bytes one call takes for a stream of n bytes in nl lines beside the general codec's workspace
u64 bfq_quals_workspace(u64 n, u64 nl)
{
    const u64 nseg = n / QL_S + 2;
    return 24 * (nl + 64) + 32 * (n / 4096 + 64) + 2 * n + 48 * nseg + 12ull * QL_MAX_TABLE + (8u << 20) + bfq_codec_workspace(4 * nl);
}

// counts at rung `hi` (rows x A) summed into the rows of rung `lo` <= hi: the rungs are nested
static std::vector<u32> ql_collapse(const std::vector<u32> &cnt, u32 hi, u32 lo, u32 A)
{
    if (hi == lo) return cnt;
    const QlPar H = ql_par(A, hi, 1), L = ql_par(A, lo, 1);
    std::vector<u32> out(ql_rows(lo, A) * A, 0);
    const u64 rows = ql_rows(hi, A);
    for (u64 x = 0; x < rows; x++) {
        u64 v = x;
        const u32 q1 = (u32)(v % A); v /= A;
        const u32 m = (u32)(v & ((1u << H.lM) - 1u)); v >>= H.lM;
        const u32 e = (u32)(v & ((1u << H.lE) - 1u)); v >>= H.lE;
        const u32 d = (u32)(v & ((1u << H.lD) - 1u)); v >>= H.lD;
        const u32 p = (u32)v;
        const u32 to = ((((((p >> (H.lP - L.lP)) << L.lD) | (d >> (H.lD - L.lD))) << L.lE) | (L.lE ? e : 0u)) << L.lM | (m >> (H.lM - L.lM))) * A + q1;
        for (u32 s = 0; s < A; s++) {
            const u64 t = (u64)out[(u64)to * A + s] + cnt[x * A + s];
            out[(u64)to * A + s] = t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)t;
        }
    }
    return out;
}
// estimated bits of the container made with these counts (the estimator of choose_order(), oracle/bfq_codec_ref.c)
static u64 ql_estimate(const std::vector<u32> &cnt, u64 rows, u32 A, u32 St)
{
    u64 bits = 0, used = 0;
    u16 f[64];
    for (u64 x = 0; x < rows; x++) {
        u64 T = 0;
        for (u32 s = 0; s < A; s++) T += cnt[x * A + s];
        if (!T) continue;
        used++;
        bfq_codec_normalise(cnt.data() + x * A, A, f);
        for (u32 s = 0; s < A; s++) bits += (u64)cnt[x * A + s] * bfq_codec_bit_cost(f[s]);
    }
    return bits / 256 * St + used * A * 16 + rows;
}

// The BFQQUAL1 container of d_in (n raw bytes on the device) into d_out.  Returns its length; 0 when the stream is not
// eligible; QL_NOFIT when the container needs more than `cap` bytes (nothing useful is in d_out then).
// flags: bit 1 = the rung in bits 8-9 is forced.
static u64 ql_container_device(bfq_ctx *c, const u8 *d_in, u64 n, u32 flags, u8 *d_out, u64 cap)
{
    if (!n) return 0;
    const size_t mk = c->mark();
    struct Rel { bfq_ctx *c; size_t mk; ~Rel() { c->release(mk); } } rel{c, mk};
    QlMem M(c);
    u8 last = 0;
    HIP_CHECK(hipMemcpyAsync(&last, d_in + n - 1, 1, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (last != 10) return 0;
    u64 nl = 0;
    const u64 *lineEnd = bfq_line_index(c, d_in, n, &nl);
    const u64 nvals = n - nl, nseg = (nvals + QL_S - 1) / QL_S;
    if (!nl || !nvals || nseg > 0xFFFFFFFFull || nvals >= (1ull << 38)) return 0;
    u32 *lens = M.get<u32>(nl + 4), *d_small = M.get<u32>(256 + 1);
    u64 *boff = M.get<u64>(nl + 2);
    HIP_CHECK(hipMemsetAsync(d_small, 0, 4 * 257, c->stream));
    KLAUNCH(c, K_CODEC, 12.0 * (double)nl, k_ql_lens, bfq_grid(nl, 256 * 8), 256, lineEnd, nl, lens, d_small + 256);
    KLAUNCH(c, K_CODEC, (double)n, k_ql_present, bfq_grid(n, 256 * 64), 256, d_in, n, d_small);
    bfq_exscan_u32(c, lens, boff, nl, boff + nl);
    u32 small[257];
    HIP_CHECK(hipMemcpyAsync(small, d_small, 4 * 257, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const u32 maxlen = small[256];
    if (maxlen > QL_MAXLINE) return 0;
    u8 alphabet[64] = {0}, map[256] = {0};
    u32 A = 0;
    for (u32 b = 0; b < 256; b++) {
        if (!small[b] || b == 10) continue;
        if (A == 64) return 0;
        map[b] = (u8)A; alphabet[A++] = (u8)b;
    }
    const u32 St = ql_sample_step(nvals);
    u32 rmax = 0;
    if (flags & 2u) rmax = (flags >> 8) & 3u;
    else {
        u64 limit = (nvals / St) >> 4;
        limit = limit < 4096 ? 4096 : limit > QL_MAX_TABLE ? QL_MAX_TABLE : limit;
        for (u32 r = 1; r < 4; r++) if (ql_rows(r, A) * A <= limit) rmax = r;
    }
    u8 *d_map = M.get<u8>(256 + 64);
    HIP_CHECK(hipMemcpyAsync(d_map, map, 256, hipMemcpyHostToDevice, c->stream));
    u64 *segFirst = M.get<u64>(nseg + 2);
    KLAUNCH(c, K_CODEC, 8.0 * (double)nseg, k_ql_segfirst, bfq_grid(nseg + 1, 256), 256, (const u64 *)boff, nl, nseg, segFirst);
    const QlIn I{d_in, n, boff, segFirst, nseg};
    u64 E = ql_rows(rmax, A) * A;
    u32 *d_cnt = M.get<u32>(E);
    HIP_CHECK(hipMemsetAsync(d_cnt, 0, 4 * E, c->stream));
    KLAUNCH(c, K_CODEC, (double)n / St, k_ql_count, bfq_grid((nseg + St - 1) / St, 256), 256, I, (const u8 *)d_map, ql_par(A, rmax, maxlen), St, d_cnt);
    std::vector<u32> cnt(E);
    HIP_CHECK(hipMemcpyAsync(cnt.data(), d_cnt, 4 * E, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    u32 rung = rmax;
    if (!(flags & 2u)) {                                           // the rung whose estimated container is smallest, the lowest among equals
        u64 bestBits = ~0ull;
        std::vector<u32> keep;
        for (u32 r = 0; r <= rmax; r++) {
            std::vector<u32> lvl = ql_collapse(cnt, rmax, r, A);
            const u64 bits = ql_estimate(lvl, ql_rows(r, A), A, St);
            if (bits < bestBits) { bestBits = bits; rung = r; keep.swap(lvl); }
        }
        cnt.swap(keep);
    }
    const u64 rows = ql_rows(rung, A);
    E = rows * A;
    std::vector<u16> freq(E);
    std::vector<u8> used((rows + 7) / 8, 0);
    std::vector<u32> fcv(E);
    u32 cnt0[64] = {0};
    u16 dflt[64];
    u64 nused = 0;
    for (u64 x = 0; x < rows; x++)
        for (u32 s = 0; s < A; s++) { const u64 v = (u64)cnt0[s] + cnt[x * A + s]; cnt0[s] = v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)v; }
    bfq_codec_normalise(cnt0, A, dflt);
    for (u64 x = 0; x < rows; x++) {
        u64 T = 0;
        for (u32 s = 0; s < A; s++) T += cnt[x * A + s];
        if (T) { nused++; used[x >> 3] |= (u8)(1u << (x & 7)); bfq_codec_normalise(cnt.data() + x * A, A, freq.data() + x * A); }
        else memcpy(freq.data() + x * A, dflt, 2 * A);
        u32 acc = 0;
        for (u32 s = 0; s < A; s++) { fcv[x * A + s] = (u32)freq[x * A + s] | (acc << 16); acc += freq[x * A + s]; }
    }
    if (cap < QL_HDR) return QL_NOFIT;
    const u64 checksum = bfq_codec_checksum_device(c, d_in, n, M.get<u64>(1));
    u64 ll = 0;
    try { ll = bfq_rans_compress_device(c, (const u8 *)lens, 4 * nl, d_out + QL_HDR, cap - QL_HDR, false); }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; return QL_NOFIT; }
    const u64 model = 64 + 2ull * A + used.size() + 2ull * A * nused;
    const u64 hdr = QL_HDR + ll + model + 4 * nseg;
    if (hdr > cap) return QL_NOFIT;
    u32 *d_fc = M.get<u32>(E), *segBytes = M.get<u32>(nseg + 1);
    u64 *off = M.get<u64>(nseg + 1), *d_total = M.get<u64>(1);
    u8 *scratch = M.get<u8>(2 * nvals + 16 * (nseg + 1) + 64);
    HIP_CHECK(hipMemcpyAsync(d_fc, fcv.data(), 4 * E, hipMemcpyHostToDevice, c->stream));
    KLAUNCH(c, K_CODEC, 3.0 * (double)n, k_ql_encode, bfq_grid(nseg, 64), 64, I, (const u8 *)d_map, ql_par(A, rung, maxlen), (const u32 *)d_fc, scratch, segBytes);
    bfq_exscan_u32(c, segBytes, off, nseg, d_total);
    KLAUNCH(c, K_CODEC, 0.0, k_ql_pack, bfq_grid(nseg * 64, 256), 256, I, (const u8 *)scratch, (const u32 *)segBytes, (const u64 *)off, d_out + hdr, cap - hdr);
    u64 total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                                     // (fcv is a host temporary too)
    if (hdr + total > cap) return QL_NOFIT;
    std::vector<u8> h(QL_HDR + model);
    u8 *p = h.data();
    memcpy(p, "BFQQUAL1", 8); ql_put64(p + 8, n); ql_put64(p + 16, nl); ql_put64(p + 24, nvals);
    ql_put32(p + 32, QL_S); ql_put32(p + 36, (u32)nseg); ql_put32(p + 40, A); ql_put32(p + 44, rung); ql_put32(p + 48, QL_SCALE); ql_put32(p + 52, maxlen);
    ql_put64(p + 56, checksum); ql_put64(p + 64, ll);
    p += QL_HDR;
    memcpy(p, alphabet, 64); p += 64;
    for (u32 s = 0; s < A; s++) { p[0] = (u8)dflt[s]; p[1] = (u8)(dflt[s] >> 8); p += 2; }
    memcpy(p, used.data(), used.size()); p += used.size();
    for (u64 x = 0; x < rows; x++) {
        if (!((used[x >> 3] >> (x & 7)) & 1)) continue;
        for (u32 s = 0; s < A; s++) { p[0] = (u8)freq[x * A + s]; p[1] = (u8)(freq[x * A + s] >> 8); p += 2; }
    }
    HIP_CHECK(hipMemcpyAsync(d_out, h.data(), QL_HDR, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(d_out + QL_HDR + ll, h.data() + QL_HDR, model, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(d_out + QL_HDR + ll + model, segBytes, 4 * nseg, hipMemcpyDeviceToDevice, c->stream));
    c->sync();
    return hdr + total;
}

// what bfq_quals_compress gives (flags as there) for d_in on the device, into d_out (capacity cap)
u64 bfq_quals_finish(bfq_ctx *c, const u8 *d_in, u64 n, u32 flags, u8 *d_out, u64 cap)
{
    const BfqError small{BFQ_E_ARG, "output buffer too small for the compressed stream"};
    if (flags & 1u) {
        const u64 got = ql_container_device(c, d_in, n, flags, d_out, cap);
        if (got == QL_NOFIT) throw small;
        return got ? got : bfq_codec_compress_device(c, d_in, n, d_out, cap);
    }
    // the general container first; the other one is kept only when it fits into fewer bytes
    const u64 general = bfq_codec_compress_device(c, d_in, n, d_out, cap);
    if (general < QL_HDR + 1) return general;
    const size_t mk = c->mark();
    QlMem M(c);
    u8 *d_z = M.get<u8>(general + 16);
    const u64 got = ql_container_device(c, d_in, n, flags, d_z, general - 1);
    if (got && got != QL_NOFIT) {
        HIP_CHECK(hipMemcpyAsync(d_out, d_z, got, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
    }
    c->release(mk);
    return got && got != QL_NOFIT ? got : general;
}

struct QlHeader { u64 n, nreads, nvals, ll, rows, nused, model, total; u32 nseg, A, rung, maxlen; };
// the header and the shares behind it; every field is checked before it is used as a size
static void ql_parse(const u8 *in, u64 len, QlHeader &H)
{
    const BfqError bad{BFQ_E_ARG, "damaged BFQQUAL1 stream"};
    if (len < QL_HDR || memcmp(in, "BFQQUAL1", 8)) throw bad;
    H.n = ql_get64(in + 8); H.nreads = ql_get64(in + 16); H.nvals = ql_get64(in + 24);
    H.nseg = ql_get32(in + 36); H.A = ql_get32(in + 40); H.rung = ql_get32(in + 44); H.maxlen = ql_get32(in + 52);
    H.ll = ql_get64(in + 64);
    if (ql_get32(in + 32) != QL_S || ql_get32(in + 48) != QL_SCALE || H.A < 1 || H.A > 64 || H.rung > 3 || H.maxlen > QL_MAXLINE) throw bad;
    if (H.nreads == 0 || H.nvals == 0 || H.nvals >= (1ull << 38) || H.nreads > (1ull << 46) || H.nvals + H.nreads != H.n ||
        (u64)H.nseg != (H.nvals + QL_S - 1) / QL_S)
        throw bad;
    H.rows = ql_rows(H.rung, H.A);
    if (H.ll > len - QL_HDR || len - QL_HDR - H.ll < 64 + 2ull * H.A + (H.rows + 7) / 8) throw bad;
    const u8 *alpha = in + QL_HDR + H.ll;
    for (u32 s = 0; s < H.A; s++) if (alpha[s] == 10 || (s && alpha[s] <= alpha[s - 1])) throw bad;
    const u8 *used = alpha + 64 + 2ull * H.A;
    H.nused = 0;
    for (u64 x = 0; x < H.rows; x++) H.nused += (used[x >> 3] >> (x & 7)) & 1;
    H.model = 64 + 2ull * H.A + (H.rows + 7) / 8 + 2ull * H.A * H.nused;
    const u64 hdr = QL_HDR + H.ll + H.model;
    if (hdr > len || 4ull * H.nseg > len - hdr) throw bad;
    H.total = hdr + 4ull * H.nseg;
    for (u32 g = 0; g < H.nseg; g++) H.total += ql_get32(in + hdr + 4ull * g);
    if (H.total > len) throw bad;
}
u64 bfq_quals_member_len(const u8 *h_in, u64 len)
{
    QlHeader H;
    ql_parse(h_in, len, H);
    return H.total;
}

// h_in: the whole container on the host, d_in: the same bytes on the device.  The raw bytes go to d_out; returns their number.
u64 bfq_quals_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap)
{
    const BfqError bad{BFQ_E_ARG, "damaged BFQQUAL1 stream"};
    QlHeader H;
    ql_parse(h_in, len, H);
    if (H.total != len) throw bad;                                 // the seg_bytes add up to the payload
    if (H.n > cap) throw BfqError{BFQ_E_ARG, "output buffer too small for the raw stream"};
    const u32 A = H.A;
    const u64 rows = H.rows;
    const u8 *lm = h_in + QL_HDR;
    if (H.ll < 16 || memcmp(lm, "BFQRANS2", 8)) throw bad;
    try { if (bfq_codec_raw_len(lm, H.ll) != 4 * H.nreads || bfq_codec_member_len(lm, H.ll) != H.ll) throw bad; }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw bad; }
    // the model: cumulative rows padded to a multiple of 8 entries with 2^12
    const u8 *alpha = lm + H.ll, *dfl = alpha + 64, *used = dfl + 2ull * A, *rp = used + (rows + 7) / 8;
    const u32 nld = (A + 7) / 8, Ap = 8 * nld;
    std::vector<u16> cum(rows * Ap);
    for (u64 x = 0; x < rows; x++) {
        const u8 *row = dfl;
        if ((used[x >> 3] >> (x & 7)) & 1) { row = rp; rp += 2ull * A; }
        u32 acc = 0;
        for (u32 s = 0; s < Ap; s++) {
            cum[x * Ap + s] = (u16)(s < A ? acc : 1u << QL_SCALE);
            if (s < A) acc += (u32)row[2 * s] | ((u32)row[2 * s + 1] << 8);
            if (acc > (1u << QL_SCALE)) throw bad;
        }
        if (acc != (1u << QL_SCALE)) throw bad;
    }
    const size_t mk = c->mark();
    struct Rel { bfq_ctx *c; size_t mk; ~Rel() { c->release(mk); } } rel{c, mk};
    QlMem M(c);
    u32 *lens = M.get<u32>(H.nreads + 4), *d_small = M.get<u32>(2);
    u64 *boff = M.get<u64>(H.nreads + 2);
    try { if (bfq_rans_decompress_device(c, lm, d_in + QL_HDR, H.ll, (u8 *)lens, 4 * H.nreads) != 4 * H.nreads) throw bad; }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw BfqError{BFQ_E_ARG, "damaged BFQQUAL1 stream (the lens member: " + e.msg + ")"}; }
    HIP_CHECK(hipMemsetAsync(d_small, 0, 8, c->stream));
    KLAUNCH(c, K_CODEC, 4.0 * (double)H.nreads, k_ql_lenmax, bfq_grid(H.nreads, 256 * 8), 256, (const u32 *)lens, H.nreads, d_small);
    bfq_exscan_u32(c, lens, boff, H.nreads, boff + H.nreads);
    u64 tv = 0;
    u32 small[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(&tv, boff + H.nreads, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(small, d_small, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (tv != H.nvals || small[0] != H.maxlen) throw bad;
    const u64 nseg = H.nseg;
    u32 *segBytes = M.get<u32>(nseg + 1), *d_bad = d_small + 1;
    u64 *off = M.get<u64>(nseg + 1), *segFirst = M.get<u64>(nseg + 2);
    u16 *d_cum = M.get<u16>(rows * Ap + 8);
    u8 *d_alpha = M.get<u8>(64);
    const u64 hdr = QL_HDR + H.ll + H.model;
    HIP_CHECK(hipMemcpyAsync(segBytes, h_in + hdr, 4 * nseg, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(d_cum, cum.data(), 2 * rows * Ap, hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemcpyAsync(d_alpha, alpha, 64, hipMemcpyHostToDevice, c->stream));
    bfq_exscan_u32(c, segBytes, off, nseg, nullptr);
    KLAUNCH(c, K_CODEC, 8.0 * (double)nseg, k_ql_segfirst, bfq_grid(nseg + 1, 256), 256, (const u64 *)boff, H.nreads, nseg, segFirst);
    const QlIn I{nullptr, H.n, boff, segFirst, nseg};
    KLAUNCH(c, K_CODEC, 3.0 * (double)H.n, k_ql_decode, bfq_grid(nseg, 64), 64, I, d_in + hdr + 4 * nseg, (const u64 *)off, (const u32 *)segBytes,
            (const u8 *)d_alpha, ql_par(A, H.rung, H.maxlen), (const u16 *)d_cum, nld, d_out, d_bad);
    KLAUNCH(c, K_CODEC, 8.0 * (double)H.nreads, k_ql_newlines, bfq_grid(H.nreads, 256 * 4), 256, (const u64 *)boff, H.nreads, d_out);
    u32 nbad = 0;
    HIP_CHECK(hipMemcpyAsync(&nbad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();                                                     // (cum is a host temporary)
    if (nbad) throw bad;
    if (bfq_codec_checksum_device(c, d_out, H.n, M.get<u64>(1)) != ql_get64(h_in + 56)) throw BfqError{BFQ_E_ARG, "damaged BFQQUAL1 stream (checksum of the decoded bytes)"};
    return H.n;
}
