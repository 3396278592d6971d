// k_compare.hip -- two FASTQ texts compared where they lie (include/bfqzip_hip.h, bfq_fastq_compare): what a lossy run did
// to the bases and the qualities, as exact integer counts.
//
// Both texts are on the device with their record indexes (k_fastq.hip: one FqRec per record, nothing gathered).  Three passes:
//   k_cmp_check   : one lane per read of A: its partner in B (directly, or through the inverse of the permutation), the
//                   smallest read whose sequence length differs (one atomic min), the header classes
//   k_cmp_compare : one wave per read, 64 positions per step: consecutive lanes read consecutive bytes of the four lines (A
//                   seq, B seq, A qual, B qual), each byte once.  What is the same for the whole wave (counts of differing
//                   positions, the base composition) comes from ballots and stays in scalar registers; the sums of |d| stay in
//                   lane registers and are reduced across the wave at the end; the histograms, the off-diagonal of the
//                   substitution matrix and the position profiles are 32-bit counters in LDS, flushed with 64-bit global
//                   atomics.  The per-read number of differing positions goes to an array
//   k_cmp_emit    : (only when a diff list is asked for and there is something to list) the reads whose offset -- the scan
//                   of that array -- lies below the cap are compared again; a step's records are placed by ballot + prefix
//                   popcount, the running count carried across the steps of a long read
//
// The LDS counters.  Layout = the report's arrays from `subst` on (CMP_NCNT = 36 + 3 * 256 + 4 * 512 = 2852 counters), so the
// flush is one loop.  Not counted per byte: the diagonal of `subst` -- a wave counts the classes of A's bases by ballot
// (comp[6]), and diagonal k = comp[k] - the off-diagonal entries of row k, which are counted one by one (they are rare).
// The quality histograms are skewed (a smoothed read is mostly one value), and 64 lanes adding 1 to one LDS word take their
// turns.  Two forms were measured at 30 M x 150 (profiles/compare/README.md): every lane adds 1 (34.3 ms), and only the lanes
// whose value differs from the lane before them add, the length of the run that starts there (one shuffle, one ballot:
// 38.4 ms).  The plain adds are what runs; $BFQ_CMP_HIST=runs selects the other form for A/B measurements.
//
// Bound of a 32-bit LDS counter: a workgroup flushes as soon as it has handled more than CMP_FLUSH_POS positions since its
// last flush, looked at after every batch of CMP_BATCH reads.  A batch has at most CMP_BATCH * BFQ_MAX_READ_LEN = 4 160 000
// positions, so at most CMP_FLUSH_POS + 4 160 000 = 2^24 positions lie between two flushes; the largest amount one position
// adds to one counter is 255 (pos_abs: |d| of two bytes), and 2^24 * 255 < 2^32.
#include <string.h>
#include <stddef.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"

#define CMP_THREADS 256
#define CMP_WAVES (CMP_THREADS / 64)
#define CMP_BATCH 64                                      // reads per workgroup and batch (16 per wave)
#define CMP_FLUSH_POS ((1u << 24) - CMP_BATCH * BFQ_MAX_READ_LEN)
#define CMP_NSUB (BFQ_CMP_SYMS * BFQ_CMP_SYMS)
#define CMP_QA CMP_NSUB
#define CMP_QB (CMP_QA + 256)
#define CMP_CBQ (CMP_QB + 256)
#define CMP_PLEN (CMP_CBQ + 256)
#define CMP_PBASE (CMP_PLEN + BFQ_CMP_POS)
#define CMP_PQUAL (CMP_PBASE + BFQ_CMP_POS)
#define CMP_PABS (CMP_PQUAL + BFQ_CMP_POS)
#define CMP_NCNT (CMP_PABS + BFQ_CMP_POS)

static_assert(CMP_BATCH * (u64)BFQ_MAX_READ_LEN < (1u << 24), "a batch must fit below the flush bound");
static_assert(((u64)CMP_FLUSH_POS + CMP_BATCH * (u64)BFQ_MAX_READ_LEN) * 255ull < (1ull << 32), "32-bit LDS counters would wrap");
static_assert(offsetof(bfq_compare_report, qual_hist_a) == offsetof(bfq_compare_report, subst) + 8 * CMP_QA &&
              offsetof(bfq_compare_report, qual_hist_b) == offsetof(bfq_compare_report, subst) + 8 * CMP_QB &&
              offsetof(bfq_compare_report, changed_base_qual_hist) == offsetof(bfq_compare_report, subst) + 8 * CMP_CBQ &&
              offsetof(bfq_compare_report, pos_len) == offsetof(bfq_compare_report, subst) + 8 * CMP_PLEN &&
              offsetof(bfq_compare_report, pos_bases) == offsetof(bfq_compare_report, subst) + 8 * CMP_PBASE &&
              offsetof(bfq_compare_report, pos_quals) == offsetof(bfq_compare_report, subst) + 8 * CMP_PQUAL &&
              offsetof(bfq_compare_report, pos_abs) == offsetof(bfq_compare_report, subst) + 8 * CMP_PABS &&
              offsetof(bfq_compare_report, reserved) == offsetof(bfq_compare_report, subst) + 8 * CMP_NCNT,
              "the LDS counters mirror the report's arrays");
static_assert(sizeof(bfq_compare_diff) == 16, "a diff record is 16 bytes");

typedef unsigned long long ull;

// A 0, C 1, G 2, N 3, T 4 (the project's order), every other byte 5
__device__ __forceinline__ u32 cmp_class(u32 b) { return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'N' ? 3u : b == 'T' ? 4u : 5u; }

// a header line without its line end: the CR of a CRLF goes too
__device__ __forceinline__ u32 cmp_hdr_len(const u8 *__restrict__ buf, const FqRec &r)
{
    return r.hdrLen && buf[r.hdrStart + r.hdrLen - 1] == 13 ? r.hdrLen - 1 : r.hdrLen;
}

__global__ __launch_bounds__(256) void k_cmp_check(CmpText A, CmpText B, const u64 *__restrict__ inv, u64 N, bfq_compare_report *rep,
                                                   ull *__restrict__ badRead)
{
    u64 same = 0, dropped = 0, changed = 0, bad = ~0ull;          // same / dropped / changed: wave-uniform
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (u64)gridDim.x * blockDim.x) {
        const u64 j = inv ? inv[i] : i;
        const FqRec ra = A.rec[i], rb = B.rec[j];
        if (ra.len != rb.len && i < bad) bad = i;
        const u32 la = cmp_hdr_len(A.buf, ra), lb = cmp_hdr_len(B.buf, rb);
        const u8 *__restrict__ ha = A.buf + ra.hdrStart, *__restrict__ hb = B.buf + rb.hdrStart;
        bool eq = la == lb;
        for (u32 k = 0; eq && k < la; k++) eq = ha[k] == hb[k];
        const u32 cls = eq ? 0u : (lb == 1 && hb[0] == (u8)'@') ? 1u : 2u;
        same += __popcll(__ballot(cls == 0));
        dropped += __popcll(__ballot(cls == 1));
        changed += __popcll(__ballot(cls == 2));
    }
    if (bad != ~0ull) atomicMin(badRead, (ull)bad);
    if (bfq_lane() == 0) {                                        // (lane 0 has the smallest index of its wave: in every trip any lane made)
        if (same) atomicAdd((ull *)&rep->headers_same, (ull)same);
        if (dropped) atomicAdd((ull *)&rep->headers_dropped, (ull)dropped);
        if (changed) atomicAdd((ull *)&rep->headers_changed, (ull)changed);
    }
}

// every active lane's value v counted in h[]: the active lanes are lanes 0 .. n - 1
template <bool RUNS> __device__ __forceinline__ void cmp_hist_add(u32 *h, u32 v, bool act, u32 lane)
{
    if (!RUNS) {
        if (act) atomicAdd(&h[v], 1u);
        return;
    }
    const u32 prev = (u32)__shfl_up((int)v, 1);
    const bool head = act && (lane == 0 || v != prev);
    const u64 hm = __ballot(head), am = __ballot(act);
    if (head) {
        const u64 above = (hm >> lane) >> 1;                      // the run heads after mine
        const u32 next = above ? lane + 1 + (u32)__builtin_ctzll(above) : (u32)__popcll(am);
        atomicAdd(&h[v], next - lane);
    }
}

// the workgroup's LDS counters into the report, and back to zero.  The caller has synchronised.
__device__ __forceinline__ void cmp_flush(u32 *cnt, u32 *comp, bfq_compare_report *rep)
{
    ull *dst = (ull *)rep->subst;
    for (u32 t = threadIdx.x; t < CMP_NCNT; t += CMP_THREADS) {
        u32 v = cnt[t];
        if (t < CMP_NSUB && t % (BFQ_CMP_SYMS + 1) == 0) {        // diagonal k: the bases of class k that did not leave it
            const u32 k = t / (BFQ_CMP_SYMS + 1);
            v = comp[k];
            for (u32 j = 0; j < BFQ_CMP_SYMS; j++)
                if (j != k) v -= cnt[BFQ_CMP_SYMS * k + j];
        }
        if (v) atomicAdd(dst + t, (ull)v);
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < CMP_NCNT; t += CMP_THREADS) cnt[t] = 0;
    if (threadIdx.x < 8) comp[threadIdx.x] = 0;
    __syncthreads();
}

template <bool RUNS>
__global__ __launch_bounds__(CMP_THREADS) void k_cmp_compare(CmpText A, CmpText B, const u64 *__restrict__ inv, u64 N, u64 nbatches,
                                                             bfq_compare_report *rep, u32 *__restrict__ readDiffs)
{
    __shared__ u32 cnt[CMP_NCNT];
    __shared__ u32 comp[8];                                       // A's bases by class since the last flush
    __shared__ u32 shPos;                                         // positions since the last flush
    const u32 lane = bfq_lane(), w = threadIdx.x >> 6;
    for (u32 t = threadIdx.x; t < CMP_NCNT; t += CMP_THREADS) cnt[t] = 0;
    if (threadIdx.x < 8) comp[threadIdx.x] = 0;
    if (threadIdx.x == 0) shPos = 0;
    __syncthreads();

    u64 absSum = 0, sqSum = 0;                                    // per lane
    u32 absMax = 0;
    u64 nDiffs = 0, nBases = 0, nQuals = 0, nUp = 0, nDown = 0, rAny = 0, rBases = 0, rQuals = 0, first = ~0ull;   // wave-uniform
    u32 compReg[BFQ_CMP_SYMS] = {0, 0, 0, 0, 0, 0};               // wave-uniform, since the last flush

    for (u64 bt = blockIdx.x; bt < nbatches; bt += gridDim.x) {
        u32 wavePos = 0;
        for (u32 k = w; k < CMP_BATCH; k += CMP_WAVES) {
            const u64 i = bt * CMP_BATCH + k;
            if (i >= N) break;
            const u64 j = inv ? inv[i] : i;
            const FqRec ra = A.rec[i], rb = B.rec[j];
            const u32 L = ra.len;                                 // (== rb.len: k_cmp_check)
            const u8 *__restrict__ sa = A.buf + ra.seqStart, *__restrict__ qa = A.buf + ra.qualStart;
            const u8 *__restrict__ sb = B.buf + rb.seqStart, *__restrict__ qb = B.buf + rb.qualStart;
            u32 rd = 0, rdB = 0, rdQ = 0;
            for (u32 p0 = 0; p0 < L; p0 += 64) {
                const u32 p = p0 + lane;
                const bool act = p < L;
                u32 ba = 0, bb = 0, xa = 0, xb = 0;
                if (act) { ba = sa[p]; bb = sb[p]; xa = qa[p]; xb = qb[p]; }
                const bool bch = ba != bb, qch = xa != xb;        // (inactive lanes: all four are 0)
                const int d = (int)xb - (int)xa;
                const u32 ad = (u32)(d < 0 ? -d : d);
                const u32 cB = (u32)__popcll(__ballot(bch)), cQ = (u32)__popcll(__ballot(qch)), cD = (u32)__popcll(__ballot(bch || qch));
                rd += cD; rdB += cB; rdQ += cQ;
                nUp += __popcll(__ballot(d > 0)); nDown += __popcll(__ballot(d < 0));
                absSum += ad; sqSum += (u64)ad * ad;
                absMax = ad > absMax ? ad : absMax;
                const u32 ca = cmp_class(ba), cb = cmp_class(bb);
#pragma unroll
                for (u32 s = 0; s < BFQ_CMP_SYMS; s++) compReg[s] += (u32)__popcll(__ballot(act && ca == s));
                if (act && ca != cb) atomicAdd(&cnt[BFQ_CMP_SYMS * ca + cb], 1u);
                cmp_hist_add<RUNS>(cnt + CMP_QA, xa, act, lane);
                cmp_hist_add<RUNS>(cnt + CMP_QB, xb, act, lane);
                if (bch) atomicAdd(&cnt[CMP_CBQ + xa], 1u);
                if (p0 < BFQ_CMP_POS) {                           // bins of their own: no two lanes meet
                    const u32 bin = p < BFQ_CMP_POS - 1 ? p : BFQ_CMP_POS - 1;
                    if (act) atomicAdd(&cnt[CMP_PLEN + bin], 1u);
                    if (bch) atomicAdd(&cnt[CMP_PBASE + bin], 1u);
                    if (qch) { atomicAdd(&cnt[CMP_PQUAL + bin], 1u); atomicAdd(&cnt[CMP_PABS + bin], ad); }
                } else {                                          // the whole step lies in the last bin
                    u32 sAbs = ad;
                    for (int o = 32; o; o >>= 1) sAbs += (u32)__shfl_xor((int)sAbs, o);
                    if (lane == 0) {
                        atomicAdd(&cnt[CMP_PLEN + BFQ_CMP_POS - 1], (L - p0 < 64u ? L - p0 : 64u));
                        if (cB) atomicAdd(&cnt[CMP_PBASE + BFQ_CMP_POS - 1], cB);
                        if (cQ) { atomicAdd(&cnt[CMP_PQUAL + BFQ_CMP_POS - 1], cQ); atomicAdd(&cnt[CMP_PABS + BFQ_CMP_POS - 1], sAbs); }
                    }
                }
            }
            wavePos += L;
            if (lane == 0) readDiffs[i] = rd;
            nDiffs += rd; nBases += rdB; nQuals += rdQ;
            if (rd) { rAny++; if (i < first) first = i; }
            rBases += rdB ? 1 : 0; rQuals += rdQ ? 1 : 0;
        }
        if (lane == 0 && wavePos) atomicAdd(&shPos, wavePos);
        __syncthreads();
        const bool flush = shPos > CMP_FLUSH_POS;                 // the same for the whole workgroup
        __syncthreads();
        if (flush) {
            if (lane < BFQ_CMP_SYMS) {
                u32 v = 0;
#pragma unroll
                for (u32 s = 0; s < BFQ_CMP_SYMS; s++) v = lane == s ? compReg[s] : v;
                if (v) atomicAdd(&comp[lane], v);
            }
#pragma unroll
            for (u32 s = 0; s < BFQ_CMP_SYMS; s++) compReg[s] = 0;
            if (threadIdx.x == 0) shPos = 0;
            __syncthreads();
            cmp_flush(cnt, comp, rep);
        }
    }
    if (lane < BFQ_CMP_SYMS) {
        u32 v = 0;
#pragma unroll
        for (u32 s = 0; s < BFQ_CMP_SYMS; s++) v = lane == s ? compReg[s] : v;
        if (v) atomicAdd(&comp[lane], v);
    }
    __syncthreads();
    cmp_flush(cnt, comp, rep);

    for (int o = 32; o; o >>= 1) {
        absSum += (u64)__shfl_xor((ull)absSum, o);
        sqSum += (u64)__shfl_xor((ull)sqSum, o);
        const u32 m = (u32)__shfl_xor((int)absMax, o);
        absMax = m > absMax ? m : absMax;
    }
    if (lane == 0) {
        if (nDiffs) atomicAdd((ull *)&rep->n_diffs, (ull)nDiffs);
        if (rAny) atomicAdd((ull *)&rep->reads_changed, (ull)rAny);
        if (rBases) atomicAdd((ull *)&rep->reads_bases_changed, (ull)rBases);
        if (rQuals) atomicAdd((ull *)&rep->reads_quals_changed, (ull)rQuals);
        if (nBases) atomicAdd((ull *)&rep->bases_changed, (ull)nBases);
        if (nQuals) atomicAdd((ull *)&rep->quals_changed, (ull)nQuals);
        if (nUp) atomicAdd((ull *)&rep->quals_raised, (ull)nUp);
        if (nDown) atomicAdd((ull *)&rep->quals_lowered, (ull)nDown);
        if (absSum) atomicAdd((ull *)&rep->qual_abs_sum, (ull)absSum);
        if (sqSum) atomicAdd((ull *)&rep->qual_sq_sum, (ull)sqSum);
        if (absMax) atomicMax((ull *)&rep->qual_abs_max, (ull)absMax);
        if (first != ~0ull) atomicMin((ull *)&rep->first_changed_read, (ull)first);
    }
}

// the differing positions of the reads whose first record lies below the cap, in (read, pos) order: record diffOff[i] + the
// number of differing positions of read i before this one
__global__ __launch_bounds__(256) void k_cmp_emit(CmpText A, CmpText B, const u64 *__restrict__ inv, u64 N, const u32 *__restrict__ readDiffs,
                                                  const u64 *__restrict__ diffOff, u64 cap, bfq_compare_diff *__restrict__ out)
{
    const u32 lane = bfq_lane();
    const u64 below = ((u64)1 << lane) - 1;
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < N; i += nwaves) {
        const u64 off = diffOff[i];
        if (!readDiffs[i] || off >= cap) continue;
        const u64 j = inv ? inv[i] : i;
        const FqRec ra = A.rec[i], rb = B.rec[j];
        const u32 L = ra.len;
        const u8 *__restrict__ sa = A.buf + ra.seqStart, *__restrict__ qa = A.buf + ra.qualStart;
        const u8 *__restrict__ sb = B.buf + rb.seqStart, *__restrict__ qb = B.buf + rb.qualStart;
        u64 at = off;                                             // record of the step's first differing position
        for (u32 p0 = 0; p0 < L && at < cap; p0 += 64) {
            const u32 p = p0 + lane;
            u32 ba = 0, bb = 0, xa = 0, xb = 0;
            if (p < L) { ba = sa[p]; bb = sb[p]; xa = qa[p]; xb = qb[p]; }
            const bool df = ba != bb || xa != xb;
            const u64 m = __ballot(df);
            const u64 idx = at + (u64)__popcll(m & below);
            if (df && idx < cap) {
                ulonglong2 r;
                r.x = i;
                r.y = (ull)p | (ull)ba << 32 | (ull)bb << 40 | (ull)xa << 48 | (ull)xb << 56;   // pos, base_a, base_b, qual_a, qual_b
                *(ulonglong2 *)(out + idx) = r;
            }
            at += (u64)__popcll(m);
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
void bfq_compare_check(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, bfq_compare_report *d_rep, u64 *d_badRead)
{
    if (!N) return;
    KLAUNCH(c, K_CMP_CHECK, (64.0 + (inv ? 8.0 : 0.0)) * (double)N, k_cmp_check, bfq_grid(N, 256), 256, A, B, inv, N, d_rep, (ull *)d_badRead);
}

void bfq_compare_pass(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, u64 total, bfq_compare_report *d_rep, u32 *readDiffs)
{
    if (!N) return;
    const u64 nbatches = ceil_div(N, CMP_BATCH);
    const unsigned grid = (unsigned)std::min<u64>(nbatches, 2048);   // 8 workgroups per CU; the rest by stride
    const double bytes = 4.0 * (double)total + (68.0 + (inv ? 8.0 : 0.0)) * (double)N;
    const char *e = getenv("BFQ_CMP_HIST");
    if (e && !strcmp(e, "runs"))
        KLAUNCH(c, K_CMP_COMPARE, bytes, (k_cmp_compare<true>), grid, CMP_THREADS, A, B, inv, N, nbatches, d_rep, readDiffs);
    else
        KLAUNCH(c, K_CMP_COMPARE, bytes, (k_cmp_compare<false>), grid, CMP_THREADS, A, B, inv, N, nbatches, d_rep, readDiffs);
}

void bfq_compare_emit(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, u64 total, const u32 *readDiffs, const u64 *diffOff, u64 cap,
                      bfq_compare_diff *d_out)
{
    if (!N || !cap) return;
    (void)total;
    KLAUNCH(c, K_CMP_EMIT, 12.0 * (double)N + 16.0 * (double)cap, k_cmp_emit, bfq_grid(N, 4), 256, A, B, inv, N, readDiffs, diffOff, cap, d_out);
}
