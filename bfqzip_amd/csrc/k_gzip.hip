// k_gzip.hip -- plain gzip inflated on the device: the candidate search, the two decoder passes, the windows, the resolve and
// the members' CRC32.  The text of every step is bfq_gzip.h's (the same that runs on the host under sanitizers); the host
// side that orders them is bfq_gzip.hip.  No workgroup waits for another anywhere: what one step needs of another comes
// through the launch order.  All launches are booked under the BGZF kernel class.
#include "bfq_internal.h"
#include "bfq_gzip.h"

#define GZ_WAVES 4

// Candidate search.  Schedule as built: one wave64 per piece, four pieces per 256-thread workgroup.  A wave goes through its
// piece 64 bytes = 512 bit offsets at a time: every lane takes one byte and tries its 8 bit offsets against the cheap tests
// (three header bits, HLIT / HDIST, the Kraft sum of the code-length code), reading 4 + 16 bytes around its own; the
// survivors -- about one offset in a few thousand -- are gathered by ballot and taken in stream order, and lane 0 alone runs
// the full header parse (bfq_gzip_full) for each, its 400 bytes of tables in LDS, until one passes: the piece's candidate.
__global__ __launch_bounds__(64 * GZ_WAVES) void k_gzip_candidates(const u8 *__restrict__ in, u64 len, u64 chunk, u64 np, u64 *cand)
{
    __shared__ bfq_gzip_hdrtab H[GZ_WAVES];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 k = (u64)blockIdx.x * GZ_WAVES + wave; k < np; k += (u64)gridDim.x * GZ_WAVES) {
        u64 found = BFQ_GZIP_NONE;
        const u64 lo = k * chunk, hi = (k + 1) * chunk < len ? (k + 1) * chunk : len;
        for (u64 at = lo; k && at < hi && found == BFQ_GZIP_NONE; at += 64) {
            const u64 byte = at + lane;
            u32 mask = 0;
            if (byte < hi) {
                u32 w = 0;
                for (u32 i = 0; i < 4; i++)
                    if (byte + i < len) w |= (u32)in[byte + i] << (8 * i);
                for (u32 o = 0; o < 8; o++)
                    if (bfq_gzip_head17(w >> o) && bfq_gzip_cheap(in, len, byte * 8 + o)) mask |= 1u << o;
            }
            u64 lanes = __ballot(mask != 0);
            while (lanes && found == BFQ_GZIP_NONE) {                  // (uniform)
                const u32 l = (u32)__ffsll((long long)lanes) - 1;
                u32 m = (u32)__shfl((int)mask, (int)l);
                for (; m && found == BFQ_GZIP_NONE; m &= m - 1) {
                    const u64 bit = (at + l) * 8 + ((u32)__ffs((int)m) - 1);
                    int ok = 0;
                    if (lane == 0) ok = bfq_gzip_full(in, len, bit, &H[wave]) ? 1 : 0;
                    if (__shfl(ok, 0)) found = bit;
                }
                lanes &= lanes - 1;
            }
        }
        if (lane == 0) cand[k] = found;
    }
}

// Pass 1 (count).  Schedule as built: one wave64 per decoder -- piece 0 and every piece with a candidate -- four per
// workgroup, the Huffman tables of a wave in LDS (3.9 KiB).  All lanes read the same bits and decode the same symbols
// (uniform control flow, as in k_bgzf.hip); nothing is written but the decoder's record, by lane 0.  A decoder ends on a
// landing, at the stream's end or at an error, and at the latest where the input ends.
__global__ __launch_bounds__(64 * GZ_WAVES) void k_gzip_pass1(const u8 *__restrict__ in, u64 len, u64 chunk, const u64 *__restrict__ cand, u64 np,
                                                                 bfq_gzip_rec *recs)
{
    __shared__ bfq_bgzf_tables T[GZ_WAVES];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 k = (u64)blockIdx.x * GZ_WAVES + wave; k < np; k += (u64)gridDim.x * GZ_WAVES) {
        if (k && cand[k] == BFQ_GZIP_NONE) {
            if (lane == 0) { bfq_gzip_rec r{}; r.status = BFQ_GZIP_ST_NONE; recs[k] = r; }
            continue;
        }
        const bfq_gzip_job J{cand[k], 0, 0, 0, 0, 0, k == 0 ? 1u : 0u};
        bfq_gzip_run(in, len, chunk, cand, np, J, nullptr, nullptr, &T[wave], lane, 64, &recs[k]);
    }
}

// Pass 2 (decode).  Schedule as built: one wave64 per decoder of the chain, four per workgroup; the wave-uniform decode of
// k_bgzf.hip with lane-shared copies: lane 0 writes tables and literals, all 64 lanes share stored runs and matches
// (sym[p + i] = sym[p - d + i mod d], or the marker of the window byte where p - d + i mod d lies before the decoder's first
// symbol), with a workgroup-scope fence between a token's stores and the next match's loads.  A decoder writes its own
// symbols [outOff, outOff + produced) and its own member ends [endsOff, endsOff + nEnds), which pass 1 counted, and nothing else.
__global__ __launch_bounds__(64 * GZ_WAVES) void k_gzip_pass2(const u8 *__restrict__ in, u64 len, u64 chunk, const u64 *__restrict__ cand, u64 np,
                                                                 const bfq_gzip_job *__restrict__ jobs, u64 nj, u16 *sym, bfq_gzip_end *ends)
{
    __shared__ bfq_bgzf_tables T[GZ_WAVES];
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 j = (u64)blockIdx.x * GZ_WAVES + wave; j < nj; j += (u64)gridDim.x * GZ_WAVES) {
        const bfq_gzip_job J = jobs[j];
        bfq_gzip_rec r;
        bfq_gzip_run(in, len, chunk, cand, np, J, sym + J.outOff, ends + J.endsOff, &T[wave], lane, 64, &r);
    }
}

// Windows.  Schedule as built: ONE workgroup of 1024 threads and one loop over the chain -- the serial term of the call.  The
// window in front of the current decoder and the one being made lie in LDS (2 x 32 KiB, swapped by index).  Per decoder a
// thread makes 32 entries, four at a time: an entry is the decoder's symbol 32 KiB from its end, or the old window's byte
// where the decoder is shorter than that, a marker resolved through the old window; it goes to the new window and to the
// decoder's 32 KiB in global memory, for the resolve.  One barrier per decoder.
__global__ __launch_bounds__(1024) void k_gzip_windows(const u16 *__restrict__ sym, const bfq_gzip_job *__restrict__ jobs, u64 nj, u8 *W)
{
    __shared__ u8 win[2][BFQ_GZIP_WIN];
    for (u32 i = threadIdx.x * 4; i < BFQ_GZIP_WIN; i += 4096) {
        *(u32 *)&win[0][i] = 0;
        *(u32 *)&W[i] = 0;
    }
    __syncthreads();
    u32 cur = 0;
    for (u64 j = 0; j + 1 < nj; j++, cur ^= 1u) {
        const u16 *s = sym + jobs[j].outOff;
        const u64 produced = jobs[j].produced;
        u8 *dst = W + (j + 1) * BFQ_GZIP_WIN;
        for (u32 i = threadIdx.x * 4; i < BFQ_GZIP_WIN; i += 4096) {
            u32 v = 0;
            for (u32 t = 0; t < 4; t++) v |= (u32)bfq_gzip_window_sym(s, produced, win[cur], i + t) << (8 * t);
            *(u32 *)&win[cur ^ 1u][i] = v;
            *(u32 *)&dst[i] = v;
        }
        __syncthreads();
    }
}

// Resolve.  Schedule as built: one streaming pass, a workgroup of 256 threads per 4096 symbols, lane-consecutive (a wave
// loads 128 bytes of symbols and stores 64 bytes of text per step).  A thread finds the decoder of its first symbol by
// bisection over the chain's offsets and moves on from there.  Markers read the decoder's 32 KiB window (L2-resident).  A
// marker that reaches before its member's first byte puts its text position into *farPos by atomicMin.  out == nullptr:
// checks only.
#define GZ_RESOLVE_TILE 4096u
__global__ __launch_bounds__(256) void k_gzip_resolve(const u16 *__restrict__ sym, const bfq_gzip_job *__restrict__ jobs, u64 nj, const u8 *__restrict__ W,
                                                      u64 raw, u8 *out, u64 *farPos)
{
    for (u64 tile = blockIdx.x; tile * GZ_RESOLVE_TILE < raw; tile += gridDim.x) {
        u64 p = tile * GZ_RESOLVE_TILE + threadIdx.x;
        if (p >= raw) continue;
        u64 lo = 0, hi = nj;                                          // the last decoder that starts at or before p
        while (hi - lo > 1) {
            const u64 mid = (lo + hi) >> 1;
            if (jobs[mid].outOff <= p) lo = mid; else hi = mid;
        }
        u64 j = lo;
        for (u32 i = 0; i < GZ_RESOLVE_TILE / 256 && p < raw; i++, p += 256) {
            while (j + 1 < nj && jobs[j + 1].outOff <= p) j++;
            bool far = false;
            const u8 v = bfq_gzip_resolve_sym(sym[p], W + j * BFQ_GZIP_WIN, jobs[j].memberPre, &far);
            if (far) atomicMin((unsigned long long *)farPos, (unsigned long long)p);
            if (out) out[p] = v;
        }
    }
}

// CRC32 of the members.  Schedule as built: one thread per sub-range of 4096 text bytes, 64 threads per workgroup, the byte
// table in LDS.  A thread takes the serial CRC of its share of every member its range touches, multiplies it by
// x^(8 * bytes that follow in the member) mod P (bfq_crc32_shift) and XORs it into the member's word (atomicXor): the XOR of
// a member's shares is its CRC32.  The host compares with the trailers.
__global__ __launch_bounds__(64) void k_gzip_crc(const u8 *__restrict__ text, u64 raw, const bfq_gzip_end *__restrict__ ends, u64 nEnds, u32 *crc)
{
    __shared__ u32 tab[256];
    for (u32 i = threadIdx.x; i < 256; i += 64) tab[i] = bfq_crc32_entry(i);
    __syncthreads();
    for (u64 r = (u64)blockIdx.x * 64 + threadIdx.x; r * BFQ_GZIP_CRC_RANGE < raw; r += (u64)gridDim.x * 64)
        bfq_gzip_crc_range(tab, text, raw, r, ends, nEnds, [crc](u64 m, u32 v) { atomicXor(&crc[m], v); });
}

void bfq_gzip_launch_pass1(bfq_ctx *c, const u8 *d_in, u64 len, u64 chunk, u64 np, u64 *d_cand, bfq_gzip_rec *d_recs)
{
    KLAUNCH(c, K_BGZF, len, k_gzip_candidates, bfq_grid(np, GZ_WAVES), 64 * GZ_WAVES, d_in, len, chunk, np, d_cand);
    KLAUNCH(c, K_BGZF, len, k_gzip_pass1, bfq_grid(np, GZ_WAVES), 64 * GZ_WAVES, d_in, len, chunk, (const u64 *)d_cand, np, d_recs);
}
void bfq_gzip_launch_pass2(bfq_ctx *c, const u8 *d_in, u64 len, u64 chunk, u64 np, const u64 *d_cand, const bfq_gzip_job *d_jobs, u64 nj, u64 raw,
                           u16 *d_sym, bfq_gzip_end *d_ends, u8 *d_win, u8 *d_out, u64 *d_far)
{
    KLAUNCH(c, K_BGZF, raw, k_gzip_pass2, bfq_grid(nj, GZ_WAVES), 64 * GZ_WAVES, d_in, len, chunk, d_cand, np, d_jobs, nj, d_sym, d_ends);
    KLAUNCH(c, K_BGZF, nj * (u64)BFQ_GZIP_WIN, k_gzip_windows, 1, 1024, (const u16 *)d_sym, d_jobs, nj, d_win);
    if (raw) KLAUNCH(c, K_BGZF, raw, k_gzip_resolve, bfq_grid(raw, GZ_RESOLVE_TILE), 256, (const u16 *)d_sym, d_jobs, nj, (const u8 *)d_win, raw, d_out, d_far);
}
void bfq_gzip_launch_crc(bfq_ctx *c, const u8 *d_text, u64 raw, const bfq_gzip_end *d_ends, u64 nEnds, u32 *d_crc)
{
    if (raw && nEnds) KLAUNCH(c, K_BGZF, raw, k_gzip_crc, bfq_grid(ceil_div(raw, BFQ_GZIP_CRC_RANGE), 64), 64, d_text, raw, d_ends, nEnds, d_crc);
}
