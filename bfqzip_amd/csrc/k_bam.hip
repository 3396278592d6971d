// k_bam.hip -- BAM records to FASTQ text on the device: the candidate search, the counting walk, the placing walk and the
// pairing check.  The text of every step is bfq_bam.h's (the same that runs on the host under sanitizers); the host side
// that orders them is bfq_bam.hip.  No workgroup waits for another; all launches are booked under the BGZF kernel class.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_bam.h"

#define BAM_WAVES 4

// how the 64 lanes of a wave agree about a tag's bytes (all lanes of the wave are active wherever this is called)
struct bam_wave {
    static __device__ __forceinline__ u32 first(bool v)
    {
        const u64 m = __ballot(v);
        return m ? (u32)__ffsll((long long)m) - 1u : 64u;
    }
    static __device__ __forceinline__ bool any(bool v) { return __ballot(v) != 0; }
};

// Candidates and the counting walk.  Schedule as built: one wave64 per piece, four pieces per 256-thread workgroup.  The wave
// goes through its piece 64 offsets at a time -- every lane tries the record-start rule at one offset; nearly all fail on
// the four bytes of the block size -- and takes the lowest that passes (ballot).  From there all lanes hop together
// (bfq_bam_walk: uniform control flow, the same loads in every lane) and share only the quality bytes, lane-consecutive,
// for the count of clamped values.  Lane 0 writes the piece's record.  `only` != NONE: the walk of that one piece from
// `from` (a repair round).  TAGS: the variant that parses the tag area of every kept record as well (bfq_bam_tags_count: the
// same few loads in every lane; the bytes of a Z / H value shared, its NUL found with one ballot per 64 bytes) and writes
// the piece's tag counts to tagc[k]; without TAGS neither G nor tagc is touched and the walk is what it was.
template <bool TAGS>
__global__ __launch_bounds__(64 * BAM_WAVES) void k_bam_walk(const u8 *__restrict__ s, u64 len, u64 hdrEnd, u64 piece, u64 np, u32 nref, bfq_bam_opts O,
                                                              u64 only, u64 from, bfq_bam_piece *recs, bfq_bam_tagsel G, bfq_bam_tagcnt *tagc)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const bool repair = only != BFQ_BAM_NONE;
    for (u64 k = repair ? (wave == 0 ? only : np) : (u64)blockIdx.x * BAM_WAVES + wave; k < np; k += repair ? np : (u64)gridDim.x * BAM_WAVES) {
        const u64 lo = hdrEnd + k * piece, hi = lo + piece < len ? lo + piece : len;
        u64 start = only != BFQ_BAM_NONE ? from : k ? BFQ_BAM_NONE : hdrEnd;
        for (u64 at = lo; start == BFQ_BAM_NONE && at < hi; at += 64) {
            const u64 o = at + lane;
            const u64 hit = __ballot(o < hi && bfq_bam_candidate(s, len, o, nref));
            if (hit) start = at + (u64)(__ffsll((long long)hit) - 1);
        }
        bfq_bam_piece P{};
        bfq_bam_tagcnt T{};
        P.start = BFQ_BAM_NONE;
        if (start != BFQ_BAM_NONE) {
            const u64 mine = bfq_bam_walk<TAGS, bam_wave>(s, len, start, hi, nref, O, lane, 64, &P, &G, &T);
            P.clamped = bfq_wave_incscan64(mine);                  // (lane 63 holds the wave's sum)
            P.clamped = __shfl(P.clamped, 63);
        }
        if (lane == 0) recs[k] = P;
        if (TAGS && lane == 0) tagc[k] = T;
    }
}

// The placing walk.  Schedule as built: one wave64 per piece of the chain, four per workgroup.  The wave hops over its
// records as the counting walk did and writes every kept record's text at the place the prefix sums gave it: lane i takes
// bytes i, i + 64, ... of the name, of the bases (a nibble each) and of the qualities, so a wave's stores are 64
// consecutive bytes and no lane writes a record alone.  A wave writes its own [byteBase, byteBase + bytes) and nothing else.
// TAGS: the variant that writes the selected tags behind the name (bfq_bam_tags_emit: a Z / H value copied lane-strided, the
// six bytes in front of a value and an integer's digits by lane 0).
template <bool TAGS>
__global__ __launch_bounds__(64 * BAM_WAVES) void k_bam_place(const u8 *__restrict__ s, u64 len, const bfq_bam_job *__restrict__ jobs, u64 nj, u32 nref,
                                                               bfq_bam_opts O, bfq_bam_outs out, bfq_bam_tagsel G)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 j = (u64)blockIdx.x * BAM_WAVES + wave; j < nj; j += (u64)gridDim.x * BAM_WAVES)
        bfq_bam_place<TAGS, bam_wave>(s, len, jobs[j], nref, O, out, lane, 64, &G);
}

// The pairing check.  Schedule as built: one thread per pair; the lowest pair whose names differ by atomicMin.
__global__ __launch_bounds__(256) void k_bam_pairs(const u8 *__restrict__ s, const u64 *__restrict__ a, const u64 *__restrict__ b, u64 n, u64 *firstBad)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256)
        if (!bfq_bam_same_name(s, a[i], b[i])) atomicMin((unsigned long long *)firstBad, (unsigned long long)i);
}

void bfq_bam_launch_walk(bfq_ctx *c, const u8 *d_s, u64 len, u64 hdrEnd, u64 piece, u64 np, u32 nref, const bfq_bam_opts &O, u64 only, u64 from,
                         bfq_bam_piece *d_recs, const bfq_bam_tagsel &G, bfq_bam_tagcnt *d_tagc)
{
    const u32 grid = only == BFQ_BAM_NONE ? bfq_grid(np, BAM_WAVES) : 1u;
    const u64 bytes = only == BFQ_BAM_NONE ? len : piece;
    if (G.on) KLAUNCH(c, K_BGZF, bytes, k_bam_walk<true>, grid, 64 * BAM_WAVES, d_s, len, hdrEnd, piece, np, nref, O, only, from, d_recs, G, d_tagc);
    else KLAUNCH(c, K_BGZF, bytes, k_bam_walk<false>, grid, 64 * BAM_WAVES, d_s, len, hdrEnd, piece, np, nref, O, only, from, d_recs, G, d_tagc);
}
void bfq_bam_launch_place(bfq_ctx *c, const u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_outs &out, u64 bytes,
                          const bfq_bam_tagsel &G)
{
    if (!nj) return;
    if (G.on) KLAUNCH(c, K_BGZF, len + bytes, k_bam_place<true>, bfq_grid(nj, BAM_WAVES), 64 * BAM_WAVES, d_s, len, d_jobs, nj, nref, O, out, G);
    else KLAUNCH(c, K_BGZF, len + bytes, k_bam_place<false>, bfq_grid(nj, BAM_WAVES), 64 * BAM_WAVES, d_s, len, d_jobs, nj, nref, O, out, G);
}
void bfq_bam_launch_pairs(bfq_ctx *c, const u8 *d_s, const u64 *d_a, const u64 *d_b, u64 n, u64 *d_firstBad)
{
    if (n) KLAUNCH(c, K_BGZF, n * 80, k_bam_pairs, bfq_grid(n, 256), 256, d_s, d_a, d_b, n, d_firstBad);
}
