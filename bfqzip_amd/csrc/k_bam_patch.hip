// k_bam_patch.hip -- FASTQ text back into BAM records on the device: the checking walk and the patching walk.  The text of
// both is bfq_bam_patch.h's (the same that runs on the host under sanitizers); the host side that orders them is
// bfq_bam_patch.hip.  No workgroup waits for another; all launches are booked under the BGZF kernel class.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_bam_patch.h"

#define BAMP_WAVES 4

// how the 64 lanes of a wave agree (all lanes of the wave are active wherever these are called)
struct bamp_wave {
    static __device__ __forceinline__ bool all(bool v) { return __all(v) != 0; }
    static __device__ __forceinline__ bool any(bool v) { return __any(v) != 0; }
};
static __device__ __forceinline__ u64 bamp_wave_sum(u64 v) { return __shfl(bfq_wave_incscan64(v), 63); }

// The checking walk.  Schedule as built: one wave64 per piece of the chain, four per workgroup.  The wave hops over its
// records as the placing walk does -- uniform control flow, the same loads in every lane -- and compares every kept
// record's l_seq with the lengths of its read's two lines; with check_names the lanes share the name's bytes and vote.  A
// wave stops at its first offending record; lane 0 puts that record's offset into *firstBad (atomicMin: the lowest over
// all waves).  only != NONE: the walk of that one piece again, which writes what it found to *err.  Nothing is written else.
__global__ __launch_bounds__(64 * BAMP_WAVES) void k_bam_patch_check(const u8 *__restrict__ s, u64 len, const bfq_bam_job *__restrict__ jobs, u64 nj, u32 nref,
                                                                      bfq_bam_opts O, bfq_bam_texts T, u64 only, u64 *firstBad, bfq_bamp_err *err)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (only != BFQ_BAM_NONE) {
        if (wave) return;
        bfq_bamp_err E;
        bfq_bam_patch_check<bamp_wave>(s, len, jobs[only], nref, O, T, lane, 64, &E);
        if (lane == 0) *err = E;
        return;
    }
    for (u64 j = (u64)blockIdx.x * BAMP_WAVES + wave; j < nj; j += (u64)gridDim.x * BAMP_WAVES) {
        bfq_bamp_err E;
        const u64 bad = bfq_bam_patch_check<bamp_wave>(s, len, jobs[j], nref, O, T, lane, 64, &E);
        if (bad != BFQ_BAM_NONE && lane == 0) atomicMin((unsigned long long *)firstBad, (unsigned long long)bad);
    }
}

// The patching walk.  Schedule as built: one wave64 per piece of the chain, four per workgroup, in place on the stream.
// Per record lane b owns bytes b, b + 64, ... of SEQ -- two bases each, read from the text as neighbouring bytes -- and
// bytes b, b + 64, ... of QUAL: no two lanes write one byte, and a wave's loads and stores are lane-consecutive.  The keep
// rule for absent qualities is one wave vote per such record before the qualities are stored; whether the read changed is
// another.  A wave writes only inside SEQ and QUAL of its own piece's kept records (plain byte stores); its counts are
// summed over the lanes and written by lane 0 into the piece's record.
__global__ __launch_bounds__(64 * BAMP_WAVES) void k_bam_patch(u8 *s, u64 len, const bfq_bam_job *__restrict__ jobs, u64 nj, u32 nref, bfq_bam_opts O,
                                                                bfq_bam_texts T, bfq_bamp_cnt *cnt)
{
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 j = (u64)blockIdx.x * BAMP_WAVES + wave; j < nj; j += (u64)gridDim.x * BAMP_WAVES) {
        bfq_bamp_cnt C{};
        bfq_bam_patch_job<bamp_wave>(s, len, jobs[j], nref, O, T, lane, 64, &C);
        C.readsChanged = bamp_wave_sum(C.readsChanged); C.basesChanged = bamp_wave_sum(C.basesChanged); C.qualsChanged = bamp_wave_sum(C.qualsChanged);
        C.unknown = bamp_wave_sum(C.unknown); C.keptHigh = bamp_wave_sum(C.keptHigh); C.keptAbsent = bamp_wave_sum(C.keptAbsent);
        C.reversed = bamp_wave_sum(C.reversed);
        if (lane == 0) cnt[j] = C;
    }
}

void bfq_bam_launch_patch_check(bfq_ctx *c, const u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T,
                                u64 only, u64 *d_firstBad, bfq_bamp_err *d_err)
{
    const u64 bytes = len + T.len[0] + T.len[1] + T.len[2];
    if (nj) KLAUNCH(c, K_BGZF, only == BFQ_BAM_NONE ? bytes : O.piece, k_bam_patch_check, only == BFQ_BAM_NONE ? bfq_grid(nj, BAMP_WAVES) : 1u, 64 * BAMP_WAVES, d_s, len,
                    d_jobs, nj, nref, O, T, only, d_firstBad, d_err);
}
void bfq_bam_launch_patch(bfq_ctx *c, u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_texts &T, bfq_bamp_cnt *d_cnt)
{
    const u64 bytes = len + T.len[0] + T.len[1] + T.len[2];
    if (nj) KLAUNCH(c, K_BGZF, bytes, k_bam_patch, bfq_grid(nj, BAMP_WAVES), 64 * BAMP_WAVES, d_s, len, d_jobs, nj, nref, O, T, d_cnt);
}
