// k_ubam.hip -- FASTQ texts as unaligned BAM records on the device: the sizing pass and the writing pass.  The text of both
// is bfq_ubam.h's (the same that runs on the host under sanitizers); the host side that orders them is bfq_ubam.hip.  No
// workgroup waits for another.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_ubam.h"

#define UBAM_WAVES 4
#define UBAM_RUN 8                                                 // consecutive records of one wave of the writing pass

// how the 64 lanes of a wave agree (all lanes of the wave are active wherever this is called)
struct ubam_wave {
    static __device__ __forceinline__ u32 first(bool v)
    {
        const u64 m = __ballot(v);
        return m ? (u32)__ffsll((long long)m) - 1u : 64u;
    }
    static __device__ __forceinline__ bool any(bool v) { return __ballot(v) != 0; }
};
static __device__ __forceinline__ u64 ubam_wave_sum(u64 v) { return __shfl(bfq_wave_incscan64(v), 63); }

// The sizing pass.  Schedule as built: one lane per record of the file, in file order (interleaved for pairs, text 0 behind),
// so that sizes[] is what the prefix sum places the records by.  A lane reads its read's header line (at most 256 bytes of
// it), with paired_check the mate's, one byte of the '+' line and the quality line, eight bytes at a time.  A refused read
// is reported through ONE atomicMin on (record index << 8 | reason): the lowest over all lanes is the offending record that
// would come first in the file.  The counts (named, comments) are summed over the wave and added by lane 0.  TAGS: the
// variant that walks the whole header line, a byte at a time, validates every field and adds the tags' stored bytes to the
// size; its tag counts go to *tcnt the same way.  Without TAGS neither G nor tcnt is touched.
template <bool TAGS>
__global__ __launch_bounds__(256) void k_ubam_size(bfq_ubam_job J, u64 nrec, u32 *__restrict__ sizes, u64 *firstBad, bfq_ubam_cnt *cnt, bfq_ubam_tagsel G,
                                                    bfq_ubam_tcnt *tcnt)
{
    bfq_ubam_cnt C{};
    bfq_ubam_tcnt T{};
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < nrec; r += (u64)gridDim.x * blockDim.x) {
        u32 k, size = 0;
        u64 i;
        bfq_ubam_where(J, r, &k, &i);
        const u32 why = bfq_ubam_size_read<TAGS>(J, k, i, &size, &C, &G, &T);
        sizes[r] = why ? 0u : size;
        if (why) atomicMin((unsigned long long *)firstBad, (unsigned long long)((r << 8) | why));
    }
    const u64 named = ubam_wave_sum(C.named), comments = ubam_wave_sum(C.comments);
    if (bfq_lane() == 0) {
        if (named) atomicAdd((unsigned long long *)&cnt->named, (unsigned long long)named);
        if (comments) atomicAdd((unsigned long long *)&cnt->comments, (unsigned long long)comments);
    }
    if (TAGS) {
        const u64 written = ubam_wave_sum(T.written), dropped = ubam_wave_sum(T.dropped), bytes = ubam_wave_sum(T.bytes);
        if (bfq_lane() == 0) {
            if (written) atomicAdd((unsigned long long *)&tcnt->written, (unsigned long long)written);
            if (dropped) atomicAdd((unsigned long long *)&tcnt->dropped, (unsigned long long)dropped);
            if (bytes) atomicAdd((unsigned long long *)&tcnt->bytes, (unsigned long long)bytes);
        }
    }
}

// The writing pass.  Schedule as built: wave w takes the records [UBAM_RUN w, UBAM_RUN (w + 1)) one after the other, four
// waves per workgroup: a wave's stores run through one contiguous stretch of the stream.  Inside a record the 64 lanes
// share its bytes as bfq_ubam_write_rec says: nine lanes the fixed fields, the name a byte per lane, SEQ four bytes (eight
// bases of text) and QUAL eight bytes per lane where the destination is aligned.  off[r]: where record r begins; off[nrec]:
// the stream's length.  A wave writes only inside its own records; the lanes' unknown bases are summed and added by lane 0.
// TAGS: the variant that cuts the header line at its tabs again (a ballot per 64 bytes) and writes the fields the sizing
// pass took between QUAL and the constant tag, a Z / H value's bytes lane-strided.
template <bool TAGS>
__global__ __launch_bounds__(64 * UBAM_WAVES) void k_ubam_write(bfq_ubam_job J, u64 nrec, const u64 *__restrict__ off, u8 *out, bfq_ubam_cnt *cnt, bfq_ubam_tagsel G)
{
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const u64 nruns = (nrec + UBAM_RUN - 1) / UBAM_RUN;
    u64 unknown = 0;
    for (u64 w = (u64)blockIdx.x * UBAM_WAVES + wave; w < nruns; w += (u64)gridDim.x * UBAM_WAVES) {
        const u64 r1 = (w + 1) * UBAM_RUN < nrec ? (w + 1) * UBAM_RUN : nrec;
        for (u64 r = w * UBAM_RUN; r < r1; r++) {
            u32 k;
            u64 i;
            bfq_ubam_where(J, r, &k, &i);
            const u64 o = off[r];
            bfq_ubam_write_rec<ubam_wave, TAGS>(out, o, (u32)(off[r + 1] - o), J, k, i, lane, 64, &unknown, &G);
        }
    }
    unknown = ubam_wave_sum(unknown);
    if (lane == 0 && unknown) atomicAdd((unsigned long long *)&cnt->unknown, (unsigned long long)unknown);
}

void bfq_ubam_launch_size(bfq_ctx *c, const bfq_ubam_job &J, u64 nrec, u32 *d_sizes, u64 *d_firstBad, bfq_ubam_cnt *d_cnt, const bfq_ubam_tagsel &G,
                          bfq_ubam_tcnt *d_tcnt)
{
    const u64 bytes = J.T.len[0] + J.T.len[1] + J.T.len[2];
    if (!nrec) return;
    if (G.on) KLAUNCH(c, K_UBAM_SIZE, bytes / 2 + 36 * nrec, k_ubam_size<true>, bfq_grid(nrec, 256), 256, J, nrec, d_sizes, d_firstBad, d_cnt, G, d_tcnt);
    else KLAUNCH(c, K_UBAM_SIZE, bytes / 2 + 36 * nrec, k_ubam_size<false>, bfq_grid(nrec, 256), 256, J, nrec, d_sizes, d_firstBad, d_cnt, G, d_tcnt);
}
void bfq_ubam_launch_write(bfq_ctx *c, const bfq_ubam_job &J, u64 nrec, const u64 *d_off, u8 *d_out, u64 rawLen, bfq_ubam_cnt *d_cnt, const bfq_ubam_tagsel &G)
{
    const u64 bytes = J.T.len[0] + J.T.len[1] + J.T.len[2] + rawLen + 40 * nrec;
    if (!nrec) return;
    if (G.on) KLAUNCH(c, K_UBAM_WRITE, bytes, k_ubam_write<true>, bfq_grid(nrec, UBAM_RUN * UBAM_WAVES), 64 * UBAM_WAVES, J, nrec, d_off, d_out, d_cnt, G);
    else KLAUNCH(c, K_UBAM_WRITE, bytes, k_ubam_write<false>, bfq_grid(nrec, UBAM_RUN * UBAM_WAVES), 64 * UBAM_WAVES, J, nrec, d_off, d_out, d_cnt, G);
}
