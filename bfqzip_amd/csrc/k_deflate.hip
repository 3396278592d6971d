// k_deflate.hip -- BGZF members written on the device: one wave64 per member, one member at a time per 64-thread workgroup.
//
// The text of the writer is bfq_deflate.h's (the same that runs on the host under sanitizers, and gives the same bytes).
// Schedule as built:
//   - the hash table, the histograms, the codes and the construction's scratch of the member live in LDS (bfq_defl_work,
//     24 KiB: six workgroups per CU by LDS), the tokens in a workspace row of the workgroup (65 280 words), the text is read
//     where it lies;
//   - all 64 lanes search (one position of a 64-position step each), insert into the table (atomicMax), take the CRC32 over
//     64 equal sub-ranges and pack the bits of an equal share of the tokens (atomicOr into the zeroed slot);
//   - lane 0 alone selects the tokens of a step from LDS, builds the three codes and writes the block header;
//   - no loop waits for another workgroup: every one runs to the member's length or to a constant.
// A member goes into its own slot of BFQ_DEFL_SLOT bytes (piece + 31, in whole words); k_bgzf_gather moves the slots to where
// a scan of their sizes puts them.
#include "bfq_internal.h"
#include "bfq_deflate.h"

__global__ __launch_bounds__(64) void k_bgzf_deflate(const u8 *__restrict__ in, u64 len, u64 nm, int level, u8 *__restrict__ slots,
                                                     u32 *__restrict__ sizes, u32 *__restrict__ tokAll)
{
    __shared__ bfq_defl_work W;
    __shared__ u32 crcTab[256];
    for (u32 i = threadIdx.x; i < 256; i += 64) crcTab[i] = bfq_crc32_entry(i);
    __syncthreads();
    const u32 lane = threadIdx.x;
    u32 *tok = tokAll + (u64)blockIdx.x * BFQ_DEFL_PIECE;
    for (u64 m = blockIdx.x; m < nm; m += gridDim.x) {
        const u64 off = m * BFQ_DEFL_PIECE;
        const u32 n = (u32)(len - off < BFQ_DEFL_PIECE ? len - off : BFQ_DEFL_PIECE);
        const u32 size = bfq_defl_member(in + off, n, level, slots + m * BFQ_DEFL_SLOT, BFQ_DEFL_SLOT, tok, &W, crcTab, lane, 64);
        if (lane == 0) sizes[m] = size;
    }
}

// member m: sizes[m] bytes of its slot to out + offs[m]; the last workgroup appends `tail` bytes (the EOF member) behind them
__global__ __launch_bounds__(256) void k_bgzf_gather(const u8 *__restrict__ slots, const u32 *__restrict__ sizes, const u64 *__restrict__ offs, u64 nm,
                                                     u8 *__restrict__ out, u32 tail)
{
    for (u64 m = blockIdx.x; m < nm; m += gridDim.x) {
        const u8 *s = slots + m * BFQ_DEFL_SLOT;
        u8 *d = out + offs[m];
        const u32 n = sizes[m] < BFQ_DEFL_SLOT ? sizes[m] : BFQ_DEFL_SLOT;
        for (u32 i = threadIdx.x; i < n; i += 256) d[i] = s[i];
        if (m == nm - 1)
            for (u32 i = threadIdx.x; i < tail; i += 256) d[n + i] = bfq_defl_eof_byte(i);
    }
}

// workgroups of a launch over nm members, and the words of token workspace they take
unsigned bfq_deflate_grid(u64 nm) { return (unsigned)(nm < 1536 ? (nm ? nm : 1) : 1536); }   // 256 CUs x 6 resident workgroups
u64 bfq_deflate_tok_words(u64 nm) { return (u64)bfq_deflate_grid(nm) * BFQ_DEFL_PIECE; }

void bfq_deflate_launch(bfq_ctx *c, const u8 *d_in, u64 len, int level, u8 *d_slots, u32 *d_sizes, u32 *d_tok)
{
    const u64 nm = bfq_defl_members(len);
    if (!nm) return;
    KLAUNCH(c, K_DEFLATE, len, k_bgzf_deflate, bfq_deflate_grid(nm), 64, d_in, len, nm, level, d_slots, d_sizes, d_tok);
}
void bfq_deflate_gather(bfq_ctx *c, const u8 *d_slots, const u32 *d_sizes, const u64 *d_offs, u64 nm, u8 *d_out, bool eof)
{
    if (!nm) return;
    KLAUNCH(c, K_MISC, 2.0 * BFQ_DEFL_PIECE * (double)nm, k_bgzf_gather, bfq_grid(nm, 1), 256, d_slots, d_sizes, d_offs, nm, d_out,
            eof ? BFQ_BGZF_EOF_LEN : 0u);
}
