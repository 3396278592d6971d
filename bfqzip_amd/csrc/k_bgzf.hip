// k_bgzf.hip -- BGZF members inflated on the device: one wave64 per member, four members per 256-thread workgroup.
//
// The text of the inflate is bfq_bgzf.h's (the same that runs on the host under sanitizers).  Schedule as built:
//   - every lane of a wave reads the same bits and decodes the same symbols (uniform control flow, the bit buffer in
//     registers, the Huffman tables of the wave in LDS: 3.9 KiB, read at one address by all lanes = a broadcast);
//   - lane 0 writes the tables and the literals; all 64 lanes share the copies: stored runs, matches
//     (out[p + i] = out[p - d + i mod d], so overlapping matches replicate), and the CRC32 over 64 equal sub-ranges of the
//     finished member, combined by x^(8 len) mod P;
//   - a match reads bytes that other lanes stored for earlier tokens: a workgroup-scope fence stands between (BFQ_BGZF_SYNC).
// A member that is refused puts (member << 8 | reason) into *status by atomicMin: the lowest failing member wins, and the
// host reads one word per call.  Nothing is written outside [out_off, out_off + ISIZE) of a member, whatever its payload holds.
#include "bfq_internal.h"
#include "bfq_bgzf.h"

#define BGZF_WAVES 4

__global__ __launch_bounds__(64 * BGZF_WAVES) void k_bgzf_inflate(const u8 *__restrict__ in, const bfq_bgzf_member *__restrict__ dir, u64 nm,
                                                                   u8 *out, u64 *status)
{
    __shared__ bfq_bgzf_tables T[BGZF_WAVES];
    __shared__ u32 crcTab[256];
    crcTab[threadIdx.x] = bfq_crc32_entry(threadIdx.x);
    __syncthreads();
    const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (u64 m = (u64)blockIdx.x * BGZF_WAVES + wave; m < nm; m += (u64)gridDim.x * BGZF_WAVES) {
        const bfq_bgzf_member d = dir[m];
        bfq_bgzf_hdr h;
        int r = bfq_bgzf_member_header(in + d.in_off, d.in_len, &h);
        if (!r && (h.total != d.in_len || h.isize != d.out_len)) r = BFQ_BGZF_E_TOTAL;    // (the host read the same bytes)
        if (!r) r = bfq_bgzf_inflate_payload(in + d.in_off + h.payOff, h.payLen, out + d.out_off, h.isize, h.crc, &T[wave], crcTab, lane, 64);
        if (r && lane == 0) atomicMin(status, (m << 8) | (u64)r);
    }
}

// a text that lacks its final newline gets one (room was left); *flag = 1 then
__global__ void k_bgzf_newline(u8 *text, u64 len, u64 *flag)
{
    if (len && text[len - 1] != (u8)'\n') { text[len] = (u8)'\n'; *flag = 1; }
}
void bfq_bgzf_newline(bfq_ctx *c, u8 *d_text, u64 len, u64 *d_flag)
{
    KLAUNCH(c, K_MISC, 1, k_bgzf_newline, 1, 1, d_text, len, d_flag);
}

void bfq_bgzf_launch(bfq_ctx *c, const u8 *d_in, const void *d_dir, u64 nm, u8 *d_out, u64 rawLen, u64 *d_status)
{
    if (!nm) return;
    KLAUNCH(c, K_BGZF, rawLen, k_bgzf_inflate, bfq_grid(nm, BGZF_WAVES), 64 * BGZF_WAVES, d_in, (const bfq_bgzf_member *)d_dir, nm, d_out, d_status);
}
