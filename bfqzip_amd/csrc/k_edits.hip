// k_edits.hip -- a run's base edits as the container BFQEDIT1 (include/bfqzip_hip.h; layout and arithmetic: bfq_edits.h): the
// kernels that make a member from the bases before and after a run, and the kernels that unpack one, validate it and write
// its bytes back.  bfq_edits.hip drives them.
//
// Both sides of a make lie where the caller has them: base arrays (read r at roff[r]), line streams (at roff[r] + r), or
// FASTQ texts with their record indexes (at rec[r].seqStart).  g = roff[r] + j numbers the bases of the collection.
//   k_edit_check  : one lane per read: the smallest read whose length differs between the sides (one atomic min), and the
//                   sum of fmix64(r 65536 + len) (`shape`)
//   k_edit_count  : 16 lanes per read, 8 bytes per lane and step (k_fq_gather's geometry): the differing bytes of a read.
//                   The last word of a read that is no multiple of 8 long overlaps the one before it; the bytes it shares
//                   with that word are masked out, so that no byte counts twice
//   k_edit_write  : the same walk again; a lane's first edit stands at the read's offset (the scan of the counts) + the edits
//                   of the read's sweeps before this one (carried) + those of the lanes before it in this sweep (a scan
//                   over the 16 lanes): ascending g whatever the length of the read.  `target_sum` is summed here
//   k_edit_segw   : one wave per segment of 1024 edits: its first position, the bit length of its largest gap, its words
//   k_edit_pack   : one lane per 64-bit word of the gaps
//   k_edit_unpack : one wave per segment: gaps -> positions by a wave scan, 64 at a time with the running position carried;
//                   what is wrong with the segment as a whole (a width that is not canonical, padding bits) is an atomic
//                   min on the index of its first edit
//   k_edit_locate : one lane per edit: out of range, not ascending, a byte outside 33..126 (atomic min on the edit's index);
//                   its read by binary search in the read offsets, where it lies in the target, the target's byte there
//                   into `target_sum`
//   k_edit_apply  : one lane per edit, one byte store
// All sums are sums of 64-bit integers mod 2^64: they do not depend on the launch geometry.
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_edits.h"

typedef unsigned long long ull;

__device__ __forceinline__ u64 ed_wave_sum(u64 v)
{
    for (int o = 32; o; o >>= 1) v += (u64)__shfl_xor((ull)v, o);
    return v;
}
__device__ __forceinline__ u64 ed_wave_max(u64 v)
{
    for (int o = 32; o; o >>= 1) { const u64 t = (u64)__shfl_xor((ull)v, o); v = t > v ? t : v; }
    return v;
}
__device__ __forceinline__ const u8 *ed_seq(const EdSide &s, const u64 *__restrict__ roff, u64 r)
{
    return s.rec ? s.buf + s.rec[r].seqStart : s.buf + roff[r] + (s.lines ? r : 0);
}
// bit 7 of every byte of x that is not zero
__device__ __forceinline__ u64 ed_nonzero_bytes(u64 x)
{
    const u64 m = 0x7F7F7F7F7F7F7F7Full;
    return (((x & m) + m) | x) & ~m;
}
// Word j of a read of L bases (j < ceil(L / 8), or j == 0 of a read shorter than 8): the 8 bytes of both sides at byte *k of
// the read, and the mask (bit 7 per byte) of the differing bytes that this word is the one to count.  Byte t of the word is
// base *k + t.
__device__ __forceinline__ u64 ed_word(const u8 *__restrict__ sa, const u8 *__restrict__ sb, u32 L, u32 j, u32 *k, u64 *wa, u64 *wb)
{
    if (L < 8) {                                                  // byte by byte: nothing is read past the read
        u64 a = 0, b = 0;
        for (u32 t = 0; t < L; t++) { a |= (u64)sa[t] << (8 * t); b |= (u64)sb[t] << (8 * t); }
        *k = 0; *wa = a; *wb = b;
        return ed_nonzero_bytes(a ^ b);
    }
    const u32 off = 8 * j;
    const bool whole = off + 8 <= L;
    const u32 at = whole ? off : L - 8;
    const u64 a = *(const u64 *)(sa + at), b = *(const u64 *)(sb + at);
    *k = at; *wa = a; *wb = b;
    u64 m = ed_nonzero_bytes(a ^ b);
    if (!whole) m &= ~0ull << (8 * (off - at));                   // the bytes below `off` belong to word j - 1 (0 < off - at < 8)
    return m;
}

__global__ __launch_bounds__(256) void k_edit_check(EdSide A, EdSide B, const u64 *__restrict__ roff, u64 rBase, u64 n, ull *__restrict__ badRead,
                                                    ull *__restrict__ shape)
{
    u64 sh = 0, bad = ~0ull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 r = rBase + i, len = roff[r + 1] - roff[r];
        if (((A.rec && A.rec[r].len != len) || (B.rec && B.rec[r].len != len) || len > BFQ_MAX_READ_LEN) && r < bad) bad = r;
        sh += bfq_edit_shape_term(i, len);
    }
    sh = ed_wave_sum(sh);
    if (bad != ~0ull) atomicMin(badRead, (ull)bad);
    if (bfq_lane() == 0 && sh) atomicAdd(shape, (ull)sh);
}

// WRITE: the second walk, which places the edits
template <bool WRITE>
__global__ __launch_bounds__(256) void k_edit_walk(EdSide A, EdSide B, const u64 *__restrict__ roff, u64 N, u32 *__restrict__ cnt,
                                                   const u64 *__restrict__ off, u64 *__restrict__ pos, u8 *__restrict__ byte, ull *__restrict__ sums)
{
    const u32 lane = bfq_lane(), sub = lane & 15u, grp = lane >> 4;
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    u64 touched = 0, tsum = 0;                                    // touched: wave-uniform; tsum: per lane
    for (u64 base = ((((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 2); base < N; base += nwaves << 2) {   // every lane of the wave makes every trip
        const u64 i = base + grp;
        const bool valid = i < N;
        u32 L = 0;
        u64 g0 = 0;
        const u8 *sa = nullptr, *sb = nullptr;
        if (valid) { g0 = roff[i]; L = (u32)(roff[i + 1] - g0); sa = ed_seq(A, roff, i); sb = ed_seq(B, roff, i); }
        const u32 nw = L >= 8 ? (L + 7) >> 3 : (L ? 1u : 0u);
        u32 have = nw;
        if (WRITE) have = valid && cnt[i] ? nw : 0u;               // a read without edits is not read again
        u32 mx = have;
        mx = max(mx, (u32)__shfl_xor((int)mx, 16));
        mx = max(mx, (u32)__shfl_xor((int)mx, 32));
        u32 c = 0;
        u64 at0 = WRITE && have ? off[i] : 0;
        for (u32 j0 = 0; j0 < mx; j0 += 16) {
            const u32 j = j0 + sub;
            u32 k = 0;
            u64 wa = 0, wb = 0, m = 0;
            if (j < have) m = ed_word(sa, sb, L, j, &k, &wa, &wb);
            const u32 n = (u32)__popcll(m);
            if (!WRITE) { c += n; continue; }
            u32 inc = n;                                          // inclusive scan over the 16 lanes of the read
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) { const u32 t = (u32)__shfl_up((int)inc, d, 16); if (sub >= (u32)d) inc += t; }
            const u32 tot = (u32)__shfl((int)inc, 15, 16);
            u64 at = at0 + inc - n;
            while (m) {
                const u32 t = (u32)__builtin_ctzll(m) >> 3;
                const u64 g = g0 + k + t;
                pos[at] = g;
                byte[at] = (u8)(wa >> (8 * t));
                tsum += bfq_edit_sum_term(g, (u32)(wb >> (8 * t)) & 255u);
                at++;
                m &= m - 1;
            }
            at0 += tot;
        }
        if (!WRITE) {
#pragma unroll
            for (int o = 8; o; o >>= 1) c += (u32)__shfl_xor((int)c, o);
            if (valid && sub == 0) cnt[i] = c;
            touched += __popcll(__ballot(valid && sub == 0 && c));
        }
    }
    if (WRITE) {
        tsum = ed_wave_sum(tsum);
        if (lane == 0 && tsum) atomicAdd(sums + 1, (ull)tsum);
    } else if (lane == 0 && touched) atomicAdd(sums, (ull)touched);
}

// per segment: its first position, its width, its words; the smallest edit whose byte is outside 33..126
__global__ __launch_bounds__(256) void k_edit_segw(const u64 *__restrict__ pos, const u8 *__restrict__ byte, u64 E, u64 nseg, u64 *__restrict__ first,
                                                   u8 *__restrict__ wt, u64 *__restrict__ words, ull *__restrict__ badEdit)
{
    const u32 lane = bfq_lane();
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 s = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < nseg; s += nwaves) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(E, s);
        u64 mx = 0, bad = ~0ull;
        for (u64 j = lane; j < c; j += 64) {
            if (j + 1 < c) { const u64 g = pos[k0 + j + 1] - pos[k0 + j] - 1; mx = g > mx ? g : mx; }
            if (!bfq_edit_byte_ok(byte[k0 + j]) && k0 + j < bad) bad = k0 + j;
        }
        mx = ed_wave_max(mx);
        if (bad != ~0ull) atomicMin(badEdit, (ull)bad);
        if (lane == 0) {
            const u32 w = bfq_edit_bitlen(mx);
            first[s] = pos[k0];
            wt[s] = (u8)w;
            words[s] = bfq_edit_seg_words(c, w);
        }
    }
}

__global__ __launch_bounds__(256) void k_edit_pack(const u64 *__restrict__ pos, u64 E, u64 nseg, const u8 *__restrict__ wt, const u64 *__restrict__ wordOff,
                                                   u64 *__restrict__ gaps)
{
    const u32 lane = bfq_lane();
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 s = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < nseg; s += nwaves) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(E, s);
        const u32 w = wt[s];
        const u64 nw = bfq_edit_seg_words(c, w), o = wordOff[s];
        for (u64 q = lane; q < nw; q += 64) gaps[o + q] = bfq_edit_word(pos + k0, c - 1, w, q);
    }
}

// the positions of a member, counted from its own first base
__global__ __launch_bounds__(256) void k_edit_unpack(const u64 *__restrict__ first, const u8 *__restrict__ wt, const u64 *__restrict__ gaps,
                                                     const u64 *__restrict__ wordOff, u64 E, u64 nseg, u64 *__restrict__ pos, ull *__restrict__ badEdit)
{
    const u32 lane = bfq_lane();
    const u64 nwaves = ((u64)gridDim.x * blockDim.x) >> 6;
    for (u64 s = ((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < nseg; s += nwaves) {
        const u64 k0 = s * BFQ_EDIT_SEG, c = bfq_edit_seg_count(E, s);
        const u32 w = wt[s];                                      // (<= 56: the host has looked at the table)
        const u64 nw = bfq_edit_seg_words(c, w);
        const u64 *__restrict__ wd = gaps + wordOff[s];
        u64 carry = first[s], mx = 0;
        for (u64 j0 = 0; j0 < c; j0 += 64) {                      // every lane makes every trip
            const u64 j = j0 + lane;
            u64 v = 0;
            if (j && j < c) { const u64 g = w ? bfq_edit_get(wd, j - 1, w) : 0; mx = g > mx ? g : mx; v = g + 1; }
            const u64 inc = bfq_wave_incscan64(v);
            if (j < c) pos[k0 + j] = carry + inc;
            carry += bfq_readlane64(inc, 63);
        }
        mx = ed_wave_max(mx);
        const u64 used = (c - 1) * w & 63;
        const bool segBad = bfq_edit_bitlen(mx) != w || (nw && used && wd[nw - 1] >> used);
        if (lane == 0 && segBad) atomicMin(badEdit, (ull)k0);
    }
}

// T, gBase, rBase: the member's bases, and where its bases and reads start in the target; sums[0] reads touched, sums[1] target_sum
__global__ __launch_bounds__(256) void k_edit_locate(const u64 *__restrict__ pos, const u8 *__restrict__ byte, u64 E, u64 T, u64 gBase, EdSide X,
                                                     const u64 *__restrict__ roff, u64 N, u64 *__restrict__ addr, ull *__restrict__ badEdit,
                                                     ull *__restrict__ sums)
{
    u64 tsum = 0, touched = 0, bad = ~0ull;
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < E; k += (u64)gridDim.x * blockDim.x) {
        const u64 g = pos[k], prev = k ? pos[k - 1] : 0;
        if ((g >= T || (k && g <= prev) || !bfq_edit_byte_ok(byte[k])) && k < bad) bad = k;
        if (g >= T) continue;
        const u64 G = gBase + g;                                  // (< roff[N]: the host has held the members' bases against the target's)
        u64 lo = 0, hi = N;
        while (lo < hi) {                                         // the read r with roff[r] <= G < roff[r + 1]
            const u64 mid = (lo + hi) >> 1;
            if (roff[mid + 1] <= G) lo = mid + 1; else hi = mid;
        }
        const u64 r = lo, j = G - roff[r];
        const u64 a = X.rec ? X.rec[r].seqStart + j : G + (X.lines ? r : 0);
        addr[k] = a;
        tsum += bfq_edit_sum_term(g, X.buf[a]);
        touched += !k || prev >= T || gBase + prev < roff[r];
    }
    tsum = ed_wave_sum(tsum);
    touched = ed_wave_sum(touched);
    if (bad != ~0ull) atomicMin(badEdit, (ull)bad);
    if (bfq_lane() == 0) {
        if (touched) atomicAdd(sums, (ull)touched);
        if (tsum) atomicAdd(sums + 1, (ull)tsum);
    }
}

__global__ __launch_bounds__(256) void k_edit_apply(const u64 *__restrict__ addr, const u8 *__restrict__ byte, u64 E, u8 *__restrict__ buf)
{
    for (u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x; k < E; k += (u64)gridDim.x * blockDim.x) buf[addr[k]] = byte[k];
}

// ---- launchers ------------------------------------------------------------------------------------------------------------
// The kernels that end in an atomic per wave run on a fixed number of workgroups and stride over their work: one workgroup
// per 16 reads made 750 000 waves at 3 M reads, and their adds to ONE word took 8.9 ms of a walk that takes 0.5 without.
#define ED_WALK_GRID 2048u                                        // 8 workgroups per CU: 32 waves, all resident
#define ED_CHECK_GRID 128u
#define ED_LOCATE_GRID 1024u
static unsigned ed_grid(u64 items, u64 perBlock, unsigned cap) { const unsigned g = bfq_grid(items, perBlock); return g < cap ? g : cap; }
void bfq_edit_check(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 rBase, u64 n, u64 *d_badRead, u64 *d_shape)
{
    if (!n) return;
    KLAUNCH(c, K_EDIT_CHECK, 48.0 * (double)n, k_edit_check, ed_grid(n, 256, ED_CHECK_GRID), 256, A, B, roff, rBase, n, (ull *)d_badRead, (ull *)d_shape);
}
void bfq_edit_count(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 total, u32 *cnt, u64 *d_sums)
{
    if (!N) return;
    KLAUNCH(c, K_EDIT_COUNT, 2.0 * (double)total + 60.0 * (double)N, (k_edit_walk<false>), ed_grid(N, 16, ED_WALK_GRID), 256, A, B, roff, N, cnt, (const u64 *)nullptr,
            (u64 *)nullptr, (u8 *)nullptr, (ull *)d_sums);
}
void bfq_edit_write(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 E, u32 *cnt, const u64 *off, u64 *pos, u8 *byte, u64 *d_sums)
{
    if (!N || !E) return;
    KLAUNCH(c, K_EDIT_WRITE, 20.0 * (double)N + 300.0 * (double)E, (k_edit_walk<true>), ed_grid(N, 16, ED_WALK_GRID), 256, A, B, roff, N, cnt, off, pos, byte, (ull *)d_sums);
}
void bfq_edit_segw(bfq_ctx *c, const u64 *pos, const u8 *byte, u64 E, u64 *first, u8 *wt, u64 *words, u64 *d_badEdit)
{
    const u64 nseg = bfq_edit_nseg(E);
    if (!nseg) return;
    KLAUNCH(c, K_EDIT_SEGW, 9.0 * (double)E, k_edit_segw, bfq_grid(nseg, 4), 256, pos, byte, E, nseg, first, wt, words, (ull *)d_badEdit);
}
void bfq_edit_pack(bfq_ctx *c, const u64 *pos, u64 E, const u8 *wt, const u64 *wordOff, u64 *gaps)
{
    const u64 nseg = bfq_edit_nseg(E);
    if (!nseg) return;
    KLAUNCH(c, K_EDIT_PACK, 16.0 * (double)E, k_edit_pack, bfq_grid(nseg, 4), 256, pos, E, nseg, wt, wordOff, gaps);
}
void bfq_edit_unpack(bfq_ctx *c, const u64 *first, const u8 *wt, const u64 *gaps, const u64 *wordOff, u64 E, u64 *pos, u64 *d_badEdit)
{
    const u64 nseg = bfq_edit_nseg(E);
    if (!nseg) return;
    KLAUNCH(c, K_EDIT_UNPACK, 16.0 * (double)E, k_edit_unpack, bfq_grid(nseg, 4), 256, first, wt, gaps, wordOff, E, nseg, pos, (ull *)d_badEdit);
}
void bfq_edit_locate(bfq_ctx *c, const u64 *pos, const u8 *byte, u64 E, u64 T, u64 gBase, EdSide X, const u64 *roff, u64 N, u64 *addr, u64 *d_badEdit,
                     u64 *d_sums)
{
    if (!E) return;
    KLAUNCH(c, K_EDIT_LOCATE, 200.0 * (double)E, k_edit_locate, ed_grid(E, 256, ED_LOCATE_GRID), 256, pos, byte, E, T, gBase, X, roff, N, addr, (ull *)d_badEdit, (ull *)d_sums);
}
void bfq_edit_apply(bfq_ctx *c, const u64 *addr, const u8 *byte, u64 E, u8 *buf)
{
    if (!E) return;
    KLAUNCH(c, K_EDIT_APPLY, 41.0 * (double)E, k_edit_apply, bfq_grid(E, 256), 256, addr, byte, E, buf);
}
