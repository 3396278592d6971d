// bfq_posbin.h -- geometry of the position-bin inversion (k_posbin.hip): plain C++, shared by host and device code.
//
// Row order -> text order is a permutation in which every text position occurs exactly once, so a radix partition on the
// position needs no counting pass: bin b of level 1 holds the positions [b << s1, (b + 1) << s1) and therefore exactly that
// many records, its base is arithmetic.  Level 2 cuts every level-1 bin into windows of BFQ_PB_W positions the same way, and
// one workgroup per window places the window's records in LDS and writes the window out in one piece.
#pragma once
#include "bfq_common.h"

#define BFQ_PB_WSHIFT 15                          // window: 32 Ki text positions (two 32 KiB byte arrays in LDS)
#define BFQ_PB_W (1u << BFQ_PB_WSHIFT)
#define BFQ_PB_MAX_BINS 512                       // bins of one partition level (LDS counters; ~8 records per bin and 4096-record tile)
#define BFQ_PB_MAX_SHIFT (BFQ_PB_WSHIFT + 9)      // a level-1 bin is at most 512 windows: 2^33 rows in all

// level-1 bin shift for n rows: the smallest s >= BFQ_PB_WSHIFT with at most BFQ_PB_MAX_BINS bins; -1: too many rows for two levels
BFQ_HD int bfq_posbin_shift(u64 n)
{
    if (!n) return BFQ_PB_WSHIFT;
    int s = BFQ_PB_WSHIFT;
    while (s <= BFQ_PB_MAX_SHIFT && ((n - 1) >> s) + 1 > (u64)BFQ_PB_MAX_BINS) s++;
    return s <= BFQ_PB_MAX_SHIFT ? s : -1;
}
BFQ_HD u64 bfq_posbin_bins(u64 n, int shift) { return n ? ((n - 1) >> shift) + 1 : 0; }     // bins (or windows) of 2^shift positions
// records of bin b = positions in it
BFQ_HD u64 bfq_posbin_cap(u64 n, int shift, u64 b)
{
    const u64 lo = b << shift;
    if (lo >= n) return 0;
    return n - lo < (1ull << shift) ? n - lo : (1ull << shift);
}
// the records: level 1 writes bfq_pack_val(position, final symbol code, final quality) (8 bytes), level 2 the position inside
// the window | code << 15 | quality << 18 (4 bytes)
BFQ_HD u32 bfq_posbin_rec4(u64 v) { return (u32)(bfq_val_pos(v) & (BFQ_PB_W - 1u)) | (bfq_val_code(v) << BFQ_PB_WSHIFT) | (bfq_val_qual(v) << (BFQ_PB_WSHIFT + 3)); }

// Write-combining (k_posbin_l1_wc; both levels in profiles/microbench/partition_wc.hip): a workgroup carries every bin's
// incomplete tail from tile to tile and writes whole 64-byte chunks only.  A bin is filled from both ends: whole chunks go up from its base through the head cursor (every claim
// is a multiple of the chunk, the base is one, so every chunk is aligned), the tails a workgroup is left with go down from the
// bin's end through the tail cursor.  Bin sizes are exact, so the two regions meet: head + tail = capacity afterwards.
#define BFQ_PB_CHUNK_BYTES 64u
BFQ_HD u32 bfq_posbin_chunk(int level) { return BFQ_PB_CHUNK_BYTES / (level == 1 ? 8u : 4u); }     // records per chunk
// a bin holds `carried` records of the tail and gets `fresh` ones from the tile: records flushed to the head / kept as the tail
BFQ_HD u32 bfq_posbin_head_claim(u32 carried, u32 fresh, u32 chunk) { return (carried + fresh) / chunk * chunk; }
BFQ_HD u32 bfq_posbin_tail_kept(u32 carried, u32 fresh, u32 chunk) { return (carried + fresh) % chunk; }
// slot inside a bin of cap records of the idx-th record the tail cursor handed out (idx < cap)
BFQ_HD u64 bfq_posbin_tail_slot(u64 cap, u64 idx) { return cap - 1 - idx; }

// Sparse form (the default): the outputs are the inputs with edits applied and the inputs are resident in the outputs' layout,
// so a row travels only if its final (symbol, quality) differs from a default the last kernel works out by itself at that
// position.  Two defaults ("polarities"), chosen per call on the device: KEEP = (input base, input quality), CONST = (input
// base, the constant v every smoothed quality becomes when M = 2); both binned when B = 1.  Rows whose symbol is the
// terminator are never sent.  The choice changes the number of rows sent, never the result.
#define BFQ_PB_KEEP 0
#define BFQ_PB_CONST 1
// forced: -1 = choose (CONST iff M = 2 and more than half of the bases were smoothed), else the polarity itself
BFQ_HD int bfq_posbin_polarity(int M, int forced, u64 smoothed, u64 bases)
{
    if (forced >= 0) return forced;
    return M == 2 && 2 * smoothed > bases ? BFQ_PB_CONST : BFQ_PB_KEEP;
}
BFQ_HD u32 bfq_posbin_default_qual(int polarity, int B, u32 inQual, u32 v)
{
    const u32 q = (polarity == BFQ_PB_CONST ? v : inQual) & 0xFFu;
    return B ? bfq_bin8(q) : q;
}
// Bins fill partially then: the live records of a bin of cap slots are its head region [0, head) and its tail region
// [cap - tail, cap); what lies between was never written and is not a record.
BFQ_HD bool bfq_posbin_live(u64 cap, u64 head, u64 tail, u64 idx) { return idx < cap && (idx < head || idx + tail >= cap); }
// slots [t0, t0 + len) of the bin hold no live record (wholly in the gap, or beyond the bin)
BFQ_HD bool bfq_posbin_gap_tile(u64 cap, u64 head, u64 tail, u64 t0, u64 len)
{
    const u64 end = t0 + len < cap ? t0 + len : cap;
    return t0 >= cap || (t0 >= head && end + tail <= cap);
}
// Terminators of a window as a bitmap (word w: window positions [64 w, 64 w + 64)) with pre[w] = terminators in the words
// below w: terminators strictly before window position idx.  A symbol's packed slot in the window's output is idx - that.
BFQ_HD bool bfq_posbin_is_term(const u64 *bm, u32 idx) { return (bm[idx >> 6] >> (idx & 63u)) & 1ull; }
BFQ_HD u32 bfq_posbin_term_rank(const u64 *bm, const u32 *pre, u32 idx)
{
    return pre[idx >> 6] + (u32)bfq_popc64(bm[idx >> 6] & ((1ull << (idx & 63u)) - 1ull));
}

// Terminated-text coordinates: read i stands at roff[i] + i, its terminator at roff[i + 1] + i.  Number of terminators
// strictly before position q = index of the read q lies in (a terminator belongs to the read it ends); q - that = where
// q's symbol goes when the reads are written back to back.
BFQ_HD u64 bfq_posbin_reads_before(const u64 *roff, u64 N, u64 q)
{
    u64 lo = 0, hi = N;                           // first i in [0, N] with roff[i + 1] + i >= q
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (roff[mid + 1] + mid < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}
