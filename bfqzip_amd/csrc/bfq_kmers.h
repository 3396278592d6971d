// bfq_kmers.h -- the k-mer spectrum report (include/bfqzip_hip.h, bfq_fastq_kmers*): what the device path (bfq_kmers.hip,
// k_kmers.hip) and the host form (bfq_kmers_host.cpp) share -- the options as taken, the constants of the layout, the cut of
// the 4096 bins into value ranges, the sort record.  Host and device: no HIP types here.
#pragma once
#include <stddef.h>
#include <vector>
#include "../../include/bfqzip_hip.h"
#include "bfq_common.h"

#define KM_TOP_BITS 12                                  // the bins of the value ranges: the top 12 bits of the 2k-bit k-mer
#define KM_BINS (1u << KM_TOP_BITS)
#define KM_STARTS 16                                    // start positions one lane owns: its bytes are 16 + k - 1 <= 46, four 16-byte loads
#define KM_GROUP 16                                     // lanes that share a read
#define KM_BATCH 64                                     // reads per workgroup and step (256 threads: 16 groups, four reads each)
#define KM_SEG_CHUNK 2048                               // sorted rows per workgroup where the runs are found (8 per thread)
#define KM_RUN_CHUNK 1024                               // runs per workgroup where they are counted and listed (4 per thread)
#define KM_MAX_PART ((1ull << 32) - 2)                  // records of one range: row numbers and B-counts are 32 bits wide

// The sort record of one window (12 bytes: bfq_common.h).  2k <= 40: the k-mer is the 40-bit key.  Above, lowBits = 2k - 40: as
// emitted the low bits are the key and the top 40 ride in the payload (km_record); k_km_rekey swaps them after the low round.
// In the final layout of both: k-mer = key40 << lowBits | (w1 & 0xFFFFFF), source = bit 0 of w2 (km_kmer).
BFQ_HD u32 km_low_bits(u32 k) { return 2 * k > 40 ? 2 * k - 40 : 0; }
BFQ_HD void km_record(u64 x, u32 src, u32 lowBits, u32 *w0, u64 *w12)
{
    const u64 key = lowBits ? x & ((1ull << lowBits) - 1) : x, hi40 = lowBits ? x >> lowBits : 0;
    const u32 w1 = (u32)(key & 0xFFu) << 24 | (u32)(hi40 >> 16), w2 = (u32)(hi40 & 0xFFFFu) << 16 | src;
    *w0 = (u32)(key >> 8);
    *w12 = (u64)w2 << 32 | w1;
}
BFQ_HD u64 km_kmer(u32 w0, u64 w12, u32 lowBits) { return ((u64)w0 << 8 | ((u32)w12 >> 24)) << lowBits | ((u32)w12 & 0xFFFFFFu); }

static inline const char *bfq_kmer_resolve(const bfq_kmer_opts *in, bfq_kmer_opts *O)   // nullptr: fine, else what is refused
{
    *O = bfq_kmer_opts{21, 3, 1, 0, 0};
    if (in) *O = *in;
    if (O->k < 8 || O->k > 31) return "k-mer report: k must be 8..31";
    if (O->solid < 2 || O->solid > 15) return "k-mer report: solid must be 2..15";
    if (O->reserved) return "k-mer report: reserved must be 0";
    O->canonical = O->canonical ? 1 : 0;
    return nullptr;
}

// The value ranges: [lo, hi) of bins, ascending, each with at least one record; a bin joins the range before it while the
// range's records stay within cap.  Empty bins end up inside or between ranges, which changes nothing.
struct KmRange { u32 lo, hi; u64 records; };
static inline std::vector<KmRange> bfq_kmer_ranges(const u64 *hist, u64 cap)
{
    std::vector<KmRange> R;
    u64 s = 0;
    u32 lo = 0;
    for (u32 b = 0; b < KM_BINS; b++) {
        if (!hist[b]) continue;
        if (s && s + hist[b] > cap) { R.push_back(KmRange{lo, b, s}); lo = b; s = 0; }
        s += hist[b];
    }
    if (s) R.push_back(KmRange{lo, KM_BINS, s});
    return R;
}

// one run of equal k-mers into the report's sums (the host form; the device's k_km_stats does the same with counters in LDS)
static inline u32 bfq_kmer_class(u64 c, u32 solid) { return c == 0 ? 0u : c < solid ? 1u : 2u; }
static inline bool bfq_kmer_listed(u64 ca, u64 cb, u32 solid)
{
    const u32 x = bfq_kmer_class(ca, solid), y = bfq_kmer_class(cb, solid);
    return (x == 2 && y == 0) || (x == 0 && y == 2);
}
