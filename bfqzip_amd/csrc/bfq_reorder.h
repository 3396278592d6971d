// bfq_reorder.h -- the sort key of the read reordering (include/bfqzip_hip.h, bfq_fastq_reorder), shared by the host
// statement (bfq_reorder_key, bfq_host.cpp) and the kernels (k_reorder.hip).  Plain C++, no HIP types.
#pragma once
#include "bfq_common.h"

#define BFQ_RO_KEY_BITS 40
#define BFQ_RO_NOKEY ((1ull << BFQ_RO_KEY_BITS) - 1)     // a read without a window of k bases in ACGT
#define BFQ_RO_KMIN 8
#define BFQ_RO_KMAX 32
#define BFQ_RO_KDEF 21

// MurmurHash3's 64-bit finaliser
BFQ_HD u64 bfq_fmix64(u64 x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
// A 0, C 1, G 2, T 3; anything else (N, lower case, CR) 4: breaks the window
BFQ_HD u32 bfq_ro_code(u8 c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }
BFQ_HD u64 bfq_ro_mask(int k) { return k >= 32 ? ~0ull : (1ull << (2 * k)) - 1; }

// The windows of a sequence taken one base at a time: x holds the last k bases two bits each, run the number of
// consecutive bases in ACGT that end here; a window ends at this base when run >= k.
struct BfqRoRoll {
    u64 x; u32 run;
    u64 best; u32 found;                     // smallest hash of the windows so far
};
BFQ_HD void bfq_ro_init(BfqRoRoll &r) { r.x = 0; r.run = 0; r.best = ~0ull; r.found = 0; }
BFQ_HD void bfq_ro_push(BfqRoRoll &r, u32 code, int k, u64 mask, bool count)   // count: a window that ends here takes part
{
    r.run = code > 3u ? 0u : r.run + 1u;
    r.x = ((r.x << 2) | (code & 3u)) & mask;
    if (count && r.run >= (u32)k) {
        const u64 h = bfq_fmix64(r.x);
        if (h < r.best) r.best = h;
        r.found = 1;
    }
}
