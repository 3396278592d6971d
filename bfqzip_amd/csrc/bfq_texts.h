// bfq_texts.h -- the plain FASTQ texts of a call (up to three) on their way to the device, as a plan: which of them are
// copied into the context's text buffer, where, and how long they are there; and the arena bytes of the line kernels that
// read them (k_fastq.hip), stated once beside the allocations they stand for.  Host-only: no HIP types here.
// The device half -- looking at the texts, placing them, counting their lines -- is bfq_io.hip's.
#pragma once
#include <stddef.h>
#include "bfq_common.h"

#define BFQ_MAX_TEXTS 3
#define BFQ_NL_CHUNK 4096                              // text bytes per workgroup iteration of the line kernels (16 per thread)
#define BFQ_SCAN_CHUNK 4096                            // items per workgroup of the prefix sums: a copy of k_scan.hip's SC_CHUNK
                                                       // (SC_THREADS * SC_ITEMS) that no assert ties to it yet -- change both
#define BFQ_FQREC_BYTES 32                             // sizeof(FqRec) (k_fastq.hip asserts it)

static inline size_t bfq_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// ---------------------------------------------------------------- the plan
// one input text as already looked at (bfq_texts_look)
struct BfqTextSeen {
    bool present = false, device = false;              // given at all; in device memory (else: host memory or a file)
    uintptr_t addr = 0;                                // device texts: the address (the line kernels load 16 aligned bytes)
    u64 len = 0;
    u8 first[2] = {0, 0};                              // its first two bytes (len >= 2), for the callers' gzip refusals
    u8 last = 10;                                      // its last byte; an empty text counts as ending in LF
};
struct BfqTextPlan {
    struct Slot { bool present = false, moves = false; u64 len = 0; size_t off = 0; };   // len: as staged; off: in the text buffer (moves)
    Slot t[BFQ_MAX_TEXTS];
    size_t bufNeed = 0;                                // bytes of the text buffer: the end of the last slot
};
static inline size_t bfq_text_slot_bytes(u64 len) { return ((size_t)len + 64 + 255) & ~(size_t)255; }   // padded for 16-byte loads, 256-byte aligned

// addLf: a text whose last byte is no LF gets one behind it.  A host or file text always moves; a device text stays where it
// lies unless its address is no multiple of 16, it gains its LF (in the copy), or it is empty (its pointer may be anything:
// it gets a slot that can be read).  An absent text takes nothing.  (Callers for which an empty text means "no records" hand
// it in as absent.)
static inline BfqTextPlan bfq_texts_plan(const BfqTextSeen *seen, int n, bool addLf)
{
    BfqTextPlan P;
    for (int k = 0; k < n && k < BFQ_MAX_TEXTS; k++) {
        const BfqTextSeen &s = seen[k];
        BfqTextPlan::Slot &t = P.t[k];
        if (!s.present) continue;
        const bool gains = addLf && s.len && s.last != 10;
        t.present = true;
        t.len = s.len + (gains ? 1 : 0);
        t.moves = !s.device || (s.addr & 15u) || gains || !s.len;
        if (!t.moves) continue;
        t.off = P.bufNeed;
        P.bufNeed += bfq_text_slot_bytes(t.len);
    }
    return P;
}

// ---------------------------------------------------------------- arena bytes of the line kernels
// bfq_exscan_*() over n items: two partial sums per workgroup, level by level (k_scan.hip)
static inline size_t bfq_scan_bytes(u64 n)
{
    size_t s = 0;
    while (n > BFQ_SCAN_CHUNK) {
        n = (n + BFQ_SCAN_CHUNK - 1) / BFQ_SCAN_CHUNK;
        s += 2 * bfq_align256(8 * (size_t)n);
    }
    return s;
}
static inline u64 bfq_nl_chunks(u64 len) { return ((len ? len : 1) + BFQ_NL_CHUNK - 1) / BFQ_NL_CHUNK; }

// The buffers of bfq_fastq_count_lines() and bfq_line_index(): newlines per chunk, their prefix sums, the total -- and the line
// ends, once the total is known.  A: an Arena (bfq_arena.h), or a context that allocates like one.
struct BfqNlBufs { u32 *counts; u64 *bases, *total; u64 nchunks; };
template <class A> static BfqNlBufs bfq_nl_alloc(A &a, u64 len)
{
    BfqNlBufs b;
    b.nchunks = bfq_nl_chunks(len);
    b.counts = (u32 *)a.alloc(4 * (size_t)b.nchunks);
    b.bases = (u64 *)a.alloc(8 * (size_t)b.nchunks);
    b.total = (u64 *)a.alloc(8);
    return b;
}
template <class A> static u64 *bfq_nl_alloc_ends(A &a, u64 newlines) { return (u64 *)a.alloc(8 * ((size_t)newlines + 2)); }

// ... and what they take, from wherever the arena's top stands (256: its alignment).  lines: as bfq_fastq_count_lines()
// returns them, newlines + 1.
static inline size_t bfq_count_lines_bytes(u64 len)
{
    const size_t nc = (size_t)bfq_nl_chunks(len);
    return 256 + bfq_align256(4 * nc) + bfq_align256(8 * nc) + 256 + bfq_scan_bytes(nc);
}
static inline size_t bfq_line_index_bytes(u64 len, u64 lines) { return bfq_count_lines_bytes(len) + bfq_align256(8 * ((size_t)lines + 2)); }
// bfq_fastq_index(): the line index, and per record its FqRec, read offset and length, and the scan over the lengths
static inline size_t bfq_fastq_index_bytes(u64 len, u64 lines)
{
    const size_t N = (size_t)(lines / 4);
    return bfq_line_index_bytes(len, lines) + bfq_align256(BFQ_FQREC_BYTES * (N + 1)) + bfq_align256(8 * (N + 2)) + bfq_align256(4 * (N + 1)) + bfq_scan_bytes(N);
}
