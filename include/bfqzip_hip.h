/*
 * bfqzip_hip.h -- C-ABI of libbfqhip.so: the MI355X (gfx950) implementation of
 * BFQzip's hot path  eBWT build -> positional clusters -> smoothing -> LF inversion.
 *
 * The reference has no in-process API for this path: its boundary is the
 * process boundary between the Python drivers and four executables
 * (BFQzip.py:178-189,206-228; BFQzip_ext.py:165-183,199-220).  The entry points
 * below are what those executables' main() functions reduce to once file I/O is
 * taken out; the drop-in front-ends in bfqzip_amd/csrc/cli/ (gsufsort, eGap,
 * bfq_int, bfq_ext) are thin argv/file wrappers over them.
 *
 * Conventions: plain pointers and sizes, no torch types.  Every function
 * returns 0 on success and a negative BFQ_E_* code on failure;
 * bfq_last_error() gives the message.  A context owns one GPU stream and one
 * device workspace; it is not thread-safe, use one context per thread/GPU.
 * "h_" = host pointer, "d_" = device pointer (hipMalloc'ed / torch storage).
 */
#ifndef BFQZIP_HIP_H
#define BFQZIP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BFQ_OK              0
#define BFQ_E_ARG          -1   /* bad argument                                            */
#define BFQ_E_HIP          -2   /* HIP runtime error / no device                           */
#define BFQ_E_SYMBOL       -3   /* symbol outside {A,C,G,T,N,TERM} (dna_string_n.hpp:87-93) */
#define BFQ_E_NOT_EBWT     -4   /* eBWT does not invert / not in #_i<#_j<A<C<G<N<T order   */
#define BFQ_E_TOO_LONG     -5   /* read longer than BFQ_MAX_READ_LEN                       */
#define BFQ_E_FREQ3        -6   /* three frequent symbols: assert of bfq_int.cpp:505        */
#define BFQ_E_NOMEM        -7
#define BFQ_E_IO           -8   /* file read / write failed (the *_fd entry points)          */

#define BFQ_MAX_READ_LEN 65000  /* LCP is held in 16 bits (reference: LONGEST 10000, bfq_int.cpp:30) */

/* Run-time form of the reference's getopt flags (bfq_int.cpp:883-935) and of its
 * compile-time knobs -DM / -DB (src_int_mem/Makefile:13-23). */
typedef struct bfq_params {
    int32_t K;      /* -k  minimum LCP inside clusters            default 16        */
    int32_t m;      /* -m  minimum cluster length                 default 2         */
    int32_t v;      /* -v  replacement quality (ASCII code, M=2)  default '>' (62)  */
    int32_t f;      /* -f  frequent-symbol percentage             default 40        */
    int32_t t;      /* -t  trusted-quality threshold (phred)      default 20        */
    int32_t term;   /* -s  terminator byte in the eBWT            default '#' (35)  */
    int32_t M;      /* 0 max, 1 mean error, 2 constant, 3 average default 2         */
    int32_t B;      /* 1 = Illumina 8-level binning               default 0         */
    int32_t ext;    /* 1 = bfq_ext arithmetic for M=3 (bfq_ext.cpp:496)             */
    int32_t piles;  /* step 1 pile by pile (first-symbol piles as in bfq_ext.cpp:190-348; 13 n bytes of workspace
                       instead of 28.6 n): 1 always, 0 when the one-piece workspace cannot be had, -1 never;
                       2: the capped mode always (see ws_cap_mib)                                                */
    int32_t ws_cap_mib; /* upper bound of the device workspace in MiB, 0 = none ($BFQ_WS_CAP in bytes, suffixes K/M/G, overrides it).
                       What a block needs: 28.6 n bytes in one piece, 13 n pile by pile; below that the capped mode runs it in
                       ~8 n: two-symbol piles one at a time, edits written to the text position of every row, no eBWT-sized
                       array, no LF table, no inversion -- same bytes out, about a third more time.  Steps 2-4
                       on a GIVEN eBWT (bfq_smooth_invert*: 17 n with the LF table) then run on 64-byte rank blocks answered
                       on demand, qualities edited in place and a replacement array: 7.3 n (LCP given) / 7.8 n + the ring
                       queue of the LCP deduction (deduced: the ring takes what the cap leaves, n/16 entries at least), the
                       eBWT and the qualities themselves included in the count                                            */
    int32_t reserved[5];
} bfq_params;

/* Counters printed by bfq_int.cpp:1004-1019. */
typedef struct bfq_stats {
    uint64_t num_clust, num_clust_discarded, num_clust_amb_discarded, num_clust_mod,
             num_clust_alleq, bases_inside, qs_smoothed, modified;
    uint64_t n_rows, n_reads, n_segments, n_big_segments;
} bfq_stats;

typedef struct bfq_ctx bfq_ctx;

void     bfq_default_params(bfq_params *p);
bfq_ctx *bfq_create(int device, const bfq_params *p);          /* NULL on failure: see bfq_create_error() */
const char *bfq_create_error(void);
void     bfq_destroy(bfq_ctx *c);
int      bfq_set_params(bfq_ctx *c, const bfq_params *p);
const char *bfq_last_error(bfq_ctx *c);
void    *bfq_stream(bfq_ctx *c);                                /* the hipStream_t all kernels run on */
int      bfq_device_count(void);

/* ---- which GPU a one-shot tool uses.  BFQzip_parallel.py:277-285 starts n concurrent `BFQzip.py` children whose
 * gsufsort / bfq_int processes know nothing of each other (BFQzip.py:178-228): the drop-in tools spread over the node's GPUs
 * through per-GPU lease files -- `<dir>/bfqzip_amd.<PCI bus id>.lock`, held by flock() until the process ends; dir =
 * $BFQ_LEASE_DIR, else /dev/shm, else /tmp.  bfq_pick_device() takes the first free GPU (polling when all are busy, so tools
 * on one GPU run one after the other instead of stacking their workspaces) and returns its device index for bfq_create(),
 * or a negative BFQ_E_* code.  $BFQ_DEVICE=k pins the tool to GPU k (still under that GPU's lease); $BFQ_LEASE=0 switches the
 * lease off (device $BFQ_DEVICE or 0); $BFQ_FAKE_DEVICES=n pretends n GPUs (slot k -> device k mod the real count; lease tests
 * on one GPU).  info (may be NULL) receives "device <k> lease <path> waited <s> s".  Long-lived hosts (parallel.py, bench.py)
 * place their ranks themselves and never call it.
 * bfq_device_lease() is the host-only part (no GPU needed): n_slots lock files named by slot_ids[k] (NULL: "slot<k>"),
 * only_slot >= 0 restricts the choice to that slot; returns the slot taken.  bfq_device_release() gives a slot back early. */
int bfq_pick_device(char *info, int info_cap);
int bfq_device_lease(int n_slots, const char *const *slot_ids, int only_slot, char *path_out, int path_cap, double *waited_s);
int bfq_device_release(int slot);

/* ---- phase timeline of a one-shot tool (process + HIP start, lease wait, allocation, file read + H2D, GPU, D2H + file
 * write): bfq_phase(name) closes the running phase and opens `name` (NULL: closes only); bfq_phase_report(tool) prints one
 * line `[bfq phases] {"tool": .., "exec_to_main": s, "<phase>": s, .., "total": s}` on stderr.  Off unless
 * bfq_phase_enable(1) was called (the tools' -V) or $BFQ_TRACE is set; bench.py's dropin_wall_s split is parsed from it. */
void bfq_phase_enable(int on);
void bfq_phase(const char *name);
void bfq_phase_report(const char *tool);

/* ---- step 1: replaces `gsufsort <fq> --bwt --qs -o OUT` (BFQzip.py:184) and
 *      `eGap <fq> --em --mem M --qs -o OUT --lcp --lbytes 1` (BFQzip_ext.py:177).
 * h_bases/h_quals: the reads back to back (lines 2 and 4 of each record),
 * h_read_off[N+1]: offsets.  Outputs (host, n = h_read_off[N]+N entries each):
 * h_bwt, h_bwtqs; h_lcp16 (exact, may be NULL).  term_out: byte written for the
 * terminator ('#' for gsufsort, 0 for eGap). */
int bfq_build_ebwt(bfq_ctx *c, const uint8_t *h_bases, const uint8_t *h_quals,
                   const uint64_t *h_read_off, uint64_t N, int term_out,
                   uint8_t *h_bwt, uint8_t *h_bwtqs, uint16_t *h_lcp16);

/* ---- steps 2-4: replaces `bfq_int -e OUT.bwt -q OUT.bwt.qs -o OUT.fq ...`
 *      (BFQzip.py:215-222; main() bfq_int.cpp:875-1062) when h_lcp is NULL, and
 *      `bfq_ext -e .. -q .. -a OUT.1.lcp ...` (BFQzip_ext.py:208-214) when h_lcp
 *      is given (lcp_bytes = 1, 2 or 4 bytes per entry, little endian).
 * Outputs: h_out_bases/h_out_quals (n - N bytes each), h_out_read_off[N+1].
 * Call bfq_count_reads() first to size them. */
int bfq_count_reads(const uint8_t *h_bwt, uint64_t n, int term, uint64_t *N);
int bfq_smooth_invert(bfq_ctx *c, const uint8_t *h_bwt, const uint8_t *h_bwtqs,
                      const void *h_lcp, int lcp_bytes, uint64_t n,
                      uint8_t *h_out_bases, uint8_t *h_out_quals, uint64_t *h_out_read_off,
                      bfq_stats *st);

/* ---- fused path (no intermediate files): reads in -> smoothed reads out. */
int bfq_run_reads(bfq_ctx *c, const uint8_t *h_bases, const uint8_t *h_quals,
                  const uint64_t *h_read_off, uint64_t N,
                  uint8_t *h_out_bases, uint8_t *h_out_quals, bfq_stats *st);

/* Same with everything resident in HBM (what bench.py times).  d_out_* may
 * alias nothing else; total = number of bases = d_read_off[N] (given by the
 * caller so that no synchronising read-back is needed). */
int bfq_run_reads_device(bfq_ctx *c, const uint8_t *d_bases, const uint8_t *d_quals,
                         const uint64_t *d_read_off, uint64_t N, uint64_t total,
                         uint8_t *d_out_bases, uint8_t *d_out_quals, bfq_stats *st);

/* ---- FASTQ text in / out, parsed and formatted on the GPU (host buffers).
 * Records are 4 lines; CR before LF is dropped from lines 2 and 4; a record whose quality line is
 * not as long as its sequence is an error (checkFASTQ.py:18-32).
 *   bfq_fastq_build_ebwt   : gsufsort / eGap on the file's bytes; outputs hold cap_rows entries
 *                            (len/2 + 1 is always enough); *n_rows / *n_reads receive the sizes.
 *   bfq_fastq_run          : the whole path, text to text; keep_headers != 0 passes every record's
 *                            header line through (BFQzip.py --headers), else "@" (bfq_int.cpp:758,805).
 *   bfq_smooth_invert_fastq: bfq_int / bfq_ext writing the FASTQ text itself; h_headers = the -H file
 *                            (one line per read) or NULL.
 *   bfq_fastq_run_streams  : the whole path with the result as the separate streams that BFQzip.py's
 *                            --m2/--m3 modes compress (BFQzip.py:19-21,192-251): h_dna = `sed -n 2~4p OUT.fq`,
 *                            h_qs = `sed -n 4~4p OUT.fq` (total bases + reads bytes each), h_hdr = `sed -n 1~4p
 *                            in.fastq` (may be NULL).  A capacity of `len` is always enough for each.
 * Output size: bfq_fastq_out_bound(total bases, reads, header bytes without newlines or 0). */
uint64_t bfq_fastq_out_bound(uint64_t total_bases, uint64_t n_reads, uint64_t header_bytes);
int bfq_fastq_build_ebwt(bfq_ctx *c, const uint8_t *h_fastq, uint64_t len, int term_out,
                         uint8_t *h_bwt, uint8_t *h_bwtqs, uint16_t *h_lcp16, uint64_t cap_rows,
                         uint64_t *n_rows, uint64_t *n_reads);
int bfq_fastq_run(bfq_ctx *c, const uint8_t *h_fastq, uint64_t len, int keep_headers,
                  uint8_t *h_out, uint64_t cap, uint64_t *out_len, bfq_stats *st);
int bfq_fastq_run_streams(bfq_ctx *c, const uint8_t *h_fastq, uint64_t len,
                          uint8_t *h_dna, uint8_t *h_qs, uint64_t cap_stream, uint64_t *stream_len,
                          uint8_t *h_hdr, uint64_t cap_hdr, uint64_t *hdr_len, bfq_stats *st);
int bfq_smooth_invert_fastq(bfq_ctx *c, const uint8_t *h_bwt, const uint8_t *h_bwtqs,
                            const void *h_lcp, int lcp_bytes, uint64_t n,
                            const uint8_t *h_headers, uint64_t headers_len,
                            uint8_t *h_out, uint64_t cap, uint64_t *out_len, bfq_stats *st);

/* ---- the two tools on open files (what the drop-in executables call): same operations as bfq_fastq_build_ebwt
 * and bfq_smooth_invert_fastq, the bytes moved between the files and the GPU by the library's pinned staging
 * pipeline (pread / pwrite by several threads: no mapping, no intermediate copy of a whole file in host memory).
 * Outputs are written from offset 0 of descriptors the caller opened for writing (and truncated); a descriptor
 * < 0 = not wanted / not given.  lcp_bytes: 1, 2 or 4 (eGap --lbytes; 1 saturates at 255). */
int bfq_fastq_build_ebwt_fd(bfq_ctx *c, int fastq_fd, uint64_t len, int term_out, int bwt_fd, int bwtqs_fd,
                            int lcp_fd, int lcp_bytes, uint64_t *n_rows, uint64_t *n_reads);
int bfq_smooth_invert_fastq_fd(bfq_ctx *c, int bwt_fd, int bwtqs_fd, int lcp_fd, int lcp_bytes, uint64_t n,
                               int headers_fd, uint64_t headers_len, int out_fd, uint64_t *out_len, bfq_stats *st);
/* What a tool can start before the GPU is initialised: bfq_output_prefault() sizes an output descriptor to map_len bytes,
 * maps it and lets helper threads fault in its first prefault_len bytes in the background (the page-cache pages of a 9 GB
 * output are allocated and zeroed by the kernel at ~6 GB/s; done beside the upload and the GPU work, the final copy runs at
 * memcpy speed).  The *_fd entry point that is later handed the same descriptor picks the mapping up and cuts the file to
 * its real length.  Bounds: eBWT / QS files <= len / 2 + 64 bytes for a FASTQ of len bytes, bfq_fastq_rows_estimate() =
 * the likely row count (from the first records of the file); the FASTQ text bfq_int writes is >= 2 n and <= 6 n + the
 * header file + 4096 bytes for an eBWT of n rows.  Optional: without it the entry points do the same from their first line. */
int      bfq_output_prefault(int fd, uint64_t map_len, uint64_t prefault_len);
uint64_t bfq_fastq_rows_estimate(int fastq_fd, uint64_t len);

/* ---- one block of BFQzip_parallel.py as one call (BFQzip_parallel.py:277-285 runs `BFQzip.py <block> --rebuild -0
 * [--headers]` per block; :325-360 appends mate block k of file 2 to block k of file 1; :153-172 cuts the
 * block's output back into OUT_1 / OUT_2 by line count).
 * The block's text is given as 1..BFQ_MAX_PARTS byte ranges (mmap'ed file ranges or pinned buffers; a part that
 * lacks its final newline gets one) processed as ONE collection, parts in order.  Any of the outputs may be
 * asked for in the same pass: the FASTQ text (out_fastq), the --m2/--m3 streams (out_dna, out_qs, out_hdr).
 * part_*[p] = where part p's share of each output starts (entry nparts = the end), part_reads[p] = index of its
 * first read.  Pinned host buffers (bfq_host_alloc) are transferred by direct DMA, pageable ones through the
 * library's pinned staging pipeline. */
#define BFQ_MAX_PARTS 4
typedef struct bfq_text_part { const uint8_t *data; uint64_t len; } bfq_text_part;
typedef struct bfq_fastq_job {
    const bfq_text_part *parts; int32_t nparts;
    int32_t keep_headers;                     /* FASTQ text: header lines verbatim (BFQzip.py --headers) or "@"  */
    uint8_t *out_fastq; uint64_t cap_fastq;   /* NULL: not wanted; bfq_fastq_out_bound() / input length + 16     */
    uint8_t *out_dna, *out_qs; uint64_t cap_stream;   /* total bases + reads bytes each                           */
    uint8_t *out_hdr; uint64_t cap_hdr;       /* `sed -n 1~4p` of the input                                      */
    /* results */
    uint64_t fastq_len, stream_len, hdr_len, n_reads, total_bases;
    uint64_t part_reads[BFQ_MAX_PARTS + 1], part_fastq_off[BFQ_MAX_PARTS + 1],
             part_stream_off[BFQ_MAX_PARTS + 1], part_hdr_off[BFQ_MAX_PARTS + 1];
    /* steps 1-5 in one call: the streams leave as BFQRANS2 containers (bfq_stream_compress, below) instead of raw bytes --
     * what `BFQzip.py --m2/--m3` without -0 produces through 7z / bsc (BFQzip.py:253-275).  The raw streams never cross
     * the bus.  stream_len / hdr_len stay the RAW lengths; *_bytes = what was written to out_dna / out_qs / out_hdr.
     * Capacities: bfq_stream_bound(raw length) always suffices (a tiny stream's container is larger than the stream; the raw
     * length is enough from a few MB on); out_dna of modes 2 / 3 holds two containers: twice that + 40. */
    int32_t  compress_streams;                /* 1: as described; 2: eBWT-domain containers (bfq_stream_ebwt_decode, below);
                                                 3: the same with the qualities in read order (smallest output) */
    int32_t  name_codec;                      /* 0: out_hdr as described; 1 (with compress_streams 1, 2 or 3): out_hdr is what
                                                 bfq_names_compress(flags 0) gives for the header stream (BFQNAME1 where shorter) */
    uint64_t dna_bytes, qs_bytes, hdr_bytes;
    int32_t  qual_codec;                      /* 0: out_qs as described; 1 (with compress_streams 1 or 3, whose qualities are lines in
                                                 read order): out_qs is what bfq_quals_compress(flags 0) gives for the quality stream
                                                 (BFQQUAL1 where shorter); with compress_streams 2 (qualities in row order): BFQ_E_ARG.
                                                 The two fields stand behind the older ones, whose offsets do not change. */
    int32_t  reserved1;
} bfq_fastq_job;
int bfq_fastq_run_job(bfq_ctx *c, bfq_fastq_job *job, bfq_stats *st);
/* ... and the run's base edits in the same call (BFQEDIT1, below).  bfq_fastq_job keeps its size and every offset: what the
 * edits need travels in a structure of its own beside it.  edits NULL or out_edits NULL: exactly bfq_fastq_run_job, nothing
 * of it runs.  Else the member of this job's collection -- the input's byte at every base the run changed -- goes to
 * out_edits and edits_bytes receives its length; with compress_streams 2 or 3 (no read-order bases): BFQ_E_ARG.  cap_edits
 * too small: BFQ_E_ARG, the message holds the size that suffices and edits_bytes keeps it; out_edits and the job's FASTQ text
 * are untouched then. */
typedef struct bfq_job_edits { uint8_t *out_edits; uint64_t cap_edits, edits_bytes; } bfq_job_edits;
int bfq_fastq_run_job_edits(bfq_ctx *c, bfq_fastq_job *job, bfq_job_edits *edits, bfq_stats *st);

/* ---- one collection over several GPUs with the UNSHARDED result (opt-in; not in the reference, whose parallel driver
 * gives up the clusters that span blocks, README.md:107).  The per-GPU pieces; bfqzip_amd/parallel.py --global holds the
 * device buffers (torch tensors) and runs the collectives.  d_ = device pointers.
 *   bfq_glob_begin      : upload and parse this rank's block; its text stays resident in the context
 *   bfq_glob_local_text : the block as terminated text: symbol codes (# 0, A 1, C 2, G 3, N 4, T 5) and qualities,
 *                         total_bases + n_reads bytes each -> exchanged so that every rank holds the whole text (n bytes)
 *   bfq_glob_pile_counts: counts36[6 s + s2] = suffixes that start with symbols s, s2 (row 0: the terminator suffixes)
 *   bfq_glob_init_out   : line-stream copy of the whole text (letters / qualities, '\n' at the terminators)
 *   bfq_glob_run_pile   : sort + refine the pile (s, s2) of the global eBWT, cluster analysis, edits written to d_sym / d_qual
 *                         at the text position each row stands for; statistics of this pile in *st
 *   bfq_glob_finish     : this block's line streams (after the exchange) -> FASTQ text / streams as in bfq_fastq_run_job
 *                         (job->parts ignored; qualities are binned here when B = 1) */
int bfq_glob_begin(bfq_ctx *c, const bfq_text_part *parts, int nparts, uint64_t *n_reads, uint64_t *total_bases);
int bfq_glob_local_text(bfq_ctx *c, uint8_t *d_T8, uint8_t *d_Q8);
int bfq_glob_pile_counts(bfq_ctx *c, const uint8_t *d_T8, uint64_t n, uint64_t *counts36);
int bfq_glob_init_out(bfq_ctx *c, const uint8_t *d_T8, const uint8_t *d_Q8, uint64_t n, uint8_t *d_sym, uint8_t *d_qual);
int bfq_glob_run_pile(bfq_ctx *c, const uint8_t *d_T8, const uint8_t *d_Q8, uint64_t n, int s, int s2,
                      uint8_t *d_sym, uint8_t *d_qual, bfq_stats *st);
int bfq_glob_finish(bfq_ctx *c, uint8_t *d_dna, uint8_t *d_qs, bfq_fastq_job *job);

/* Pinned (page-locked) host memory for the buffers above. */
void *bfq_host_alloc(uint64_t bytes);
void  bfq_host_free(void *p);

/* Host-side line index of a text (what BFQzip_parallel.py:295-319 does with Python line loops): counts[i] =
 * number of '\n' in bytes [i*chunk, (i+1)*chunk), computed by `threads` threads (0: default);
 * bfq_text_nth_newline = offset of the k-th (0-based) '\n' of the range or -1.  Pure host functions (no GPU). */
int     bfq_text_count_lines(const uint8_t *h_text, uint64_t len, uint64_t chunk, uint64_t *counts, int threads);
/* a host buffer into a file at an offset by several threads (fallocate + shared mapping; pwrite when the file cannot be
 * mapped): how the multi-GPU driver puts every block's outputs at their final place of the shared output files
 * (BFQzip_parallel.py:137-179 merges with `cat`).  fd must be open for reading and writing; the file grows as needed and is
 * never shrunk, so several processes may fill different ranges of one file.  threads 0: by the CPU budget.  Host only. */
int     bfq_file_put(int fd, uint64_t offset, const void *src, uint64_t len, int threads);
/* ... or the range itself as memory to fill (allocated, mapped, populated by a few threads): an output buffer for
 * bfq_fastq_run_job / bfq_glob_finish that IS the file -- no copy afterwards.  NULL when the file cannot be mapped;
 * bfq_file_unmap() takes the same offset and length. */
void   *bfq_file_map(int fd, uint64_t offset, uint64_t len, int threads);
int     bfq_file_unmap(void *p, uint64_t offset, uint64_t len);
int64_t bfq_text_nth_newline(const uint8_t *h_text, uint64_t len, uint64_t k);

/* Device-resident eBWT of the last bfq_run_reads*() / bfq_build_ebwt() call
 * (valid until the next call on the context): copies to host. Any may be NULL.
 * h_bwtqs receives the permuted qualities as built (before smoothing). */
int bfq_fetch_ebwt(bfq_ctx *c, uint8_t *h_bwt, uint8_t *h_bwtqs, uint16_t *h_lcp16);

/* ---- synthetic reads (seeded, counter based; DESIGN.md "synthetic workload").
 * Fixed length L when Lmin == Lmax.  Host and device versions produce identical
 * bytes.  read_off[N+1] is written too. */
typedef struct bfq_synth {
    uint64_t seed;
    uint64_t N;          /* reads                                   */
    uint32_t Lmin, Lmax; /* read length range (inclusive)           */
    uint32_t coverage;   /* genome length = N*Lavg/coverage         */
    uint32_t err_ppm;    /* substitution errors, per million bases  */
    uint32_t n_ppm;      /* 'N' calls, per million bases            */
    uint32_t snp_every;  /* haplotype SNP period (~1000)            */
    uint32_t dsnp_every; /* adjacent double-SNP period (~10000)     */
    uint32_t both_strands;
    uint64_t first;      /* these N reads are reads [first, first+N) ...                          */
    uint64_t collection; /* ... of a collection of this many reads (0: N; sets the genome length): */
    uint32_t reserved[2];/*     a block of BFQzip_parallel's split can be generated on its own     */
} bfq_synth;
void bfq_synth_default(bfq_synth *s, uint64_t N, uint32_t L);
uint64_t bfq_synth_total(const bfq_synth *s);                    /* total bases = read_off[N] */
int bfq_synth_host(const bfq_synth *s, uint8_t *h_bases, uint8_t *h_quals, uint64_t *h_read_off);
int bfq_synth_device(bfq_ctx *c, const bfq_synth *s, uint8_t *d_bases, uint8_t *d_quals,
                     uint64_t *d_read_off);
/* The same reads as the text of a FASTQ file (header lines "@SYN.<read number>", "+" lines bare), generated and
 * formatted on the device, copied to h_out (cap >= N * (2 * Lmax + 30) is always enough). */
int bfq_synth_fastq(bfq_ctx *c, const bfq_synth *s, uint8_t *h_out, uint64_t cap, uint64_t *out_len);

/* ---- stream codec: entropy coding of OUT.fq.dna / OUT.fq.qs / OUT.h on the GPU.
 * Replaces step 5 of the reference, which hands every stream to an external tool: `7z a -mm=PPMd <f>.7z <f>`
 * (step5, BFQzip.py:253-263) or `external/libbsc/bsc e <f> <f>.bsc -T` (step5b, BFQzip.py:265-275).  The front-end
 * dropin/external/libbsc/bsc takes that command line (`bsc e IN OUT [options]`, `bsc d IN OUT`).
 * The containers are this project's own -- neither 7z nor libbsc are part of the reference tree -- and are stated in
 * oracle/bfq_codec_ref.c: "BFQRANS2" (any bytes: static order-k model + range-ANS, segments of 8192 symbols), "BFQLINE1"
 * (read names: a line-delta transform in front of it; "BFQNAME1", below, is the opt-in tokenised form) and "BFQDNAC1" (read-order DNA, lines of A C G T N: a hashed
 * order-K context model that adapts block by block, rebuilt by the decoder from what it has decoded; a third of the static
 * container's size at 30x coverage, a quarter of its speed; $BFQ_DNA_STATIC=1 keeps the static one).
 * Any bytes compress; host buffers in and out.  bfq_stream_decompress takes containers of any kind back to back. */
uint64_t bfq_stream_bound(uint64_t len);                          /* capacity that always suffices for `len` raw bytes */
int64_t  bfq_stream_raw_len(const uint8_t *h_in, uint64_t len);   /* raw length of a container, -1 if it is not one  */
int bfq_stream_compress(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_stream_decompress(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
/* ---- read names as tokens: the opt-in container "BFQNAME1" (k_names.hip; tests/names_model.py states it in Python).  On real
 * names the counters change in every line, so the shared-prefix transform of BFQLINE1 leaves most of a line as literals; here
 * a line is cut into tokens and every token is coded against the token at the same place of the line before.
 * All fields little endian.  The stream is lines, each ended by '\n'; a line is its bytes without the '\n'.
 *   tokens   : maximal runs of ASCII digits / of other bytes.  A digit token is NUMERIC when it has at most 18 digits and
 *              either one digit or a first digit other than '0'; its value is its decimal value (< 10^18).  Every other token
 *              (non-digits, a leading zero, 19 digits or more) is text.
 *   groups   : R = 256 consecutive lines (the last may be shorter).  A line is coded against the line before it in the
 *              input, the first line of a group against the empty line (no tokens).  Groups decode independently.
 *   streams  : `ops` (operations), `num` (DELTA payloads), `text` (TEXT payloads).  For token t of a line, P = token t of the
 *              line before (or absent), v = the token's value, u = P's value when P exists and is numeric, else 0, d = v - u:
 *                SAME   P exists with the same bytes.  Consecutive SAME tokens form a run, written when another operation
 *                       or the end of the line follows, in pieces of at most 240, the 240s first: a piece of k is byte 15 + k
 *                INC    numeric, d = 1: byte 2
 *                DELTA  numeric otherwise: byte 3; `num` gets the LEB128 of z = 2 d (d >= 0) or -2 d - 1 (d < 0)
 *                TEXT   anything else: byte 4; `text` gets the LEB128 of the token's length, then its bytes
 *              in this order of precedence; after a line's last token (and its pending run) byte 0 (END).  Bytes 1 and 5..15
 *              are no operations.  LEB128: seven bits per byte, low groups first, bit 7 set on all but the last byte.
 *   index    : per group four u32: its bytes of ops, of num, of text, and its raw bytes (newlines included)
 *   container: "BFQNAME1" | u64 raw_len | u32 R = 256 | u32 0 | u64 lines | u64 bytes of member 0..3 | the members back to
 *              back: index, ops, num, text, each exactly what bfq_stream_compress writes for those bytes (an empty member
 *              included); the members carry the codec's checksums.
 * Eligible: a stream of at least one byte that ends with '\n' and has no line longer than 65 535 bytes.
 * The decoder re-tokenises the line it has just written to find P and writes numbers as shortest decimals.  It refuses with
 * BFQ_E_ARG "damaged BFQNAME1 stream": R != 256 or the reserved field set; no lines or more lines than raw bytes; member lengths
 * that do not add up to the container; an index of other than 16 ceil(lines / 256) bytes; members whose raw lengths are not
 * the sums of the index columns; raw shares that do not add up to raw_len (or members larger than any encoder output: ops and
 * text above 2 raw_len, num above 5 raw_len); and in a group: a byte that is no operation, a SAME run past the tokens of the
 * line before, a DELTA result outside 0 .. 10^18 - 1, a LEB128 of more than nine bytes, a TEXT length of 0 or past the group's
 * text share, a line beyond 65 535 bytes, a share of ops / num / text not consumed exactly, a raw share not filled exactly, a
 * line count other than min(256, lines left).  Every read and write stays inside the group's stated shares.
 * bfq_stream_decompress, bfq_stream_raw_len and bfq_fastq_restore* take BFQNAME1 members wherever they take BFQLINE1 ones.
 *   bfq_names_compress       : flags 0: the BFQNAME1 container when the stream is eligible and the container is strictly
 *                              shorter than what bfq_stream_compress writes for the same bytes, else exactly those bytes;
 *                              bfq_stream_bound(len) therefore suffices.  flags bit 0 ("always"): BFQNAME1 whenever the stream
 *                              is eligible (tests, diagnostics).  Other bits: BFQ_E_ARG.
 *   bfq_names_compress_device: both buffers in device memory outside the context's workspace, which the call sizes itself */
int bfq_names_compress(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint32_t flags, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_names_compress_device(bfq_ctx *c, const uint8_t *d_in, uint64_t len, uint32_t flags, uint8_t *d_out, uint64_t cap, uint64_t *out_len);
/* ---- quality lines by their place in the read: the opt-in container "BFQQUAL1" (k_quals.hip; tests/quals_model.py states it
 * in Python).  BFQRANS2 sees the k bytes in front of a value inside an arbitrary segment; here a value is coded against the
 * value before it, a coarse view of the two before that, its place in the read and how noisy the read has been so far.
 * All fields little endian.  The stream is lines, each ended by '\n'; lens[i] = length of line i, vals = the lines without
 * their newlines, nvals = len(vals), maxlen = max(lens).
 *   eligible : the stream ends with '\n', nvals >= 1, no line longer than 65 535, vals has at most 64 distinct byte values
 *              (and nvals < 2^38: the model's counters are 32 bits wide).  Otherwise the general container is written.
 *   alphabet : the distinct values of vals, ascending, A of them; a value's rank is its index there.
 *   segments : S = 1024; segment g = the reads whose first value has an index in [g S, (g + 1) S) of vals (the rule of
 *              BFQDNAC1; a segment may be empty, a read longer than S lies in one segment); nseg = ceil(nvals / S).
 *   context  : for value j of a read with ranks s[0..l), a missing predecessor counting as 0: q1 = s[j-1], q2 = s[j-2],
 *              q3 = s[j-3]; m8 = max(q2, q3) 8 / A; e = (q2 == q3); p16 = min(15, j / W), W = max(1, ceil(maxlen / 16));
 *              delta = sum over t = 1..j-1 of |s[t] - s[t-1]|; d4 = (delta >= 8) + (delta >= 32) + (delta >= 128).
 *   rungs    : rung r = 0..3 has (M, P, D, E) = (1,1,1,1), (4,4,2,1), (8,8,4,1), (8,16,4,2); m = m8 >> (3 - log2 M),
 *              p = p16 >> (4 - log2 P), d = d4 >> (2 - log2 D), e counts only when E = 2;
 *              ctx = (((p D + d) E + e) M + m) A + q1, rows = P D E M A.  The rungs are nested.
 *   model    : static, counted on a sample: the segments with g % St == 0, St = clamp(nvals / 2^24, 1, 64).  Counts are taken
 *              at rmax, the largest rung with rows A <= min(2^22, max(4096, (nvals / St) / 16)) (rung 0 always qualifies);
 *              the container is made with the rung <= rmax whose estimated size is smallest (choose_order()'s estimator in
 *              oracle/bfq_codec_ref.c: payload from the normalised rows times St, + 16 A bits per used row + 1 bit per row;
 *              the lowest rung among equals).  Rows are normalised to 2^12 as normalise() there: every symbol has a
 *              non-zero share in every row.  The order-0 row `dflt` (all counts of the chosen rung) serves rows without counts.
 *   rANS     : BFQRANS2's (state in [2^23, 2^31), byte-wise renormalisation), one stream per non-empty segment: the values
 *              of the segment's reads in order, coded last to first.
 *   container: "BFQQUAL1" | u64 raw_len | u64 nreads | u64 nvals | u32 S, nseg, A, rung, scale_bits (12), maxlen
 *              | u64 checksum of the raw bytes (the codec's) | u64 Lb | a BFQRANS2 container (Lb bytes) of lens[] as u32
 *              | u8 alphabet[64] | u16 dflt[A] | u8 used[ceil(rows / 8)] | u16 freq[used rows][A] | u32 seg_bytes[nseg] | payload
 * The decoder refuses with BFQ_E_ARG "damaged BFQQUAL1 stream": S != 1024, scale != 12, A outside 1..64, rung > 3, an
 * alphabet that is not ascending or holds '\n', nseg != ceil(nvals / S), a lens member whose raw length is not 4 nreads,
 * sum(lens) != nvals or max(lens) != maxlen, nvals + nreads != raw_len, a row (dflt included) that does not sum to 2^12,
 * seg_bytes that do not add up to the payload, bytes for an empty segment, an initial state below 2^23, a refill past the
 * segment's share or a share not consumed exactly, a checksum mismatch.  Every read and write stays inside the stated shares.
 * bfq_stream_decompress, bfq_stream_raw_len and bfq_fastq_restore* take BFQQUAL1 members wherever they take BFQRANS2 members
 * of a quality input; members of both kinds may be mixed in one file.
 *   bfq_quals_compress       : flags 0: the BFQQUAL1 container when the stream is eligible and the container is strictly
 *                              shorter than what bfq_stream_compress writes for the same bytes, else exactly those bytes;
 *                              bfq_stream_bound(len) therefore suffices.  Bit 0 ("always"): BFQQUAL1 whenever the stream is
 *                              eligible.  Bit 1 ("rung forced"): the rung is bits 8-9 and the counts are taken there (the
 *                              sample budget is ignored, the 2^22 cap always holds for A <= 64); tests and diagnostics.
 *                              Any other bit (bits 8-9 without bit 1 included): BFQ_E_ARG.
 *   bfq_quals_compress_device: both buffers in device memory outside the context's workspace, which the call sizes itself */
int bfq_quals_compress(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint32_t flags, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_quals_compress_device(bfq_ctx *c, const uint8_t *d_in, uint64_t len, uint32_t flags, uint8_t *d_out, uint64_t cap, uint64_t *out_len);
/* eBWT-domain containers (bfq_fastq_job.compress_streams = 2; out_fastq must be NULL): out_dna receives "BFQEBWT1" |
 * u64 rows | u64 reads | u32 terminator byte | u32 flags | u64 bytes of the next container | the container of the eBWT's
 * symbols AFTER noise reduction | the container of the replaced rows' original symbols (0 elsewhere), out_qs the
 * container of the rows' qualities after smoothing (row order, n = bases + reads bytes each).  In row order the symbols of a
 * deep collection are runs -- half the size of the read-order stream -- and the compressing side skips the inversion.
 * compress_streams = 3 (flags bit 0) keeps the qualities in READ order (OUT.fq.qs as in mode 1: they code better along the
 * read) at the price of one walk on the compressing side.
 * bfq_stream_ebwt_decode inverts them back to the line streams OUT.fq.dna / OUT.fq.qs (cap >= rows bytes each). */
int bfq_stream_ebwt_decode(bfq_ctx *c, const uint8_t *h_bwtz, uint64_t len_b, const uint8_t *h_qsz, uint64_t len_q,
                           uint8_t *h_dna, uint8_t *h_qs, uint64_t cap, uint64_t *stream_len, uint64_t *n_reads);
/* ---- the way back: the compressed streams of one collection -> its FASTQ text, in one call.  The reference leaves this to
 * `7z x` / `bsc d` on every stream and `paste`; here the containers are decoded on the device, the decoded streams stay
 * there, and only the finished text comes down.  For read i: header line i of the header stream verbatim (h_hdr NULL /
 * hdr_fd < 0: "@"), '\n', DNA line i, "\n+\n", quality line i, '\n' -- byte for byte what bfq_fastq_run_job writes to
 * out_fastq with the same keep_headers (bfq_int.cpp:797-810).  Accepted inputs are what the project's own writers produce:
 *   read-order containers (compress_streams = 1, `bsc e`, parallel.py --compress): dna and qs one or more BFQDNAC1 / BFQRANS2
 *     (qs also BFQQUAL1) members back to back each, hdr one or more BFQLINE1 / BFQRANS2 / BFQNAME1 members; the member boundaries of the three inputs
 *     need not coincide;
 *   eBWT-domain containers (compress_streams = 2 / 3): dna ONE BFQEBWT1 member, qs the one-member container of the rows'
 *     (mode 2) or the reads' (mode 3) qualities.  More than one BFQEBWT1 member is refused with BFQ_E_ARG: no writer of the
 *     project produces that (a sharded run writes read-order containers).
 * An input that is not a container is BFQ_E_ARG; raw streams are not guessed at.  Streams that do not describe the same
 * reads (line counts differ, DNA and quality line of a read differ in length, header count != read count, a line beyond
 * BFQ_MAX_READ_LEN) are BFQ_E_ARG with a message that names the first offending read (0-based); nothing is written to
 * h_out / out_fd then (the file is left empty).  Device memory: the decoded streams + the text + the larger of the codec's
 * workspace for the largest member and 64 bytes per read of index, reserved once from the container headers; above
 * ws_cap_mib: BFQ_E_NOMEM with the size in the message.  A static (BFQRANS2) DNA container states no read count: the index
 * is then sized for one read per byte.
 *   bfq_fastq_restore_bound: upper bound of the text; host only, reads the container headers; -1: not containers
 *   bfq_fastq_restore      : host buffers (pinned: direct DMA); cap >= the text, else BFQ_E_ARG and *out_len = 0
 *   bfq_fastq_restore_fd   : open files; the text goes out through the background writers into out_fd (a mapping
 *                            registered by bfq_output_prefault is picked up), which is cut to its real length */
int64_t bfq_fastq_restore_bound(const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                const uint8_t *h_hdr, uint64_t hdr_len);
int bfq_fastq_restore(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                      const uint8_t *h_hdr, uint64_t hdr_len, uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_restore_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len,
                         int hdr_fd, uint64_t hdr_len, int out_fd, uint64_t *out_len, uint64_t *n_reads);
/* ---- the way back, block by block.  The members of one block of a sharded run (parallel.py --compress appends one container
 * per block to every .bsc) decode independently of every other block: an archive is a sequence of GROUPS, and the grouped
 * calls restore one group after another in an arena sized by the largest group instead of by the whole archive.
 *   bfq_fastq_restore_groups: the plan.  Host only (no context, no GPU), reads the container headers and decodes nothing.
 *     The DNA and the quality input are walked with one cursor each; a group takes one member of each and then further
 *     members of whichever side has decoded to fewer bytes until both have decoded to the same number, and ends there (the
 *     finest cut; a group of raw length 0 is a block of no reads).  A BFQEBWT1 member is one DNA member of `rows` raw bytes
 *     with ONE quality member of the same raw length beside it.  A header input must have exactly one member per group.
 *     Returns the number of groups G and fills min(G, cap) entries; a negative BFQ_E_* with the reason in `why` (why_cap
 *     bytes, may be NULL) when the totals of the two inputs never meet ("not of the same collection"), bytes are no member,
 *     an input is empty or the header members do not count G.
 *   bfq_stream_members: number of members in [h_in, h_in + len) (a BFQEBWT1 member counts once); -1: bytes that are no member.
 *   bfq_fastq_restore_grouped / _fd: groups [first, first + count) of the plan (count = ~0: to the end), their texts
 *     concatenated from offset 0 of the output; for every archive both calls accept, (0, ~0) writes byte for byte what
 *     bfq_fastq_restore writes, and the groups restored one at a time concatenate to the same bytes.  Several BFQEBWT1
 *     members (the outputs of several compress_streams = 2 / 3 jobs back to back) are restored here, one per group.
 *     Device memory, reserved once before the first group from the LARGEST group of the range: its decoded streams + two
 *     text buffers of its text bound + the larger of (its compressed members + the codec's workspace for its largest
 *     member) and its index + 64 MiB; above ws_cap_mib: BFQ_E_NOMEM naming that group and the cap.  The text of group g
 *     leaves the device (background writers of the file form; direct DMA into a pinned h_out) while group g + 1 is decoded;
 *     the two text buffers alternate.  Every group but the archive's last must end each of its non-empty decoded streams with
 *     '\n' (a line index would otherwise give the cut line a newline of its own and split a read): else BFQ_E_ARG naming
 *     the group and the stream.  A read the validator refuses is named by its index in the archive (the reads of the earlier
 *     groups plus its index in the group -- when first > 0, where every earlier DNA member states its reads) and the group.
 *     Whatever the plan can refuse (also: first >= G, first + count > G) is refused before a byte is written.  On any
 *     failure *out_len = 0; the file form leaves out_fd empty; a MEMORY destination may have been written up to the failing
 *     group.  No BFQPERM1 permutation here: records in the original order draw on all groups at once. */
typedef struct bfq_restore_group {
    uint64_t dna_off, dna_len;     /* this group's members inside the DNA input (bytes)        */
    uint64_t qs_off,  qs_len;
    uint64_t hdr_off, hdr_len;     /* 0, 0 without a header input                               */
    uint64_t raw_stream;           /* decoded bytes of its DNA members = of its quality members */
    uint64_t raw_hdr;
    uint64_t reads;                /* where every DNA member states it (BFQDNAC1, BFQEBWT1), else ~0 */
    uint64_t text_bound;           /* as bfq_fastq_restore_bound, for this group                */
} bfq_restore_group;
int64_t bfq_fastq_restore_groups(const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                 const uint8_t *h_hdr, uint64_t hdr_len,
                                 bfq_restore_group *groups, uint64_t cap, char *why, int why_cap);
int64_t bfq_stream_members(const uint8_t *h_in, uint64_t len);
int bfq_fastq_restore_grouped(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                              const uint8_t *h_hdr, uint64_t hdr_len, uint64_t first, uint64_t count,
                              uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_restore_grouped_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                 uint64_t first, uint64_t count, int out_fd, uint64_t *out_len, uint64_t *n_reads);
/* ---- reads of a FASTQ in another order (the pre-pass of `BFQzip_parallel.py --reorder {1,2}`, :35,59-75,389-437, which shells
 * out to randomFASTQ.py / SPRING's reorder-only tool): FASTQ text in -> the same records, verbatim, in a new order out.  A
 * sharded run cuts the input into blocks of consecutive reads; reads of one locus brought together end up in one block and
 * keep their clusters.  The order is ascending key, ties in input order:
 *   mode 2 "locus" : over every window of k consecutive bytes of the sequence line (CR before LF dropped) that are all in
 *                    ACGT: x = the window packed two bits per base (A 0, C 1, G 2, T 3, first base most significant), h =
 *                    MurmurHash3's 64-bit finaliser of x; key = (min h) >> 24, 40 bits.  No valid window: 2^40 - 1.
 *                    k: 8..32, 0 = 21.
 *   mode 1 "random": key = fmix64(seed + read index) >> 24.
 * Two parts are mates: record i of part 2 moves with record i of part 1; the pair's key is mate 1's, or mate 2's when mate 1
 * has no valid window; different record counts are BFQ_E_ARG.  A record is its four lines byte for byte (header, '+' line
 * and CRs as they are); a part that lacks its final newline gets one, so out_len[p] = parts[p].len (+ 1 then).
 * h_perm (uint64[number of reads] or NULL): perm[j] = input index of output record j.  Malformed text: the code and message
 * of bfq_fastq_run.  cap[p] < out_len[p]: BFQ_E_ARG, out_len zeroed, nothing written.  Device memory: the input, the
 * output and ~160 bytes of index per read; above ws_cap_mib: BFQ_E_NOMEM with the size in the message (an input larger than
 * device memory is not split).
 *   bfq_reorder_key     : the mode-2 key of one sequence line, host only (the statement the kernel is tested against);
 *                         UINT64_MAX when k is outside 8..32
 *   bfq_fastq_reorder   : host buffers (pinned: direct DMA)
 *   bfq_fastq_reorder_fd: open files (nparts inputs, nparts outputs); the text goes out through the background writers into
 *                         out_fd[p] (a mapping registered by bfq_output_prefault is picked up); on failure they are left empty */
typedef struct bfq_reorder_opts {
    int32_t  mode;       /* 1 random, 2 locus                           */
    int32_t  k;          /* window of mode 2: 8..32, 0 = 21             */
    uint64_t seed;       /* mode 1                                      */
    uint64_t reserved[2];
} bfq_reorder_opts;
uint64_t bfq_reorder_key(const uint8_t *seq, uint64_t len, int k);
int bfq_fastq_reorder(bfq_ctx *c, const bfq_text_part *parts, int nparts, const bfq_reorder_opts *opts, uint8_t *const *h_out,
                      const uint64_t *cap, uint64_t *out_len, uint64_t *h_perm, uint64_t *n_reads);
int bfq_fastq_reorder_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, const bfq_reorder_opts *opts,
                         const int *out_fd, uint64_t *out_len, uint64_t *n_reads);
/* ---- the way back to the input order.  A reordered run loses the order of the original file unless the permutation is
 * kept; these calls keep it, as a file, and undo it on the device.
 * Container BFQPERM1, all fields little endian:
 *   header, 40 bytes: "BFQPERM1" | u64 N (reads) | u32 w (bits per entry) | u32 mode | u32 k | u32 reserved = 0 | u64 seed
 *                     (mode / k / seed: the bfq_reorder_opts it came from, k = 0 written as 21; informational).  w = bit length of N - 1, and 1
 *                     when N <= 2; N < 2^56.
 *   payload         : ceil(N w / 64) u64 words.  Entry j is perm[j], the input index of output record j (h_perm of
 *                     bfq_fastq_reorder); it occupies bits [j w, (j + 1) w) of the bit stream, bit b of the stream being bit
 *                     b % 64 of word b / 64.  The padding bits of the last word are 0.
 *   total length    : exactly 40 + 8 ceil(N w / 64) bytes (~94 MB at 30 M reads, against 240 MB as raw u64).
 * A container is well formed only if the magic, w, the total length and the zero padding are as above, every entry is < N and
 * no value occurs twice.  Its first offending position is the smallest j with perm[j] >= N or perm[j] met at an earlier
 * position.
 * Host only (no GPU; the statement the kernels are tested against):
 *   bfq_perm_bound : the exact container length for n_reads (0 when n_reads >= 2^56)
 *   bfq_perm_reads : N, or -1 when magic / w / length / padding are wrong (the entries are not looked at)
 *   bfq_perm_encode: h_perm[N] -> container; BFQ_E_ARG and nothing written when cap < bfq_perm_bound(N) or h_perm is not a
 *                    permutation of 0..N-1
 *   bfq_perm_decode: container -> h_perm[N], *N, *opts_out (may be NULL); BFQ_E_ARG and nothing written when the container is
 *                    not well formed or cap_entries < N; *first_bad (may be NULL) is then the first offending position, or
 *                    UINT64_MAX when the fault is in the header or the arguments
 * On the device:
 *   bfq_fastq_reorder_keep / _keep_fd: bfq_fastq_reorder / _fd, and the container of what they did: the permutation is packed
 *     on the device and leaves as the packed bytes.  cap_permz < bfq_perm_bound(N): BFQ_E_ARG, nothing written (the texts
 *     neither).  On any failure *permz_len = 0 and h_permz is untouched / perm_fd is left empty, like the text outputs.
 *   bfq_fastq_unreorder / _fd: FASTQ text in the order of a reordered run + its container -> output record perm[j] is input
 *     record j, byte for byte; two parts are mates and the one permutation applies to both; a missing final newline is added.
 *     The container is uploaded, unpacked, validated and inverted on the device (inv[v] = the smallest j with perm[j] = v),
 *     and the reorder's gather reads through the inverse.  Refusals, all BFQ_E_ARG with nothing written (files left empty):
 *     not a BFQPERM1 container; a permutation of X reads for a text of Y records (the message names both); an entry out of
 *     range or a value twice (the message names the first offending position).  Malformed text, cap[p] too small and memory
 *     above ws_cap_mib: as bfq_fastq_reorder.  Device memory: as bfq_fastq_reorder.
 *   bfq_fastq_restore_ordered / _fd: bfq_fastq_restore / _fd with the records un-reordered in the same call: the output is
 *     that of bfq_fastq_restore with output record perm[j] = its record j.  After the streams have been checked (their
 *     messages are those of bfq_fastq_restore and come first) the container is validated and inverted as above, the record
 *     sizes are scanned through the inverse, and the text is written once, record i from read inv[i] of the line streams: no
 *     second pass over the text.  A permutation whose N differs from the streams' read count is BFQ_E_ARG with both numbers
 *     in the message.  Device memory: bfq_fastq_restore's, with 96 instead of 64 bytes of index per read (the container's
 *     payload, the unpacked permutation and its inverse: ~24 bytes per read, and 4 of sizes), reserved in the same single
 *     reservation. */
uint64_t bfq_perm_bound(uint64_t n_reads);
int64_t  bfq_perm_reads(const uint8_t *h_permz, uint64_t len);
int bfq_perm_encode(const uint64_t *h_perm, uint64_t N, const bfq_reorder_opts *opts, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_perm_decode(const uint8_t *h_permz, uint64_t len, uint64_t *h_perm, uint64_t cap_entries, uint64_t *N,
                    bfq_reorder_opts *opts_out, uint64_t *first_bad);
int bfq_fastq_reorder_keep(bfq_ctx *c, const bfq_text_part *parts, int nparts, const bfq_reorder_opts *opts, uint8_t *const *h_out,
                           const uint64_t *cap, uint64_t *out_len, uint8_t *h_permz, uint64_t cap_permz, uint64_t *permz_len,
                           uint64_t *n_reads);
int bfq_fastq_reorder_keep_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, const bfq_reorder_opts *opts,
                              const int *out_fd, int perm_fd, uint64_t *out_len, uint64_t *permz_len, uint64_t *n_reads);
int bfq_fastq_unreorder(bfq_ctx *c, const bfq_text_part *parts, int nparts, const uint8_t *h_permz, uint64_t permz_len,
                        uint8_t *const *h_out, const uint64_t *cap, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_unreorder_fd(bfq_ctx *c, const int *in_fd, const uint64_t *in_len, int nparts, int perm_fd, uint64_t permz_len,
                           const int *out_fd, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_restore_ordered(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                              const uint8_t *h_hdr, uint64_t hdr_len, const uint8_t *h_permz, uint64_t permz_len,
                              uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_restore_ordered_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                 int perm_fd, uint64_t permz_len, int out_fd, uint64_t *out_len, uint64_t *n_reads);
/* ---- what a run did to the data: two FASTQ texts compared on the device, A "before" and B "after" (k_compare.hip;
 * tests/compare_model.py states it in Python).  The reference leaves this question to a bwa + GATK pipeline downstream.
 * Inputs: each text is 1..BFQ_MAX_PARTS parts taken as one text, in order; a part without its final newline gets one, as in
 *   bfq_fastq_run_job; the part boundaries of A and B need not correspond.  Records are four lines; a CR before LF is dropped
 *   from lines 1, 2 and 4 of both texts.  Malformed text of either input: the code and message of bfq_fastq_run, prefixed by
 *   "A: " or "B: ".
 * Pairing: read i of A with read i of B.  With h_permz / perm_fd (a BFQPERM1 container: what bfq_fastq_reorder_keep writes for
 *   the run that produced B's order) record j of B is compared with record perm[j] of A.  Every read index the call reports
 *   (first_changed_read, bfq_compare_diff.read, messages) is A's.  The container is validated and inverted on the device as in
 *   bfq_fastq_restore_ordered, with its refusals: another N (both numbers named), a bad entry (first offending position named).
 * Refusals, BFQ_E_ARG unless said otherwise; *rep is zeroed and h_diffs untouched then: the record counts differ (both are
 *   named); a read's sequence length differs between A and B (the smallest such A index and both lengths are named).  Device
 *   memory: the two texts + about 160 bytes of index per read + 16 bytes per diff record asked for (min(cap_diffs, the bases
 *   the text can hold)), reserved once; above ws_cap_mib: BFQ_E_NOMEM with the size in the message.  An input pair larger than
 *   device memory is not split.
 * Counting: a position differs when the base bytes differ, the quality bytes differ, or both (n_diffs).  bases_changed counts
 *   byte inequality ('a' against 'A' is a change); reads_*_changed count the reads with at least one such position.  d =
 *   (int) qual_b - (int) qual_a: quals_raised d > 0, quals_lowered d < 0, qual_abs_sum / qual_sq_sum / qual_abs_max over |d|.
 *   pos_len[p] = compared positions that fall in bin p: the denominator of pos_bases (base changed), pos_quals (quality
 *   changed) and pos_abs (sum of |d|).
 * Headers: a header is the header line without its line end.  same: equal bytes; dropped: B's header is exactly "@" and A's
 *   is not (what a run without --headers writes); changed: any other inequality.  The three sum to n_reads.
 * Diff list: the first min(n_diffs, cap_diffs) differing positions in ascending (read, pos) go to h_diffs; nothing is written
 *   beyond them.  cap_diffs = 0 with h_diffs = NULL is the plain report.
 * Every sum is an integer sum: the report is exact and does not depend on the launch geometry.
 *   bfq_fastq_compare   : host buffers (pinned: direct DMA); h_permz NULL / permz_len 0: no permutation
 *   bfq_fastq_compare_fd: open files; perm_fd < 0: no permutation */
#define BFQ_CMP_SYMS 6      /* classes of a base byte: A C G N T (the project's order) = 0..4, every other byte = 5 */
#define BFQ_CMP_POS  512    /* position bins: position p of a read counts in bin min(p, 511) */
typedef struct bfq_compare_diff { uint64_t read; uint32_t pos; uint8_t base_a, base_b, qual_a, qual_b; } bfq_compare_diff; /* 16 bytes */
typedef struct bfq_compare_report {
    uint64_t n_reads, total_bases;
    uint64_t n_diffs;                 /* positions where the base or the quality differs */
    uint64_t reads_changed, reads_bases_changed, reads_quals_changed;
    uint64_t bases_changed, quals_changed, quals_raised, quals_lowered;
    uint64_t qual_abs_sum, qual_sq_sum, qual_abs_max;      /* of d = (int) qual_b - (int) qual_a */
    uint64_t first_changed_read;      /* smallest read index with a difference, UINT64_MAX: none */
    uint64_t headers_same, headers_dropped, headers_changed;
    uint64_t subst[BFQ_CMP_SYMS * BFQ_CMP_SYMS];           /* [6 * class(base_a) + class(base_b)], every position: sums to total_bases */
    uint64_t qual_hist_a[256], qual_hist_b[256];           /* every quality byte of A / of B */
    uint64_t changed_base_qual_hist[256];                  /* qual_a at the positions whose base changed */
    uint64_t pos_len[BFQ_CMP_POS], pos_bases[BFQ_CMP_POS], pos_quals[BFQ_CMP_POS], pos_abs[BFQ_CMP_POS];
    uint64_t reserved[8];
} bfq_compare_report;
int bfq_fastq_compare   (bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb,
                         const uint8_t *h_permz, uint64_t permz_len,
                         bfq_compare_report *rep, bfq_compare_diff *h_diffs, uint64_t cap_diffs);
int bfq_fastq_compare_fd(bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, int perm_fd, uint64_t permz_len,
                         bfq_compare_report *rep, bfq_compare_diff *h_diffs, uint64_t cap_diffs);
/* ---- bases back exactly: a run's base edits as a side file, the opt-in container "BFQEDIT1" (k_edits.hip, bfq_edits.hip;
 * tests/edits_model.py states it in Python).  A run changes few bases (0.26 % at 30 M x 150); keeping the input's byte at those
 * positions beside the smoothed output makes the bases lossless while the DNA stream keeps its ratio.
 * An edit is (g, byte): g = the index of a base in the collection's read order -- base j of read r has g = read_off[r] + j, no
 * newline or terminator counted --, byte = the INPUT's byte there.  Edits are strictly ascending in g.  All fields little endian.
 *   header, 64 bytes: "BFQEDIT1" | u64 N (reads) | u64 T (bases) | u64 E (edits) | u32 S = 1024 | u32 flags = 0 | u64 shape |
 *                     u64 target_sum | u64 payload (bytes after the header).  shape = sum over the reads of fmix64(r 65536 + len_r),
 *                     target_sum = sum over the edits of fmix64(g 256 + b), b = the byte the RUN'S OUTPUT holds at g; both mod
 *                     2^64, fmix64 = MurmurHash3's 64-bit finaliser (the reorder key's).  T <= 2^56, E <= T.
 *   segment table   : a segment is S consecutive edits (the last may be shorter), nseg = ceil(E / S).  u64 first[nseg], the g of
 *                     each segment's first edit, then u8 w[nseg], zero-padded to a multiple of 8 bytes.
 *   gaps            : the gap of edit k is g_k - g_(k-1) - 1 >= 0.  A segment of c edits packs its c - 1 gaps (its first edit
 *                     has none: `first` states it) w bits each, gap j in bits [j w, (j + 1) w) of the segment's bit stream, bit b
 *                     being bit b % 64 of word b / 64 (BFQPERM1's order).  Every segment starts on a fresh u64 word and
 *                     zero-pads its last one: ceil((c - 1) w / 64) words.
 *   bytes           : the E input bytes in order, zero-padded to a multiple of 8.
 *   w is canonical  : the bit length of the segment's largest gap, 0 when it has none or all are 0.  The container is a function
 *                     of the edit list: the host form, the device form and the Python model give identical bytes.  E = 0 is a
 *                     valid container of 64 bytes.
 * Well formed: the magic, S = 1024, flags = 0, T <= 2^56, E <= T, every w <= 56, the stated length exact, all padding of the
 * table and of the bytes zero -- faults of the header and the table, found before any edit is looked at; first_bad is then
 * UINT64_MAX, except for a w above 56, whose first_bad is the first edit of that segment.  Then, per edit: every w canonical and
 * the padding bits of a segment's last word zero (both charged to the segment's first edit), `first` above the position of the
 * edit before it (that is: the positions strictly ascending), every g < T, every byte in 33..126.  The first offending edit
 * is the smallest such k.
 * Several members may follow one another, one per block of a sharded run, like every other stream of an archive: member m's
 * positions (and its read indexes in `shape`) count from the first base (read) after the members before it.  N is bounded by
 * nothing in the file (reads may be empty): whoever applies members holds every member's N and T against the reads and bases
 * the target has left behind the members before it, before either sizes a copy or a launch; sums of N or T over members
 * saturate at UINT64_MAX instead of wrapping.
 * Host only (no GPU; the statement the kernels are tested against; messages: bfq_edits_host_error(), per thread):
 *   bfq_edits_bound      : a capacity that always suffices for E edits in T bases (0 when T > 2^56 or E > T)
 *   bfq_edits_member_len : bytes of the first member of the buffer, -1 when its header or table is not well formed
 *   bfq_edits_info       : the sums of N, T and E over all members and their number; BFQ_E_ARG naming the member whose header or
 *                          table is wrong (the edits are not looked at)
 *   bfq_edits_encode     : the edit list -> one member; BFQ_E_ARG and nothing written when cap is too small, a position is
 *                          >= T or not above the one before it, or a byte is outside 33..126
 *   bfq_edits_decode     : ONE member of exactly len bytes -> h_pos[E], h_byte[E] and the header's fields (any may be NULL);
 *                          BFQ_E_ARG and nothing written when it is not well formed (*first_bad as above) or cap_entries < E
 *   bfq_fastq_edits_host : two plain FASTQ texts in the same read order, A the run's input, B its output -> the member.  One
 *                          thread; refusals as bfq_fastq_edits
 *   bfq_fastq_unedit_host: a plain FASTQ text and the members of its edits -> the text with the input's bases, every other
 *                          byte as it was.  Refusals as bfq_fastq_unedit
 * On the device:
 *   bfq_edits_make_device : both base arrays in device memory, reads back to back, read r at d_read_off[r] of both (the layout
 *                           of bfq_run_reads_device); the member goes to d_out (device memory too).  d_read_off[0] != 0,
 *                           d_read_off[N] != total, a read longer than BFQ_MAX_READ_LEN or offsets that are not ascending
 *                           (the first such read named): BFQ_E_ARG before a base is read; bfq_edits_apply_device likewise.  cap too small: BFQ_E_ARG, the
 *                           message holds the size that suffices, stats->bytes too, nothing is written.
 *   bfq_edits_apply_device: the members (host memory) unpacked and validated on the device, then written into d_bases: a base
 *                           array as above, or, lines != 0, a line stream (read r at d_read_off[r] + r).
 *   bfq_fastq_edits / _device / _fd: two FASTQ texts in the same read order (each 1..BFQ_MAX_PARTS parts taken as one, a BGZF
 *                           part is inflated, a part without its final newline gets one, CR before LF dropped: as
 *                           bfq_fastq_compare takes them; _device: one plain text each, in device memory) -> the member.
 *                           Refusals, BFQ_E_ARG with *out_len = 0 and nothing written (a file left empty): the record counts
 *                           differ (both named); a read's sequence length differs (the smallest such read and both lengths
 *                           named); a differing byte of A outside 33..126 (the edit named); cap too small (the size named).
 *                           The _fd form has no capacity: it makes the member in input length / 8 + 4096 bytes and, should
 *                           that not do (more than about a tenth of the bases differ), once more in the size that suffices.
 *   bfq_fastq_unedit / _fd: one FASTQ text (plain or BGZF) and one or more members -> the text with the input's bases,
 *                           otherwise byte for byte the (inflated) text; the members' reads and bases must add up to the
 *                           text's.  Refusals, BFQ_E_ARG and nothing written (the file left empty): bytes that are no members;
 *                           a damaged member (the member and its first offending edit named); N, T or shape that are not the
 *                           text's (the message names both numbers); a target_sum that is not that of the text's bytes at the
 *                           edit positions: "the text is not the output these edits were made from".
 *   A pass proves the pairs fit and sums `shape`; a pass counts the differing bytes per read, 8 bytes per lane, 16 lanes per
 *   read; an exclusive scan; a pass writes (g, byte) in order; one wave per segment finds the largest gap and packs.  The way
 *   back: positions by a wave scan per segment, one atomic min for the first offending edit, one lane per edit finds its read
 *   by binary search in the read offsets; nothing is written before every check of every member has passed.  Device memory:
 *   the texts + their indexes + 12 bytes per read + about 18 bytes per edit (make) / 25 (apply).
 * bfq_fastq_run_job_edits (bfq_job_edits: out_edits / cap_edits / edits_bytes) makes the member of a job's run in the same call, from the parsed
 * input bases and the output bases while both are still on the device -- in the fused, pile and capped modes alike; without
 * out_edits no kernel of these is launched.
 * bfq_fastq_restore_edited / _fd: bfq_fastq_restore_ordered / _fd with an optional permutation (h_permz NULL and permz_len 0 /
 * perm_fd < 0: none) and optional edits (h_edits NULL and edits_len 0 / edits_fd < 0: none): read-order containers as
 * bfq_fastq_restore takes them, with the members that the jobs of the same blocks wrote to out_edits, back to back in block
 * order.  After the streams have been checked (their messages come first) and the permutation validated, the members are held
 * against the decoded DNA lines -- reads, bases, shape, target_sum, with the refusals of bfq_fastq_unedit -- and the input's
 * bytes written into them; then the text is formatted once.  The edits are in the order of the run, the permutation is
 * applied after them.  Nothing is written to h_out / out_fd on any refusal.  The grouped restore takes no edits: a text
 * restored group by group goes through bfq_fastq_unedit. */
typedef struct bfq_edit_stats { uint64_t reads, bases, edits, reads_touched, bytes; } bfq_edit_stats;
uint64_t bfq_edits_bound(uint64_t n_edits, uint64_t total_bases);
int64_t  bfq_edits_member_len(const uint8_t *h_edits, uint64_t len);
int bfq_edits_info(const uint8_t *h_edits, uint64_t len, uint64_t *n_reads, uint64_t *total_bases, uint64_t *n_edits, uint64_t *members);
int bfq_edits_encode(const uint64_t *h_pos, const uint8_t *h_byte, uint64_t n_edits, uint64_t n_reads, uint64_t total_bases,
                     uint64_t shape, uint64_t target_sum, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_edits_decode(const uint8_t *h_edits, uint64_t len, uint64_t *h_pos, uint8_t *h_byte, uint64_t cap_entries,
                     uint64_t *n_reads, uint64_t *total_bases, uint64_t *n_edits, uint64_t *shape, uint64_t *target_sum,
                     uint64_t *first_bad);
const char *bfq_edits_host_error(void);
int bfq_fastq_edits_host(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, uint8_t *h_out, uint64_t cap,
                         uint64_t *out_len, bfq_edit_stats *stats);
int bfq_fastq_unedit_host(const uint8_t *text, uint64_t len, const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out,
                          uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats);
int bfq_edits_make_device(bfq_ctx *c, const uint8_t *d_in_bases, const uint8_t *d_out_bases, const uint64_t *d_read_off, uint64_t N,
                          uint64_t total, uint8_t *d_out, uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats);
int bfq_edits_apply_device(bfq_ctx *c, const uint8_t *h_edits, uint64_t edits_len, uint8_t *d_bases, const uint64_t *d_read_off,
                           uint64_t N, uint64_t total, int lines, bfq_edit_stats *stats);
int bfq_fastq_edits(bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb, uint8_t *h_out, uint64_t cap,
                    uint64_t *out_len, bfq_edit_stats *stats);
int bfq_fastq_edits_device(bfq_ctx *c, const uint8_t *d_a, uint64_t a_len, const uint8_t *d_b, uint64_t b_len, uint8_t *d_out,
                           uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats);
int bfq_fastq_edits_fd(bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, int out_fd, uint64_t *out_len,
                       bfq_edit_stats *stats);
int bfq_fastq_unedit(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out,
                     uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats);
int bfq_fastq_unedit_fd(bfq_ctx *c, int text_fd, uint64_t len, int edits_fd, uint64_t edits_len, int out_fd, uint64_t *out_len,
                        bfq_edit_stats *stats);
int bfq_fastq_restore_edited(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                             const uint8_t *h_hdr, uint64_t hdr_len, const uint8_t *h_permz, uint64_t permz_len,
                             const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads);
int bfq_fastq_restore_edited_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                int perm_fd, uint64_t permz_len, int edits_fd, uint64_t edits_len, int out_fd, uint64_t *out_len,
                                uint64_t *n_reads);
/* ---- which k-mers a run removed, kept and created: the k-mer spectrum of one FASTQ text, or of two side by side (k_kmers.hip,
 * bfq_kmers.hip; tests/kmers_model.py states it in Python).  bfq_fastq_compare says how much a run touched; this says whether
 * what it touched was noise: a sequencing error makes up to k k-mers that occur once, a real allele makes k-mers that occur
 * about as often as the coverage, so a run that does its job removes weak k-mers and loses no solid ones.  Nothing is paired:
 * the report does not depend on the order of the reads, and the texts may hold different numbers of records.
 * Inputs: A and B exactly as bfq_fastq_compare* takes them (1..BFQ_MAX_PARTS parts read as one text, a part without its final
 *   newline gets one, a BGZF part is inflated, four lines per record, a CR before the LF dropped; malformed text: the parser's
 *   code and message, prefixed "A: " or "B: ").  B may be absent (nb = 0, b_fd < 0, b NULL): every B field is then 0 and the
 *   call is the spectrum of one file.
 * Windows: k consecutive bytes of a sequence line; valid when all k are one of A C G T (upper case).  Any other byte breaks
 *   the windows that hold it: those count in windows_skipped_*.  A read shorter than k has no window and counts in reads_short_*
 *   (so windows + windows_skipped = the sum of len - k + 1 over the reads of at least k bases).
 * Coding: A 0, C 1, G 2, T 3, the first base most significant: a window is a 2k-bit integer.  Its k-mer is min(that value, the
 *   value of its reverse complement); with opts.canonical = 0 the forward value.  Even k is allowed (a palindrome is its own
 *   reverse complement and counts once per window).  k: 8..31.
 * Report: with cA / cB the number of windows of A / B whose k-mer is x, over the distinct x of both texts:
 *   distinct_a (cA > 0), distinct_b, distinct_both, only_a (cB = 0), only_b, occ_only_a (the sum of cA where cB = 0), occ_only_b,
 *   distinct_changed (cA != cB); hist_a[min(cA, 255)] for cA > 0 and hist_b likewise (bin 0 stays 0); joint[16 * min(cA, 15) +
 *   min(cB, 15)]; trans[3 * class(cA) + class(cB)] with the classes absent (0), weak (1 .. solid - 1), solid (>= solid), solid =
 *   opts.solid, 2..15: trans[6], "solid lost", is the number to look at first.  k, solid and canonical are the options as
 *   taken; n_partitions says in how many value ranges the k-mers were sorted (below).  Every field is a 64-bit integer sum:
 *   the report is exact and depends neither on the launch geometry nor on the partitioning.
 * List: the k-mers whose class pair is solid -> absent or absent -> solid, in ascending value, with their counts (saturating
 *   at 2^32 - 1): n_listed of them exist, the first min(n_listed, cap_list) go to h_list, nothing is written beyond them.
 *   cap_list = 0 with h_list = NULL is the plain report.
 * opts (NULL: k 21, solid 3, canonical 1, part_records 0); reserved != 0: BFQ_E_ARG.
 * How: one pass over the sequence lines where they lie in the staged texts counts the valid windows and their histogram over
 *   the top 12 bits of the k-mer (4096 bins, A and B together).  The host cuts the bins into ascending ranges -- a bin joins the
 *   range before it while the range's records stay within part_records (0: what the memory below allows; a range is never
 *   smaller than one non-empty bin, empty bins belong to nobody) -- and per range: the windows in range are counted per read,
 *   scanned and emitted as 12-byte sort records, sorted on the whole 2k-bit key by the suffix sort's radix passes (2k <= 40:
 *   ceil(2k / 8) passes; above: the bits below the top 40 first, one re-keying kernel, then five passes), and the runs of equal
 *   k-mers are counted.  The ranges ascend, so the sums and the list simply continue from one to the next.
 * Device memory: the two texts as staged + about 172 bytes of index per read of both (bfq_fastq_index, and 12 bytes for the
 *   per-read counts and their scan) + 16 bytes per list entry asked for (min(cap_list, the valid windows)) + per record of
 *   the largest range 2 x 12 bytes for the sort's two buffers, 12 x 256 bytes per radix block and 36 bytes per 2048 records for
 *   the run counts.  Above ws_cap_mib: the ranges get smaller; when the texts and their index alone, or one bin, do not fit:
 *   BFQ_E_NOMEM with the size in the message (a bin's records are named).  A range holds less than 2^32 records.
 * Refusals: k or solid out of range, cap_list without a buffer: BFQ_E_ARG.  On every refusal *rep is zeroed and h_list untouched.
 *   bfq_fastq_kmers      : host buffers (pinned: direct DMA)
 *   bfq_fastq_kmers_fd   : open files; b_fd < 0: no B
 *   bfq_fastq_kmers_host : one thread of the host, plain text only, no context and no GPU: the same report and list.  It
 *                          states the algorithm and is what the tests compare with; NO entry point falls back to it.  Message:
 *                          bfq_kmers_host_error() (of the calling thread).
 *   bfq_kmers_geometry   : introspection: the rows of a workgroup's chunk when the runs of the sorted records are found, the
 *                          runs of a workgroup's chunk when they are counted and listed, the start positions one lane owns. */
typedef struct bfq_kmer_opts { uint32_t k, solid, canonical, reserved; uint64_t part_records; } bfq_kmer_opts;   /* 24 bytes */
typedef struct bfq_kmer_entry { uint64_t kmer; uint32_t count_a, count_b; } bfq_kmer_entry;                      /* 16 bytes */
typedef struct bfq_kmer_report {
    uint64_t k, solid, canonical, n_partitions;
    uint64_t n_reads_a, n_reads_b, reads_short_a, reads_short_b;
    uint64_t windows_a, windows_b, windows_skipped_a, windows_skipped_b;
    uint64_t distinct_a, distinct_b, distinct_both, only_a, only_b, occ_only_a, occ_only_b, distinct_changed;
    uint64_t n_listed;
    uint64_t hist_a[256], hist_b[256];                     /* distinct k-mers by multiplicity, bin 255: >= 255 */
    uint64_t joint[16 * 16];                               /* [16 * min(cA, 15) + min(cB, 15)] */
    uint64_t trans[3 * 3];                                 /* [3 * class in A + class in B] */
    uint64_t reserved[8];
} bfq_kmer_report;
int bfq_fastq_kmers     (bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb, const bfq_kmer_opts *opts,
                         bfq_kmer_report *rep, bfq_kmer_entry *h_list, uint64_t cap_list);
int bfq_fastq_kmers_fd  (bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, const bfq_kmer_opts *opts,
                         bfq_kmer_report *rep, bfq_kmer_entry *h_list, uint64_t cap_list);
int bfq_fastq_kmers_host(const uint8_t *a, uint64_t a_len, const uint8_t *b, uint64_t b_len, const bfq_kmer_opts *opts,
                         bfq_kmer_report *rep, bfq_kmer_entry *h_list, uint64_t cap_list);
const char *bfq_kmers_host_error(void);
int bfq_kmers_geometry(uint64_t *seg_chunk_rows, uint64_t *run_chunk_runs, uint64_t *lane_starts);
/* ---- bgzip-compressed input: BGZF inflated on the device (k_bgzf.hip; the format and every bound: csrc/bfq_bgzf.h).
 * A BGZF file (bgzip, htslib, BCL Convert) is a chain of independent gzip members of at most 64 KiB in and out; each states
 * its size in its header ('B','C' subfield) and its CRC32 and raw size (ISIZE) in its trailer, so the place of every
 * member's text is known before a byte is decoded.  One wave64 inflates one member: stored, fixed and dynamic blocks.
 * There is no host inflate.  Plain gzip -- one member, no blocks to inflate side by side -- is refused with a message of its
 * own that says to recompress with bgzip.
 *   bfq_bgzf_probe : 1 when h begins with a well-formed BGZF member header, else 0.  A FASTQ text begins with '@', never
 *     with 1f 8b.  Host only.
 *   bfq_bgzf_index : the directory -- member i lies at [in_off, in_off + in_len) and inflates to [out_off, out_off + out_len)
 *     of the text; *raw_len = the length of the text = the sum of the ISIZE fields.  Fills min(*n_members, cap) entries; m may
 *     be NULL to size.  BFQ_E_ARG when a member header is refused: *n_members = the members before it, *raw_len theirs,
 *     *bad_off = where the refused member starts.  A file need not end with the 28-byte EOF member.  Host only.
 *   bfq_bgzf_inflate* : the text of h_in[0, len).  Capacity: cap >= the raw length (bfq_bgzf_index) -- every size that follows
 *     from an input's length follows from its RAW length when the input is BGZF; a smaller cap is BFQ_E_ARG, nothing written.
 *     Device memory: the compressed bytes + 24 bytes per member (+ the text, for the host and file forms), in the workspace.
 *       bfq_bgzf_inflate        : host buffer out (pinned: direct DMA)
 *       bfq_bgzf_inflate_device : device buffer out; the text never exists on the host
 *       bfq_bgzf_inflate_fd     : open files; out_fd < 0: inflate and verify only
 * Refusals: BFQ_E_ARG, bfq_last_error() = "damaged BGZF input: member <i> at byte <off>: <reason>", the lowest failing member
 *   of the file, one reason per rule: header (not gzip; FLG != 4; a subfield past XLEN; no BC subfield; member size below
 *   XLEN + 20 or past the end of the input; ISIZE > 65536) and payload (bits needed past the payload; output past ISIZE; a
 *   distance before the member's first byte; over-subscribed or incomplete code lengths -- the single one-bit distance code
 *   and the empty distance set of a literal-only block stand; symbols 286 / 287 / 30 / 31; no end-of-block code; a repeat with
 *   nothing before it or past HLIT + HDIST; HLIT > 286 or HDIST > 30; stored LEN != ~NLEN or past the payload; block type 3;
 *   length != ISIZE; CRC32 mismatch; payload bytes after the final block).  A refused member writes nothing outside its own
 *   [out_off, out_off + out_len); the output of a refused call is undefined in the members' ranges and untouched beyond the raw
 *   length.  The context stays usable.
 * Transparent input: a text source that begins with 1f 8b is taken as BGZF wherever these take FASTQ text -- memory or
 *   descriptor -- and is inflated into the device text instead of uploaded: bfq_fastq_run, bfq_fastq_run_streams,
 *   bfq_fastq_run_job (any part, mixed with plain parts), bfq_fastq_build_ebwt, bfq_fastq_build_ebwt_fd, both sides of
 *   bfq_fastq_compare*.  A part that lacks its final newline gets one, as a plain part does.  Capacity rules: wherever a
 *   comment above says that the input length ("len", "the input length", "len / 2 + 64") is enough for an output or bounds
 *   it, read the RAW length + 1 per BGZF part (bfq_bgzf_index) for such a source: eBWT / QS rows <= (raw + 1) / 2 + 64, the
 *   streams <= raw + 1 each, the FASTQ text <= raw + 16 + 5 per part; bfq_fastq_rows_estimate() estimates from the first
 *   member.  Refusals of such a source: as bfq_bgzf_inflate ("A: " / "B: " in front in the compare).
 * bfq_fastq_reorder* and bfq_glob_begin do not take BGZF parts: BFQ_E_ARG with a message that says "inflate first". */
typedef struct bfq_bgzf_member { uint64_t in_off, out_off; uint32_t in_len, out_len; } bfq_bgzf_member;
int bfq_bgzf_probe(const uint8_t *h, uint64_t len);
int bfq_bgzf_index(const uint8_t *h_in, uint64_t len, bfq_bgzf_member *m, uint64_t cap, uint64_t *n_members,
                   uint64_t *raw_len, uint64_t *bad_off);
int bfq_bgzf_inflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_bgzf_inflate_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *out_len);
int bfq_bgzf_inflate_fd(bfq_ctx *c, int in_fd, uint64_t len, int out_fd, uint64_t *out_len);
/* ---- plain gzip input: one long deflate stream per member, inflated side by side on the device (k_gzip.hip; the format,
 * the algorithm and every bound: csrc/bfq_gzip.h).  What gzip, pigz, bcl2fastq and `cat a.gz b.gz` write: any number of
 * RFC 1952 members (FEXTRA, FNAME, FCOMMENT, FHCRC with its CRC16 checked; reserved FLG bits refused), zero bytes allowed
 * after the last one.  A member has no directory, so the work is found and proved instead of read:
 *   1 the compressed bytes are cut into pieces of `chunk` bytes; in every piece after the first the device looks for the
 *     first bit offset that passes the block-start rule (BFINAL 0, BTYPE 2, a dynamic header that passes every check of the
 *     inflate): the piece's candidate;
 *   2 pass 1: one decoder per candidate (and one at the first member's first block) runs block by block and counts, until a
 *     block ends exactly on a later candidate (its landing), the stream ends, or an error.  The host walks the landings from
 *     piece 0: the chain.  Decoders off the chain started on false candidates and are discarded; correctness rests on the
 *     chain and on every member's CRC32, never on a candidate;
 *   3 pass 2: the chain's decoders write 16-bit symbols (a byte, or a marker for a byte of the unknown 32 KiB in front of the
 *     decoder); one workgroup resolves the 32 KiB window in front of every chain decoder in order; one streaming pass turns
 *     symbols into bytes; every member's CRC32 and length (mod 2^32) are checked against its trailer.
 *   chunk : a power of two >= 512; 0 = the default (131 072, or $BFQ_GZIP_CHUNK); anything else is BFQ_E_ARG.
 *   bfq_gzip_probe   : 1 when h begins with a well-formed gzip member header (BGZF included), else 0.  Host only.
 *   bfq_gzip_measure : steps 1-2 only: *raw_len = the length of the text, *n_members, *stats.  CRC32 and far distances are
 *     not checked by it.
 *   bfq_gzip_inflate* : the text.  cap < the raw length: BFQ_E_ARG, nothing written, *out_len = the length needed (every other
 *     failure leaves *out_len = 0).  Device memory, in the workspace: the compressed bytes, 56 bytes per piece, 2 x the raw
 *     length of symbols, 32 KiB per chain decoder, 24 bytes per member (+ the text, for the host and file forms).
 *       bfq_gzip_inflate        : host buffer out
 *       bfq_gzip_inflate_device : device buffer out
 *       bfq_gzip_inflate_fd     : open files; out_fd < 0: inflate and verify only
 *   bfq_gzip_inflate_host : the same steps by one thread, with no context and no GPU: the same bytes and the same *stats as
 *     the device gives.  It states the algorithm and is what the tests compare with; NO entry point falls back to it.
 *   stats (may be NULL): members, pieces, decoders started, decoders of the chain, candidates the chain ran past, decoders
 *     discarded.
 * A BGZF file is a gzip file and goes through the same general path here; bfq_bgzf_* stays the fast way for it.
 * Refusals: BFQ_E_ARG, bfq_last_error() = "damaged gzip input: member <i> at byte <off>: <reason>" (<off>: where the member's
 *   header begins).  A structural error -- header or deflate data, the reasons of bfq_bgzf_inflate where the rule is the same,
 *   and: reserved flag bits, header CRC16, a header field past the end, trailing bytes that are neither zero nor a member, the
 *   input ending inside a trailer -- at the lowest place in the stream is named first; CRC32 and length mismatches only when
 *   there is none, lowest member first.  bfq_gzip_inflate_host returns BFQ_E_ARG and leaves the same message in
 *   bfq_gzip_host_error() (of the calling thread's last call).  The text of a refused call is undefined; the context stays usable.
 * The entry points that take FASTQ text keep reading 1f 8b as BGZF and keep refusing plain gzip: their buffers are sized
 * from a raw length that is known before any GPU work, which plain gzip cannot give.  Inflate first. */
typedef struct bfq_gzip_stats { uint64_t members, pieces, decoders, chain, skipped, discarded; } bfq_gzip_stats;
int bfq_gzip_probe(const uint8_t *h, uint64_t len);
int bfq_gzip_measure(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint64_t *raw_len, uint64_t *n_members, bfq_gzip_stats *stats);
int bfq_gzip_inflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                     bfq_gzip_stats *stats);
int bfq_gzip_inflate_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                            bfq_gzip_stats *stats);
int bfq_gzip_inflate_fd(bfq_ctx *c, int in_fd, uint64_t len, uint64_t chunk, int out_fd, uint64_t *out_len, bfq_gzip_stats *stats);
int bfq_gzip_inflate_host(const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                          bfq_gzip_stats *stats);
const char *bfq_gzip_host_error(void);
/* ---- BAM input: the records of a BAM file as FASTQ text, made on the device (k_bam.hip; the format, the record check, the
 * record-start rule and every bound: csrc/bfq_bam.h).  Unaligned BAM (GATK, DRAGEN, instrument software) and aligned BAM
 * alike.  A BAM file is a BGZF file: bfq_bgzf_inflate puts its inflated stream into device memory; a source that begins
 * with "BAM\1" itself is taken as that stream and uploaded as it is.  Records are length-prefixed, so the work is found
 * and proved as for plain gzip:
 *   1 the stream behind the header (walked on the host, any size, up to 2^20 references) is cut into pieces of opts.piece
 *     bytes; in every piece behind the first the device looks for the lowest offset that passes the record-start rule (a
 *     well-formed record with pos, next_pos >= -1 and a printable name, followed by another or by the end): a heuristic;
 *   2 one walker per piece hops from record to record up to the first record at or behind the piece's end (its landing),
 *     checks every record and counts records, kept records and text bytes per output;
 *   3 the host walks the landings from the header's end: the chain.  A piece whose walker did not start at the chain's
 *     landing (a false start, even one that fell back into step; or no walker) is walked again from there, one round
 *     each.  Exactness rests on the chain: every record on it has passed the record check;
 *   4 prefix sums of the chain's counts place every piece's text; a second walk writes it, a wave64 per piece, the lanes
 *     sharing each record's bytes.
 * What a record becomes (this project's definition, modelled on the defaults of `samtools fastq`; parity with samtools is
 * not pinned by a test):  flag & exclude_flags != 0: left out.  "@name" ["/1" | "/2" with mate_suffix, where exactly one of
 * READ1 0x40 / READ2 0x80 is set] \n sequence (=ACMGRSVTWYHKDBN) \n + \n phred + 33 \n.  Flag 0x10: reverse complement
 * (=TGKCYSBAWRDMHVN) and reversed qualities.  A quality above 93 is written '~' (clamped_quals); absent qualities (0xFF)
 * become default_qual + 33 (no_qual counts the records).  split: READ1-only records to output 1, READ2-only to output 2,
 * the rest to output 0 -- else everything to output 0 -- each in file order.  paired_check (needs split): refused unless
 * outputs 1 and 2 hold the same number of records and their k-th names are equal (compared on the device):
 * "unpaired BAM input: pair <k>: <what>; collate the file by name first".  A kept record is l_read_name + 2 l_seq + 5
 * bytes of text, + 2 with a suffix.
 *   opts (NULL: the defaults): exclude_flags 0x900, mate_suffix 1, default_qual 1 (0..93), split 0, paired_check 0,
 *     piece 0 = the default (65 536; 64 .. 2^30).  The texts and all statistics but pieces .. rounds do not depend on piece.
 *   bfq_bam_probe   : 1 for "BAM\1", or a BGZF file whose first member inflates to a text that begins so (inflated on the
 *     host), else 0.  Host only.
 *   bfq_bam_measure : steps 1-3: exact out_len[3], n_reads[3] and *stats; nothing is written.
 *   bfq_bam_to_fastq* : the texts.  A cap[k] below the measured length: BFQ_E_ARG, nothing written, out_len[] = the lengths
 *     needed (every other failure leaves them 0).  Device memory, in the workspace: the compressed bytes, the inflated
 *     stream, 168 bytes per piece, 8 bytes per record of outputs 1 and 2 with paired_check, and -- for the host and file
 *     forms -- 4/3 of the stream for the texts.
 *       bfq_bam_to_fastq        : host buffers out
 *       bfq_bam_to_fastq_device : device buffers out; the text never exists on the host
 *       bfq_bam_to_fastq_fd     : open files; an out_fd[k] < 0 is not written
 *   bfq_bam_to_fastq_host : the same steps by one thread on the INFLATED stream raw[0, raw_len), with no context and no
 *     GPU: the same bytes and the same *stats.  It states the algorithm and is what the tests compare with; NO entry point
 *     falls back to it.  Its message: bfq_bam_host_error() (of the calling thread's last call).
 *   stats (may be NULL): records of the file, written[3], skipped (excluded), reversed, no_qual, clamped_quals (of the kept
 *     records), n_ref, header_bytes, pieces, walkers started by the rule (piece 0's included), dead (walkers that met a
 *     record failing the check), repaired (pieces walked again), rounds (1 + repaired).
 * Refusals: BFQ_E_ARG, "damaged BAM input: record <i> at byte <off of the inflated stream>: <reason>" for a record that
 *   fails the check on the chain (block size below 32 / above 2^24 / past the end of the stream -- a stream that ends inside
 *   a record --, l_read_name 0, the fields not fitting the block, a name without its NUL or with one inside, a reference
 *   index outside [-1, n_ref)); BFQ_E_TOO_LONG with the same words for l_seq > BFQ_MAX_READ_LEN; "damaged BAM input: header at
 *   byte <off>: <reason>"; a refusal of the BGZF layer keeps the BGZF message.  With paired_check the device form may have
 *   written text before the names are refused; the host and file forms write nothing.  The context stays usable.
 * The entry points that take FASTQ text keep reading 1f 8b as BGZF-compressed FASTQ: BAM is taken by these calls only. */
typedef struct bfq_bam_opts { uint32_t exclude_flags, mate_suffix, default_qual, split, paired_check, piece, check_names, reserved; } bfq_bam_opts;
typedef struct bfq_bam_stats {
    uint64_t records, written[3], skipped, reversed, no_qual, clamped_quals, n_ref, header_bytes, pieces, walkers, dead, repaired, rounds;
} bfq_bam_stats;
/* Aux tags into the header line -- this project's definition, modelled on `samtools fastq -T` (csrc/bfq_bam.h states it in
 * full).  opts->reserved == BFQ_BAM_OPTS_TAGS: opts points to a bfq_bam_tag_opts, read by bfq_bam_measure, bfq_bam_to_fastq,
 * _device, _fd and _host (bfq_bam_patch* ignores it; any other value of reserved is ignored as before).  Behind the name and
 * its suffix every selected tag of a kept record is written as \tXX:T:value, in the record's order: A as XX:A:c, c C s S i I
 * as XX:i:<decimal>, Z and H as XX:Z: / XX:H:<bytes>.  n_tags 0: every tag; else the tags of tag[0, n_tags) (at most 32,
 * each [A-Za-z][A-Za-z0-9], else BFQ_E_ARG before any work).  A selected tag of type f or B, one whose Z / H value or A
 * character holds a byte outside [0x20, 0x7e], and one whose key is not [A-Za-z][A-Za-z0-9] is left out and counted
 * (tags_dropped) -- with strict refused, nothing written: "BAM tags: record <i> at byte <off>: tag <XX> of type <T> cannot
 * be carried".  The tag area of every kept record must parse (a known type, every value inside the block, a NUL for every
 * Z / H), else "damaged BAM input: record <i> at byte <off>: malformed tag area".  *stats (may be NULL): tags_written,
 * tags_dropped, tag_bytes (the bytes of text the tags took).  With tags the host and file forms reserve 5/2 of the stream
 * for the texts. */
#define BFQ_BAM_OPTS_TAGS 0x31474154u
typedef struct bfq_bam_tag_stats { uint64_t tags_written, tags_dropped, tag_bytes; } bfq_bam_tag_stats;
typedef struct bfq_bam_tag_opts { bfq_bam_opts o; uint32_t n_tags, strict; uint8_t tag[32][2]; bfq_bam_tag_stats *stats; } bfq_bam_tag_opts;
void bfq_bam_default_opts(bfq_bam_opts *o);
int bfq_bam_probe(const uint8_t *h, uint64_t len);
int bfq_bam_measure(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint64_t out_len[3], uint64_t n_reads[3],
                    bfq_bam_stats *stats);
int bfq_bam_to_fastq(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                     uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats);
int bfq_bam_to_fastq_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint8_t *const d_out[3], const uint64_t cap[3],
                            uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats);
int bfq_bam_to_fastq_fd(bfq_ctx *c, int in_fd, uint64_t len, const bfq_bam_opts *opts, const int out_fd[3], uint64_t out_len[3],
                        uint64_t n_reads[3], bfq_bam_stats *stats);
int bfq_bam_to_fastq_host(const uint8_t *raw, uint64_t raw_len, const bfq_bam_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                          uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats);
const char *bfq_bam_host_error(void);
/* ---- BAM output: "this BAM, with the reads of these FASTQ texts in it" (k_bam_patch.hip; the definition in full, the two
 * walks and the host form: csrc/bfq_bam_patch.h).  The way back of bfq_bam_to_fastq*: the sequence and quality lines of up
 * to three plain FASTQ texts are written into the SEQ and QUAL fields of the records they came from; the header, every
 * other field, every tag and every record that meets no read stay byte for byte, every record keeps its size.
 *   Inputs: a BAM source as bfq_bam_to_fastq* takes it (BGZF, or the inflated stream itself); opts with the same meaning
 *     as on the way in; text[k], k = 0, 1, 2.  The i-th kept record of output k -- the record bfq_bam_to_fastq with the same
 *     options writes as read i of output k -- meets read i of text[k].  A NULL text[k] leaves the records of output k as they
 *     are (a paired run that dropped the "neither READ1 nor READ2" records); excluded records are never touched.
 *   The text is plain FASTQ: one that begins with 1f 8b is refused ("inflate the text first").  CR before LF is stripped.
 *     The header line is used only with opts.check_names (the first word behind piece; 0 keeps the earlier meaning, and the
 *     way in ignores it): a run without kept headers writes "@" alone.
 *   Bases: case-insensitive over =ACMGRSVTWYHKDBN to their nibbles; any other byte becomes 15 (N; unknown_bases).  Flag 0x10:
 *     text base i goes to position l_seq - 1 - i as its complement.  The spare nibble of an odd length keeps its value.
 *   Qualities: char - 33, reversed under 0x10.  The record's value stays where the text says 93 ('~') and the record holds
 *     more (kept_high_quals); absent qualities (0xFF) stay absent when every quality of the read is default_qual + 33
 *     (kept_absent), else all l_seq values are written.  So the texts of the way in, patched back, give the same stream.
 *   Refusals, all BFQ_E_ARG, nothing written, the context stays usable: "BAM patch: text <k> is compressed ..."; the FASTQ
 *     refusals ("FASTQ: number of lines is not a multiple of 4", "FASTQ: len(DNA) != len(QS) in a record"); "BAM patch: text
 *     <k> holds <n> reads, the BAM file holds <m> records for it"; "BAM patch: text <k> read <i>: <n> bases, record <r> at
 *     byte <off> holds <m>" and, with check_names, "BAM patch: text <k> read <i>: the name differs from that of record <r>
 *     at byte <off>" (the name: the bytes behind '@' up to the first blank, less the "/1" or "/2" mate_suffix adds) -- of
 *     the offending records the one that comes first in the file is named, by the device (atomicMin) as by the host form.
 *     A damaged BAM keeps the messages of the way in.
 *   The result: a valid BAM with the same header and the same records in the same order with the same sizes.  The BGZF
 *     layer is this project's (bfq_bgzf_deflate: members cut at 65 280 bytes of stream whatever the input's cut was, the EOF
 *     member at the end), so an index (.bai, .csi) of the input does NOT fit the output, and the MD and NM tags of an
 *     aligned record go stale where a base changed: they are copied like every tag.  Parity with an htslib tool is not
 *     pinned by a test.
 *       bfq_bam_patch_host   : one thread on the INFLATED stream, no context, no GPU: states the algorithm and is what the
 *         tests compare with; NO entry point falls back to it.  cap < raw_len: BFQ_E_ARG.  Message: bfq_bam_host_error().
 *       bfq_bam_patch_device : texts in device memory; the patched inflated stream into d_out_raw (cap < the stream's
 *         length: BFQ_E_ARG, nothing written, *raw_len = the length needed).  Not compressed.
 *       bfq_bam_patch        : host texts in, the BGZF-compressed BAM into a host buffer; level as for bfq_bgzf_deflate; a
 *         cap below bfq_bgzf_deflate_bound(raw length): BFQ_E_ARG, nothing written, *out_len = that bound.
 *       bfq_bam_patch_fd     : open files; a text_fd[k] < 0 is an absent text; out_fd is sized to *out_len.
 *     The stream is deflated where it lies: it never crosses to the host uncompressed.  Device memory, in the workspace and
 *     reserved once: the compressed bytes, the stream, 8 bytes per text line, 232 bytes per piece, the deflate batch; texts
 *     that are uploaded (or lie at an address that is no multiple of 16) go into the context's text buffer beside it.
 *   stats (may be NULL): records of the file, patched[k] (records that met a read of text k), skipped (the others), reversed
 *     (patched, 0x10), reads_changed, bases_changed / quals_changed (positions whose stored value differs from before),
 *     unknown_bases, kept_high_quals, kept_absent, raw_len, pieces, repaired.  Only the last two depend on opts.piece. */
typedef struct bfq_bam_patch_stats {
    uint64_t records, patched[3], skipped, reversed, reads_changed, bases_changed, quals_changed, unknown_bases, kept_high_quals, kept_absent, raw_len,
             pieces, repaired;
} bfq_bam_patch_stats;
int bfq_bam_patch_host(const uint8_t *raw, uint64_t raw_len, const bfq_bam_opts *opts, const uint8_t *const text[3], const uint64_t text_len[3],
                       uint8_t *out_raw, uint64_t cap, bfq_bam_patch_stats *stats);
int bfq_bam_patch_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, const uint8_t *const d_text[3],
                         const uint64_t text_len[3], uint8_t *d_out_raw, uint64_t cap, uint64_t *raw_len, bfq_bam_patch_stats *stats);
int bfq_bam_patch(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, const uint8_t *const h_text[3], const uint64_t text_len[3],
                  int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len, bfq_bam_patch_stats *stats);
int bfq_bam_patch_fd(bfq_ctx *c, int bam_fd, uint64_t len, const bfq_bam_opts *opts, const int text_fd[3], int level, int out_fd, uint64_t *out_len,
                     bfq_bam_patch_stats *stats);
/* ---- unaligned BAM output: "these FASTQ texts as an unaligned BAM" (k_ubam.hip; the definition in full, both passes and
 * the host form: csrc/bfq_ubam.h).  Unlike the patch above it needs no BAM to write into: records are made, not edited.  It
 * is this project's definition, modelled on the defaults of `samtools import`; parity with an htslib tool is not pinned by a
 * test.
 *   Inputs: text[k], k = 0, 1, 2, with the meaning of the outputs of bfq_bam_to_fastq*.  Unpaired: text[0] alone, every
 *     record flag 4.  Paired: text[1] and text[2] together -- record 2i is read i of text[1] (flag 77), record 2i + 1 read i of
 *     text[2] (flag 141) --, an optional text[0] behind all pairs (flag 4).  A text that begins with 1f 8b is refused
 *     ("inflate the text first"); CR before LF is stripped; a last line without its LF counts.
 *   Name: the bytes behind '@' up to the first blank, tab or line end; the rest of the header line is dropped
 *     (comments_dropped).  With mate_suffix a trailing "/1" of a text[1] name and "/2" of a text[2] name is removed where at
 *     least one byte remains.  An empty name ("@" alone: a run without kept headers) becomes the read's 1-based index in
 *     decimal -- both mates share theirs, the reads of text[0] count on behind the pairs -- (named).  paired_check: the names
 *     of read i of text[1] and text[2] are compared after the suffix removal.
 *   Record: refID -1, pos -1, mapq 0, bin 4680, no CIGAR, next_refID -1, next_pos -1, tlen 0.  SEQ: case-insensitive over
 *     =ACMGRSVTWYHKDBN, any other byte 15 (unknown_bases), the spare nibble of an odd length 0; l_seq may be 0.  QUAL: char - 33,
 *     always written: absent qualities cannot come back from a text, so BAM -> text -> BAM is an identity only for records
 *     that held qualities <= 93 and no tags.  Tags: none, or RG:Z:<rg_id> on every record.  A record is 36 + (l_name + 1) +
 *     ceil(l_seq / 2) + l_seq bytes, + 4 + strlen(rg_id): the stream's length is exact before anything is written.
 *   Header: header_text[0, header_len) as it is -- the caller's to make valid, e.g. the header text of the original BAM --,
 *     or with header_text NULL "@HD\tVN:1.6\tSO:unsorted\n" and, with rg_id, "@RG\tID:<rg_id>\n".  n_ref is 0.
 *   Refusals, nothing written, the context stays usable.  BFQ_E_ARG: "FASTQ to BAM: text <k> is compressed ..."; "FASTQ:
 *     number of lines is not a multiple of 4"; "FASTQ to BAM: text 1 holds <n> reads, text 2 holds <m>" (one mate text
 *     absent, or differing counts); "FASTQ: len(DNA) != len(QS) in a record"; "FASTQ to BAM: text <k> read <i>: <reason>" for
 *     a header line that does not begin with '@', a name above 254 bytes or with a byte outside [!-?A-~], a name that
 *     differs from its mate's (paired_check), a third line that does not begin with '+', a quality byte outside [33, 126];
 *     an rg_id that is empty, above 255 bytes or holds a byte outside [ -~]; a level other than 0 or 1.  BFQ_E_TOO_LONG: "...
 *     read longer than 65000 bases".  Of all offending reads the one whose record would come first in the file is named, by
 *     the device (one atomicMin) as by the host form.
 *   The BGZF layer is this project's (bfq_bgzf_deflate: members cut at 65 280 bytes of stream, the EOF member at the end);
 *   opts.level as for bfq_bgzf_deflate.
 *       bfq_fastq_to_bam_measure : host texts in; *raw_len = the exact length of the stream, n_reads[3], *stats (without
 *         unknown_bases, which the writing pass counts); nothing is written.
 *       bfq_fastq_to_bam_host    : one thread, no context, no GPU, the stream out (not compressed): states the algorithm and
 *         is what the tests compare with; NO entry point falls back to it.  cap below the length: BFQ_E_ARG, nothing written,
 *         *raw_len = the length needed.  Message: bfq_ubam_host_error() (of the calling thread's last call).
 *       bfq_fastq_to_bam_device  : texts in device memory, the stream into d_out_raw, not compressed; cap as above.
 *       bfq_fastq_to_bam         : host texts in, the BGZF file into a host buffer; a cap below bfq_bgzf_deflate_bound(stream
 *         length): BFQ_E_ARG, nothing written, *out_len = that bound.
 *       bfq_fastq_to_bam_fd      : open files; a text_fd[k] < 0 is absent; out_fd is sized to *out_len (0 on a refusal).
 *       bfq_fastq_restore_bam_fd : bfq_fastq_restore_fd (perm_fd < 0) or bfq_fastq_restore_ordered_fd with the restored text
 *         turned into records (unpaired) and those deflated where they lie: containers in, uBAM out; the FASTQ text never
 *         exists on the host.  The grouped restore has no such form; the two archives of a paired run restore to two texts
 *         and go through bfq_fastq_to_bam_fd.
 *     The stream is deflated where it lies: it never crosses to the host uncompressed.  Device memory, in the workspace and
 *     reserved once: 8 bytes per text line (and 12 per 4 KiB of text while they are indexed), 12 bytes per record, the stream,
 *     the deflate batch; texts that are uploaded (or lie at an address that is no multiple of 16) go into the context's text
 *     buffer beside it.
 *   stats (may be NULL): records, written[k] (records made of text k), named, comments_dropped, unknown_bases, raw_len,
 *     members (of the BGZF file: ceil(raw_len / 65280) + 1). */
typedef struct bfq_ubam_opts {
    uint32_t mate_suffix, paired_check, level, reserved;
    const uint8_t *header_text; uint64_t header_len;
    const char *rg_id;
} bfq_ubam_opts;
typedef struct bfq_ubam_stats { uint64_t records, written[3], named, comments_dropped, unknown_bases, raw_len, members; } bfq_ubam_stats;
/* Aux tags out of the header line -- this project's definition, modelled on `samtools import -T` (csrc/bfq_ubam.h states it
 * in full).  opts->reserved == BFQ_UBAM_OPTS_TAGS: opts points to a bfq_ubam_tag_opts, read by every entry point that takes
 * a bfq_ubam_opts (any other value of reserved is ignored as before).  Behind the name the header line is cut at tabs (a
 * name ended by a space: the bytes up to the first tab are a comment and dropped).  A field [A-Za-z][A-Za-z0-9]:[AiZH]:value
 * -- A: one byte of [ -~]; i: an optional '-' and 1..10 digits within [-2^31, 2^32 - 1], stored at the smallest width (C S I
 * / c s i); Z: bytes of [ -~]; H: an even number of hex digits -- becomes a tag of the record, in line order, between QUAL and
 * the RG tag of rg_id, when n_tags is 0 or it is one of tag[0, n_tags) (at most 32, each [A-Za-z][A-Za-z0-9], else BFQ_E_ARG
 * before any work).  Every other field is dropped and counted (fields_dropped), never refused; so is an RG field when rg_id
 * is set.  comments_dropped then counts the reads of which some byte behind the name did not become a tag.  *stats (may be
 * NULL): tags_written, fields_dropped, tag_bytes (the bytes of stream the tags took).  BAM -> text (every tag) -> BAM (tags
 * on, header_text the original's) gives the stream back byte for byte for uBAM records of flags 4 / 77 / 141 with qualities
 * <= 93 whose tags are of types A / Z / H or integers at their smallest width, with printable values. */
#define BFQ_UBAM_OPTS_TAGS 0x32474154u
typedef struct bfq_ubam_tag_stats { uint64_t tags_written, fields_dropped, tag_bytes; } bfq_ubam_tag_stats;
typedef struct bfq_ubam_tag_opts { bfq_ubam_opts o; uint32_t n_tags, pad; uint8_t tag[32][2]; bfq_ubam_tag_stats *stats; } bfq_ubam_tag_opts;
void bfq_ubam_default_opts(bfq_ubam_opts *o);
int bfq_fastq_to_bam_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint64_t *raw_len,
                             uint64_t n_reads[3], bfq_ubam_stats *stats);
int bfq_fastq_to_bam_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *out_raw, uint64_t cap,
                          uint64_t *raw_len, bfq_ubam_stats *stats);
const char *bfq_ubam_host_error(void);
int bfq_fastq_to_bam_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *d_out_raw,
                            uint64_t cap, uint64_t *raw_len, bfq_ubam_stats *stats);
int bfq_fastq_to_bam(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_ubam_opts *opts, uint8_t *h_out, uint64_t cap,
                     uint64_t *out_len, bfq_ubam_stats *stats);
int bfq_fastq_to_bam_fd(bfq_ctx *c, const int text_fd[3], const bfq_ubam_opts *opts, int out_fd, uint64_t *out_len, bfq_ubam_stats *stats);
int bfq_fastq_restore_bam_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len, int perm_fd,
                             uint64_t permz_len, const bfq_ubam_opts *opts, int out_fd, uint64_t *out_len, bfq_ubam_stats *stats);
/* ---- interleaved paired FASTQ: one text with the mates alternating <-> the two texts of mates (k_pairs.hip; the definition
 * in full, the key rule, the messages and the host forms: csrc/bfq_pairs.h).  What `bwa mem -p`, fastp --interleaved_in and
 * `samtools fastq` without -1 -2 read and write.  Records move verbatim: a record is its four lines byte for byte (header
 * comment, '+' line and CRs included); a text whose last line lacks its LF gets one.
 *   The text: plain FASTQ, parsed by the line index and record parser of bfq_fastq_reorder; malformed text keeps the words
 *     of bfq_fastq_run ("FASTQ: number of lines is not a multiple of 4", "FASTQ: len(DNA) != len(QS) in a record",
 *     BFQ_E_TOO_LONG "read longer than BFQ_MAX_READ_LEN").  A text that begins with 1f 8b: BFQ_E_ARG, "... inflate the text
 *     first" (bfq_bgzf_inflate*, bfq_gzip_inflate*): these calls take no compressed parts.
 *   Key of a record: the bytes behind '@' up to the first blank, tab, CR or line end; with mate_suffix a trailing "/1" or "/2"
 *     is removed -- either one, at either position, where at least one byte remains (laxer than bfq_fastq_to_bam, which
 *     removes only the matching suffix: in orphan mode a record's role is not known before the pairing).  Keys compare in
 *     full at any length; two empty keys ("@" alone) are equal.
 *   opts (NULL: the defaults): check_names 1, mate_suffix 1, orphans 0; reserved != 0: BFQ_E_ARG.
 *   bfq_fastq_deinterleave* : one text -> out[3]: 0 singletons, 1 and 2 the mates.
 *     orphans 0: an odd record count N: BFQ_E_ARG "interleaved FASTQ: <N> records, an odd number".  Record 2k to output 1,
 *       record 2k + 1 to output 2, output 0 empty.  check_names: "interleaved FASTQ: pair <k> (records <2k> and <2k+1>): the
 *       names differ", the first offending pair of the file (compared on the device, one atomicMin).
 *     orphans 1: the file is cut into maximal runs of consecutive records with equal keys; in a run that starts at record s
 *       with r records, s + 2j and s + 2j + 1 are a pair for 2j + 1 < r (outputs 1 and 2); with r odd the run's last record
 *       goes to output 0, in file order.  Nothing is refused for pairing; check_names is implied.  The run start of every
 *       record is an inclusive max-scan over the whole file.
 *   bfq_fastq_interleave* : text[3] -> one text: record k of text[1], record k of text[2], for every k, then the records of
 *     an optional text[0] (a NULL text, or text_fd < 0, holds no reads).  "FASTQ interleave: text 1 holds <n> reads, text 2
 *     holds <m>"; check_names: "FASTQ interleave: pair <k>: the names differ".
 *   Every refusal is BFQ_E_ARG but the too-long read, writes nothing in every form -- sizes and checks are finished before
 *   the first byte moves; the device forms write straight into the caller's buffers after them -- and leaves the context
 *   usable.  Output lengths are exact before anything is written.
 *       _measure : host text(s) in; out_len, n_reads[3] (reads per output; of the merge: per input text) and *stats; nothing
 *                  is written.
 *       plain    : host buffers.  A cap[k] below the measured length: BFQ_E_ARG, nothing written, out_len[] = the lengths
 *                  needed (every other failure leaves them 0).
 *       _device  : device buffers in and out; the text never exists on the host.  cap as above.
 *       _fd      : open files; an out_fd[k] < 0 is not written; output files are sized to their text (0 on a failure).
 *       _host    : one thread, no context, no GPU: the same bytes, stats and messages.  States the algorithm and is what the
 *                  tests compare with; NO entry point falls back to it.  Message: bfq_pairs_host_error() (of the calling
 *                  thread's last call).
 *   Device memory: the input text(s) (in the context's text buffer when uploaded, or when a device text lies at an address
 *   that is no multiple of 16 or lacks its final LF), and in the workspace, reserved once: 8 bytes per line and 44 per
 *   record of index, 16 per pair (orphans: 57 per record) of sizes and offsets, and -- host and file forms -- the outputs.
 *   Above ws_cap_mib: BFQ_E_NOMEM with the size in the message.
 *   stats (may be NULL): records, pairs, singles, out_len[3] (of the merge: out_len[0] = the interleaved text's length). */
typedef struct bfq_pairs_opts  { uint32_t check_names, mate_suffix, orphans, reserved; } bfq_pairs_opts;
typedef struct bfq_pairs_stats { uint64_t records, pairs, singles, out_len[3]; } bfq_pairs_stats;
void bfq_pairs_default_opts(bfq_pairs_opts *o);
int bfq_fastq_deinterleave_measure(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const bfq_pairs_opts *opts, uint64_t out_len[3], uint64_t n_reads[3],
                                   bfq_pairs_stats *stats);
int bfq_fastq_deinterleave(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                           uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats);
int bfq_fastq_deinterleave_device(bfq_ctx *c, const uint8_t *d_text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const d_out[3], const uint64_t cap[3],
                                  uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats);
int bfq_fastq_deinterleave_fd(bfq_ctx *c, int in_fd, uint64_t len, const bfq_pairs_opts *opts, const int out_fd[3], uint64_t out_len[3],
                              uint64_t n_reads[3], bfq_pairs_stats *stats);
int bfq_fastq_deinterleave_host(const uint8_t *text, uint64_t len, const bfq_pairs_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                                uint64_t out_len[3], uint64_t n_reads[3], bfq_pairs_stats *stats);
int bfq_fastq_interleave_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint64_t *out_len,
                                 uint64_t n_reads[3], bfq_pairs_stats *stats);
int bfq_fastq_interleave(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *h_out, uint64_t cap,
                         uint64_t *out_len, bfq_pairs_stats *stats);
int bfq_fastq_interleave_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *d_out,
                                uint64_t cap, uint64_t *out_len, bfq_pairs_stats *stats);
int bfq_fastq_interleave_fd(bfq_ctx *c, const int text_fd[3], const bfq_pairs_opts *opts, int out_fd, uint64_t *out_len, bfq_pairs_stats *stats);
int bfq_fastq_interleave_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_pairs_opts *opts, uint8_t *out, uint64_t cap,
                              uint64_t *out_len, bfq_pairs_stats *stats);
const char *bfq_pairs_host_error(void);
/* ---- repair paired FASTQ: the mates matched by name across files, wherever they stand (k_pairs.hip, the repair section;
 * the definition: csrc/bfq_pairs.h).  For mate files that were filtered on their own, for the text of a coordinate-sorted BAM
 * (bfq_bam_to_fastq without -1 -2, then this call with the text as text[0]) and for any mixed or shuffled interleaved file.
 *   The texts: text[1], text[2] and text[0] as in bfq_fastq_interleave (a NULL text, or text_fd < 0, holds no reads); plain
 *     FASTQ with the parsing, the messages and the 1f 8b refusal of the merge ("FASTQ repair: text <k> is compressed ...").
 *     A record is its four lines byte for byte.  The global number g of a record counts the records of text 1, then those of
 *     text 2, then those of text 0.
 *   Key: as above, with mate_suffix.  Hint of a record: 1 from text 1, 2 from text 2; from text 0, with mate_suffix, 1 where
 *     the key lost "/1" and 2 where it lost "/2"; else 0.
 *   Group: all records of the call with equal keys (compared in full), split in global order by hint into L1, L2 and L0.
 *     Pairs: (L1[k], L2[k]) for k < min(|L1|, |L2|), then (L0[2j], L0[2j+1]) for 2j + 1 < |L0|; the first record of a pair
 *     goes to out[1], the second to out[2], every other record of the group to out[0].
 *   Order: pairs in increasing global number of their out[1] record (a repaired R1 keeps R1's order), singletons in increasing
 *     global number.  The outputs are a function of the texts and mate_suffix only: neither hash_bits nor seed shows in them.
 *   opts (NULL: the defaults): mate_suffix 1, hash_bits 40 (1..40, else BFQ_E_ARG), seed 0; reserved != 0: BFQ_E_ARG.  The
 *     records are sorted (stable radix passes, ceil(hash_bits / 8) of them) by the top hash_bits bits of a 64-bit hash of the
 *     key (csrc/bfq_pairs.h states it) and each run of equal sort keys is cut into groups by the full hash and then the key's
 *     bytes.  A run of more than 1024 records: BFQ_E_ARG, "FASTQ repair: more than 1024 records share a name or a name hash
 *     (the first: record <i> of text <k>): names do not identify the mates" -- <i>: the smallest global number in such a
 *     run, relative to its text.  The bound limits every loop of the grouping; a file of "@"-only headers is refused by it.
 *     Small hash_bits force runs with several names in them: a knob for tests.
 *   Every refusal writes nothing in any form and leaves the context usable; all sizes are exact before the first byte moves.
 *       _measure : host texts in; out_len[3], n_reads[3] (reads per output) and *stats; nothing is written.
 *       plain    : host buffers.  A cap[k] below its length: BFQ_E_ARG, nothing written, out_len[] = the lengths needed.
 *       _device  : device buffers in and out, written straight after the last check.  A device text at an address that is no
 *                  multiple of 16, or without its final LF, is copied first.
 *       _fd      : open files; an out_fd[k] < 0 is not written; output files are sized to their text (0 on a failure).
 *       _host    : one thread, no context, no GPU: the same bytes, stats and messages.  States the algorithm; NO entry point
 *                  falls back to it.  Message: bfq_pairs_host_error().
 *   Device memory: the texts as for the merge; in the workspace, reserved once from the counted lines: 8 bytes per line and
 *   44 per record of index, 83 per record of hashes, sort records, roles, ranks, sizes and offsets, and -- host and file forms
 *   -- the outputs.  Above ws_cap_mib: BFQ_E_NOMEM with the size in the message.
 *   stats (may be NULL): records, pairs, singles, out_len[3], n_in[3] (records per input text), dup_groups (groups of more
 *   than two records), mixed_runs (runs of equal sort key with more than one name), max_run (the longest run). */
typedef struct bfq_repair_opts  { uint32_t mate_suffix, hash_bits; uint64_t seed; uint32_t reserved[2]; } bfq_repair_opts;
typedef struct bfq_repair_stats { uint64_t records, pairs, singles, out_len[3], n_in[3], dup_groups, mixed_runs, max_run; } bfq_repair_stats;
void bfq_repair_default_opts(bfq_repair_opts *o);
int bfq_fastq_repair_measure(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint64_t out_len[3],
                             uint64_t n_reads[3], bfq_repair_stats *stats);
int bfq_fastq_repair(bfq_ctx *c, const uint8_t *const h_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint8_t *const h_out[3],
                     const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats);
int bfq_fastq_repair_device(bfq_ctx *c, const uint8_t *const d_text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint8_t *const d_out[3],
                            const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats);
int bfq_fastq_repair_fd(bfq_ctx *c, const int text_fd[3], const bfq_repair_opts *opts, const int out_fd[3], uint64_t out_len[3], uint64_t n_reads[3],
                        bfq_repair_stats *stats);
int bfq_fastq_repair_host(const uint8_t *const text[3], const uint64_t text_len[3], const bfq_repair_opts *opts, uint8_t *const h_out[3],
                          const uint64_t cap[3], uint64_t out_len[3], uint64_t n_reads[3], bfq_repair_stats *stats);
/* ---- exact duplicate removal: reads, or pairs, with equal sequences leave one unit behind (k_dedup.hip; the definition and
 * the host form: csrc/bfq_dedup.h).  What clumpify's dedupe, fastuniq, seqkit rmdup -s and fastp --dedup do.
 *   The texts: text[0] holds mate 1 or the single-end file, text[1] mate 2 (NULL, or text_fd < 0: single-end); plain FASTQ with
 *     the parsing, the messages and the 1f 8b refusal of bfq_fastq_interleave ("FASTQ dedup: text <k> is compressed ...").  In
 *     paired form the k-th records of the two texts are one unit; unequal record counts: BFQ_E_ARG, "FASTQ dedup: text 0 holds
 *     <n> reads, text 1 holds <m>".  A record is its four lines byte for byte; the global number g of a unit is its record index.
 *   Key of a unit: the bytes of the sequence line without its LF and without one trailing CR; paired: the ordered pair of the
 *     mates' keys, lengths included -- ("AC","G") != ("A","CG"), (x,y) != (y,x).  Bytes compare as they are (case matters, N
 *     equals N); header, '+' line and qualities are no part of the key.
 *   Group: all units of the call with equal keys.  Kept unit of a group: keep = 0, the smallest g; keep = 1, the largest score
 *     and among equals the smallest g; score = the sum of max(byte - 33, 0) over every quality byte of the unit (both mates;
 *     the LF and one trailing CR are no quality bytes), a 64-bit sum.
 *   out[0] / out[1]: the kept units' records in increasing g; dup[0] / dup[1]: every other unit's, in increasing g (optional:
 *     absent, they are counted and not written).  The outputs are a function of the texts and keep only.
 *   opts (NULL: the defaults): keep 0 (> 1: BFQ_E_ARG), hash_bits 40 (1..40, else BFQ_E_ARG), seed 0; reserved != 0: BFQ_E_ARG.
 *     The units are sorted (stable radix passes) by the top hash_bits bits of a 64-bit hash of the key (csrc/bfq_dedup.h states
 *     it); each run of equal sort keys is cut into groups in rounds: every unresolved unit is compared -- full hash, lengths,
 *     bytes -- with its run's current head and joins it or proposes itself as the next head.  A run holds one sequence on real
 *     data: one round.  The number of EQUAL units is not bounded; a run with more than 1024 DIFFERENT keys is refused after
 *     round 1024: BFQ_E_ARG, "FASTQ dedup: more than 1024 different sequences share a hash (the first: record <g>)" -- <g>: the
 *     smallest global number in such a run.  Small hash_bits force runs with several keys: a knob for tests.
 *   Every refusal writes nothing in any form and leaves the context usable; all sizes are exact before the first byte moves.
 *       _measure : host texts in; out_len[2], dup_len[2] and *stats; nothing is written.
 *       plain    : host buffers.  A cap below its length: BFQ_E_ARG, nothing written, out_len[] / dup_len[] = the lengths needed.
 *                  h_dup == NULL: the removed records are counted (dup_len[]) and not written, and dup_cap is not read.
 *       _device  : device buffers in and out.  A device text at an address that is no multiple of 16, or without its final
 *                  LF, is copied first.
 *       _fd      : open files; out_fd[0] < 0, or in paired form out_fd[1] < 0: BFQ_E_ARG ("bad file descriptor"), the kept
 *                  records need a place; dup_fd == NULL or dup_fd[k] < 0: not written; output files are sized to their text (0
 *                  on a failure).
 *       _host    : one thread, no context, no GPU: the same bytes, stats and messages.  States the algorithm; NO entry point
 *                  falls back to it.  Message: bfq_dedup_host_error().
 *   Device memory: the texts as for the merge; in the workspace, reserved once from the counted lines: 8 bytes per line and
 *   44 per record of index, 114 per unit of hashes, scores, sort records, heads, groups and flags (then, in the same space, 32
 *   of sizes and offsets), and -- host and file forms -- the outputs.  Above ws_cap_mib: BFQ_E_NOMEM with the size in the message.
 *   stats (may be NULL): units, kept, removed, dup_groups (groups of >= 2), max_group, max_group_first (the smallest g in the
 *   largest group, the smallest such g among equals; 0 without units), level_groups[k] / level_units[k]: the groups of
 *   2^k <= size < 2^(k+1) and the units in them (FastQC's duplication levels, exact; k = 31 takes everything above),
 *   out_len[2], dup_len[2]; and three that depend on hash_bits and seed: mixed_runs (runs with more than one key), max_run
 *   (the longest run), rounds. */
typedef struct bfq_dedup_opts  { uint32_t keep, hash_bits; uint64_t seed; uint32_t reserved[2]; } bfq_dedup_opts;
typedef struct bfq_dedup_stats { uint64_t units, kept, removed, dup_groups, max_group, max_group_first, level_groups[32], level_units[32], out_len[2], dup_len[2],
                                          mixed_runs, max_run, rounds; } bfq_dedup_stats;
void bfq_dedup_default_opts(bfq_dedup_opts *o);
int bfq_fastq_dedup_measure(bfq_ctx *c, const uint8_t *const h_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint64_t out_len[2],
                            uint64_t dup_len[2], bfq_dedup_stats *stats);
int bfq_fastq_dedup(bfq_ctx *c, const uint8_t *const h_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const h_out[2],
                    const uint64_t out_cap[2], uint8_t *const h_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                    bfq_dedup_stats *stats);
int bfq_fastq_dedup_device(bfq_ctx *c, const uint8_t *const d_text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const d_out[2],
                           const uint64_t out_cap[2], uint8_t *const d_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                           bfq_dedup_stats *stats);
int bfq_fastq_dedup_fd(bfq_ctx *c, const int text_fd[2], const bfq_dedup_opts *opts, const int out_fd[2], const int dup_fd[2], uint64_t out_len[2],
                       uint64_t dup_len[2], bfq_dedup_stats *stats);
int bfq_fastq_dedup_host(const uint8_t *const text[2], const uint64_t text_len[2], const bfq_dedup_opts *opts, uint8_t *const h_out[2],
                         const uint64_t out_cap[2], uint8_t *const h_dup[2], const uint64_t dup_cap[2], uint64_t out_len[2], uint64_t dup_len[2],
                         bfq_dedup_stats *stats);
const char *bfq_dedup_host_error(void);
/* ---- bgzip-compressed output: BGZF members deflated on the device (k_deflate.hip; the format and every bound:
 * csrc/bfq_deflate.h).  A text of len bytes is cut at multiples of 65 280 bytes (htslib's member size; the cut depends on
 * nothing else); every piece becomes one BGZF member -- htslib's 18-byte header, a raw deflate payload, CRC32 and ISIZE --
 * and the 28-byte EOF member ends the file (an empty text gives exactly those 28 bytes).  Any gzip reader takes the result
 * (htslib, zcat, Python's gzip), and bfq_bgzf_inflate* and every transparent input above do.
 *   payload : matches inside the member only (distance <= 32 768, length 3..258), found through one hash slot per position
 *     and a distance-1 probe, taken greedily where they are estimated to cost fewer bits than their literals; one dynamic
 *     block (code lengths limited to 15, the code-length code to 7, the header run-length coded).  A member whose coded form
 *     would be no shorter than the stored form is one stored block: a member is at most its piece + 31 bytes, and
 *       bfq_bgzf_deflate_bound(len) = len + 31 * ceil(len / 65280) + 28       (host arithmetic; what callers size buffers with)
 *   The output is deterministic: the same text gives the same bytes on every run, with any batch size and grid, and
 *   bfq_bgzf_deflate_host -- the host form of csrc/bfq_deflate.h: one thread, no context, no GPU -- gives the same bytes as
 *   the kernel.  It is the statement of the format and what the tests compare with; NO entry point falls back to it: a call
 *   that cannot run on the device fails.
 *   level : 0 = every member stored, 1 = the compressor; anything else is BFQ_E_ARG.
 *   cap   : cap < bfq_bgzf_deflate_bound(len) is BFQ_E_ARG, nothing written.
 *   An input that begins with 1f 8b is refused (BFQ_E_ARG: "the input is already compressed ...").
 *       bfq_bgzf_deflate        : host text in, host buffer out
 *       bfq_bgzf_deflate_device : device text in (d_in), host buffer out; the text never exists on the host
 *       bfq_bgzf_deflate_fd     : open files (out_fd is sized to *out_len)
 *   The host-memory and file forms work in batches of text: whole members, a default chosen from the arena (6144 members,
 *   fewer under a workspace cap), BFQ_BGZF_BATCH = bytes of text per batch overrides it.  Device memory: one batch of text, a
 *   worst-case slot per member of the batch, 255 KiB of tokens per workgroup of the launch (at most 1536) and two output
 *   buffers -- it does not grow with len.  The output of a batch leaves through the background writers while the next batch
 *   is uploaded and deflated.
 *   bfq_fastq_restore_bgzf_fd : bfq_fastq_restore_fd (perm_fd < 0) or bfq_fastq_restore_ordered_fd (perm_fd >= 0) with the
 *     text deflated where it lies: out_fd receives the BGZF file, *out_len its length, *raw_len the length of the text.  The
 *     FASTQ text never crosses to the host.  The grouped restore has no such form. */
uint64_t bfq_bgzf_deflate_bound(uint64_t len);
int bfq_bgzf_deflate_host(const uint8_t *h_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_bgzf_deflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_bgzf_deflate_device(bfq_ctx *c, const uint8_t *d_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len);
int bfq_bgzf_deflate_fd(bfq_ctx *c, int in_fd, uint64_t len, int level, int out_fd, uint64_t *out_len);
int bfq_fastq_restore_bgzf_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                              int perm_fd, uint64_t permz_len, int level, int out_fd, uint64_t *out_len, uint64_t *raw_len,
                              uint64_t *n_reads);
/* device-resident form (input and output in device memory): bfq_stream_reserve(len) sizes the workspace once */
int bfq_stream_reserve(bfq_ctx *c, uint64_t len);
int bfq_stream_compress_device(bfq_ctx *c, const uint8_t *d_in, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *out_len);

/* ---- profiling: per-kernel HIP-event times accumulated over the calls since
 * the last bfq_prof_reset() (events recorded on bfq_stream()). */
int  bfq_prof_enable(bfq_ctx *c, int on);
void bfq_prof_reset(bfq_ctx *c);
int  bfq_prof_count(bfq_ctx *c);
/* introspection: how bfq_run_reads_device() brings n_rows rows (bases + reads) back to text order by position bins --
 * the window (text positions per workgroup of the last stage) and the shift of a first-level bin (2^shift positions).
 * BFQ_E_ARG (bin_shift -1): more rows than two partition levels hold; such a call inverts by LF walks. */
int  bfq_posbin_geometry(uint64_t n_rows, uint64_t *window, int *bin_shift);
/* introspection: what the position bins of the context's last finished call did.  By default only the rows whose final
 * (base, quality) differs from a default at their position travel: polarity 0 = the default is the input ("keep"), 1 = the
 * input base with the constant quality of M = 2 ("const"; chosen on the device when more than half of the bases were
 * smoothed, or forced by BFQ_POSBIN_POLARITY=keep|const), -1 = the call sent every row (BFQ_POSBIN_SPARSE=0, BFQ_POSBIN_WC=0)
 * or ran no position bins.  rows_sent: the rows that travelled = the output positions that differ from the default. */
int  bfq_posbin_sparse_last(bfq_ctx *c, int *polarity, uint64_t *rows_sent);
/* introspection: how the suffix sort cuts n_rows rows -- the rows of a scatter tile and of a radix block (a whole number of
 * tiles, which one workgroup runs through one after the other; fewer tiles for smaller collections). */
int  bfq_radix_geometry(uint64_t n_rows, uint64_t *tile_rows, uint64_t *block_rows);
/* introspection: which form of the refinement's chunk kernel the context launches, as bfq_create() / bfq_set_params() read it
 * from BFQ_REFINE_PIPE: 1 (default) = a round's text words by two loads side by side, 0 = the third word behind the first two. */
int  bfq_refine_form(bfq_ctx *c);
int  bfq_prof_get(bfq_ctx *c, int idx, char *name, int name_cap, double *total_ms,
                  uint64_t *launches, double *alg_bytes_total);
/* per-launch durations (ms, launch order, since the last reset) of ONE kernel chosen by its bfq_prof_get index (-1: none):
 * bfq_prof_trace copies up to cap of them and returns how many there are -- e.g. the radix passes one by one */
int     bfq_prof_trace_select(bfq_ctx *c, int idx);
int64_t bfq_prof_trace(bfq_ctx *c, float *ms, uint64_t cap);

uint64_t bfq_workspace_bytes(bfq_ctx *c);      /* current device workspace size */
/* Test hook: waits for the context's stream and copies the workspace's bytes [off, off + len) to dst (host memory), cut at the
   workspace's end.  Returns the number of bytes copied.  With BFQ_POISON=<byte> in the environment (read by bfq_create and
   bfq_set_params) the workspace holds that byte everywhere whenever a call starts over in it, and every other device
   allocation of the library holds it when it is made: what a call reads before it has written it is then not zero. */
uint64_t bfq_workspace_read(bfq_ctx *c, uint64_t off, void *dst, uint64_t len);
const char *bfq_version(void);

#ifdef __cplusplus
}
#endif
#endif
