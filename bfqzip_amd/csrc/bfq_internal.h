// bfq_internal.h -- context, workspace arena, profiling and stage entry points
// shared by the .hip translation units of libbfqhip.so.  Not part of the ABI.
#pragma once
#include <stdlib.h>
#include <errno.h>
#include <unistd.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <new>
#include <optional>
#include <string>
#include <vector>
#include <thread>
#include "../../include/bfqzip_hip.h"
#include "bfq_common.h"
#include "bfq_internal_host.h"
#include "bfq_arena.h"
#include "bfq_texts.h"
#include "bfq_outfiles.h"

#define HIP_CHECK(expr)                                                                        \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            throw BfqError{BFQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)};     \
    } while (0)

// ---- kernel ids for the profiler ------------------------------------------------
enum BfqKernel {
    K_TEXT = 0, K_PACK, K_KEYS, K_RADIX_HIST, K_SCAN, K_RADIX_SCATTER, K_HUGE_ROUND, K_CLUSTER_BIG,
    K_REFINE_WAVE, K_REFINE_BIG, K_EMIT, K_RANK_BUILD, K_RANK_FINAL, K_LCP_FLAGS, K_CLUSTER,
    K_INVERT_COUNT, K_INVERT, K_SYNTH, K_FASTQ, K_BFS, K_CODEC, K_MISC, K_RESTORE, K_FQ_FORMAT, K_RO_KEYS, K_RO_GATHER,
    K_FQ_FORMAT_ORD, K_PERM_PACK, K_PERM_INVERT, K_POSBIN_L1, K_POSBIN_L2, K_POSBIN_APPLY, K_POSBIN_CHECK,
    K_CMP_CHECK, K_CMP_COMPARE, K_CMP_EMIT, K_BGZF, K_DEFLATE, K_UBAM_SIZE, K_UBAM_WRITE, K_PAIRS_CMP, K_PAIRS_MOVE,
    K_KM_HIST, K_KM_COUNT, K_KM_EMIT, K_KM_REKEY, K_KM_SEG, K_KM_STATS,
    K_EDIT_CHECK, K_EDIT_COUNT, K_EDIT_WRITE, K_EDIT_SEGW, K_EDIT_PACK, K_EDIT_UNPACK, K_EDIT_LOCATE, K_EDIT_APPLY, K_NUM
};
extern const char *const BFQ_KERNEL_NAMES[K_NUM];

struct ProfRec { int id; hipEvent_t a, b; double bytes; };

#define BFQ_IO_MAX_WORKERS 16
#define BFQ_IO_STAGE_BYTES (16u << 20)

// device-side counters / small outputs read back by the host (one hipMemcpy)
struct DevCounters {
    u64 stats[8];        // bfq_stats cluster counters, same order
    u64 bigCount;        // number of segments > 64 rows
    u64 errSymbol;       // >0: forbidden symbol met
    u64 errInvert;       // >0: LF walk did not close
    u64 errFreq3;        // >0: three frequent symbols in a cluster
    u64 errTooLong;      // >0: read longer than BFQ_MAX_READ_LEN
    u64 tot[6];          // symbol totals of the eBWT: # A C G N T
    u64 mismatch;        // >0: rebuilt eBWT differs from the given one
    u64 nSegs;           // segments of >= 2 rows met by the refinement
    u64 errFastq;        // >0: a record whose quality line is not as long as its sequence
    u64 hugeCount;       // segments above BFQ_HUGE_SEG rows, left to the radix rounds of k_bigseg.hip
    u64 hugeRows;        // their rows
    u64 bigClusters;     // clusters above CL_BIG rows, left to k_cluster_big
    u64 bigTotal;        // segments > 64 rows of the piles already refined (pile mode: bigCount restarts per pile)
    u64 pbPolarity;      // sparse position bins: the polarity level 1 chose + 1 (0: the call ran no sparse stage)
    u64 pbSent;          // ... and the rows it sent
    u64 pad[3];
};

// the tabulated rank queries: one u64 per eBWT row (layout: bfq_rank.h)
struct RankIndex {
    u64 *lfq;               // [n]
    u64 n;
};

// What one top-level call decides for the stages below it.  guarded() starts every call from CallState{} and puts that back
// when the call throws: nothing here survives a call.
struct CallState {
    bool piles = false;             // step 1 runs pile by pile (k_piles.hip): set by the reservation of the current call
    bool capped = false;            // the whole path in position mode, one two-symbol pile at a time (workspace cap): set likewise
    u64 cappedPileRows = 0;         // ... and the rows of the largest pile its arena has room for
    bool keepRecs = false;          // step 1 leaves the packed text and the sorted records' (w1, w2) words in the arena (position mode)
    const u64 *d_w12 = nullptr, *d_text3 = nullptr;
    size_t keepMark = 0;
    size_t writeHint = 0;           // bytes the caller is going to queue in all: sizes the writer pool when it is created
    bool arenaHeld = false;         // the caller reserved the arena for several pieces of work and holds buffers in it (grouped
                                    // restore): bfq_ebwt_decode_lines allocates above the current top and reserves nothing
    // one-shot tools (the *_fd entry points): the eBWT and its qualities live outside the arena (in the text buffer, whose
    // FASTQ text is dead once the reads are gathered), so that the arena can be freed while they are still being written;
    // onRows(start, rows) is called whenever rows [start, start + rows) of the eBWT / QS / LCP are final (pile by pile)
    u8 *extBwt = nullptr, *extQual = nullptr;
    bool lcpScratch = false;        // pile mode: nobody reads the LCP (gsufsort): one pile's worth of scratch instead of 2 n bytes
    std::function<void(u64, u64)> onRows;
};

struct bfq_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copyStream = nullptr;   // device -> host copies that overlap the tail of the inversion
    hipStream_t copy() { if (!copyStream) HIP_CHECK(hipStreamCreateWithFlags(&copyStream, hipStreamNonBlocking)); return copyStream; }   // ... created on first use
    bfq_params P;
    BfqEnv env;                         // the BFQ_* environment as bfq_create() / bfq_set_params() found it
    std::string err;

    // workspace arena (bump allocator, reset per top-level call)
    Arena ws;
    void reserve(size_t bytes);
    void wsFree();
    void adoptWorkspace(char *p, size_t bytes);   // frees the arena: this buffer is the arena now, and the context's to free
    void quiesce() { (void)hipStreamSynchronize(stream); }
    // BFQ_POISON: the byte over the whole arena (a plain memset on the stream, no profiled launch), done when it returns
    void poisonWs()
    {
        if (env.poison < 0 || !ws.base || !ws.cap) return;
        HIP_CHECK(hipMemsetAsync(ws.base, env.poison, ws.cap, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    // an arena being allocated on a helper thread while the caller uploads its input (a one-shot tool's 86 GB can land on
    // memory the driver has not cleared yet: 2 s instead of 0); reserve() joins it and takes it over when it is large enough
    void reserveBegin(size_t bytes);
    void reserveJoin(bool adopt, size_t need);
    std::thread *wsThread = nullptr;
    char *wsPend = nullptr;
    size_t wsPendBytes = 0;
    double wsPendSecs = 0;
    void dropWorkspace();           // frees the arena now (one-shot tools: lets the driver scrub it while outputs are written)
    void *allocBytes(size_t bytes) { return ws.alloc(bytes); }
    template <class T> T *alloc(size_t count) { return (T *)allocBytes(count * sizeof(T)); }
    size_t mark() const { return ws.mark(); }
    void release(size_t m) { ws.release(m); }

    DevCounters *d_cnt = nullptr;   // device
    DevCounters h_cnt;              // host copy
    int pbLastPolarity = -1;        // what the last finished call's sparse position bins did (bfq_posbin_sparse_last): -1 = none ran
    u64 pbLastSent = 0;
    double *d_powtab = nullptr;     // 256 doubles: pow(10,-(q-33)/10) by host libm
    double *d_qthr = nullptr;       // thresholds for round(-10*log10(x))
    int qthrLo = 0, qthrN = 0;

    // last eBWT (device, inside ws)
    u8 *d_bwt = nullptr; u8 *d_qual = nullptr; u16 *d_lcp = nullptr;
    u32 *d_gcnt = nullptr;          // symbol counts per 256-row group, written by k_emit_bwt
    int gcntTerm = -1;              // terminator byte those counts were taken with
    u64 n = 0, N = 0;
    CallState call;
    size_t wsLimit() const { return env.wsCap ? (size_t)env.wsCap : (size_t)(P.ws_cap_mib > 0 ? P.ws_cap_mib : 0) << 20; }

    // profiling
    bool profOn = true;
    std::vector<hipEvent_t> evPool;
    size_t evUsed = 0;
    std::vector<ProfRec> recs;
    double profMs[K_NUM];
    u64 profLaunches[K_NUM];
    double profBytes[K_NUM];
    int profTraceId = -1;               // per-launch times of this kernel id are kept too (bfq_prof_trace), newest last
    std::vector<float> profTrace;
    void profBegin(int id, double bytes);
    void profEnd();
    void profCollect();   // after a stream synchronise

    void sync();
    void fetchCounters();
    void zeroCounters();

    // host <-> device transfers (bfq_io.hip): per-worker stream + two pinned staging buffers
    struct IoWorker { hipStream_t stream = nullptr; char *stage[2] = {nullptr, nullptr}; hipEvent_t done[2] = {nullptr, nullptr}; };
    IoWorker io[BFQ_IO_MAX_WORKERS];
    int ioWorkers = 0;
    void ioInit(int want);          // at least min(want, the thread budget) staging workers exist afterwards
    void ioFree();
    struct BfqWriter *writer = nullptr;  // background device -> host / file writes (bfq_write_async, bfq_io.hip)

    // device copy of the FASTQ text of the current call (outside the arena: its record count sizes the arena);
    // kept between calls, grown when a larger text arrives
    u8 *d_text = nullptr;
    size_t textCap = 0;
    u8 *textBuf(size_t bytes);
    u64 residentLen = 0;            // global mode: length of the block text bfq_glob_begin left in d_text
    bool residentValid = false;
    int residentParts = 0;          // ... and where its parts start (entry residentParts = residentLen)
    u64 residentPstart[BFQ_MAX_PARTS + 1] = {0, 0, 0, 0, 0};
    u64 globN = 0;                  // global mode: the two-symbol pile sizes bfq_glob_pile_counts found for a text of globN rows
    u64 globCounts[36] = {0};
};
using ScopedArena = ScopedArenaT<bfq_ctx>;

// Every device allocation of the library outside the arena is made here (the arena's own two: reserveBegin() and reserve(),
// bfq_api.hip).  BFQ_POISON: filled with the byte once, before anyone sees it.  false: no memory (the HIP error is cleared).
static inline bool bfq_dev_malloc(bfq_ctx *c, void **p, size_t bytes)
{
    *p = nullptr;
    if (hipMalloc(p, bytes) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return false; }
    if (c->env.poison >= 0 && bytes) {
        hipError_t e = hipMemsetAsync(*p, c->env.poison, bytes, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { (void)hipFree(*p); *p = nullptr; throw BfqError{BFQ_E_HIP, std::string("BFQ_POISON fill: ") + hipGetErrorString(e)}; }
    }
    return true;
}
// one device allocation and its hipFree
struct DevBuf {
    char *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { free(); }
    bool tryAlloc(bfq_ctx *c, size_t bytes)
    {
        free();
        return bfq_dev_malloc(c, (void **)&p, bytes);
    }
    void alloc(bfq_ctx *c, size_t bytes, const char *what) { if (!tryAlloc(c, bytes)) throw BfqError{BFQ_E_NOMEM, std::string("device buffer for ") + what}; }
    void free() { if (p) (void)hipFree(p); p = nullptr; }
    char *release() { char *q = p; p = nullptr; return q; }   // to another owner
};
// an event without timing, to order one stream behind another
struct ScopedEvent {
    hipEvent_t e = nullptr;
    ScopedEvent() { HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    ScopedEvent(const ScopedEvent &) = delete; ScopedEvent &operator=(const ScopedEvent &) = delete;
    ~ScopedEvent() { (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};

void bfq_upload(bfq_ctx *c, void *d_dst, HostRef src, size_t len);
void bfq_download(bfq_ctx *c, HostRef dst, const void *d_src, size_t len);
// A text source of a call -- memory or an open file -- measured and placed (bfq_bgzf.hip).  A FASTQ text cannot begin with
// 1f 8b: a source that does is taken as BGZF, its members are inflated into the device text instead of uploaded, and every
// size that follows from a source's length follows from its raw length.
//   bfq_text_measure: per part, whether it is BGZF, its raw length, its directory; bound = what the parts take on the device at
//     most (a part that lacks its final newline gets one; whether a BGZF part does is known only once it is inflated: room is
//     left); stage = bytes of staging behind the text that the BGZF parts need (compressed bytes, directory, status), 0: none.
//   bfq_text_put: the parts back to back at d_dst; pstart[p] = where part p starts, pstart[nparts] = the length of the text.
struct TextSrc { HostRef ref; u64 len; };
struct TextMeasure {
    struct Part { bool bgzf = false; u64 raw = 0; u8 addNl = 0; std::vector<bfq_bgzf_member> dir; };
    Part part[BFQ_MAX_PARTS];
    int nparts = 0;
    u64 bound = 0, stage = 0;
    bool anyBgzf() const { return stage != 0; }
};
void bfq_text_measure(const TextSrc *parts, int nparts, TextMeasure *M);
void bfq_text_put(bfq_ctx *c, const TextSrc *parts, TextMeasure *M, u8 *d_dst, u8 *d_stage, u64 *pstart);
bool bfq_text_is_gzip(const TextSrc &t);        // begins with 1f 8b (the entry points that do not take BGZF refuse by it)
// The plain texts of a call, up to three, staged one way (bfq_texts.hip; the plan and the sizes: bfq_texts.h).  A text is host
// memory or an open file (ref), or device memory (d); neither: absent.
//   bfq_text_peek   n bytes at `off` of a text of any of the three kinds (c may be null for the first two)
//   bfq_texts_look  fills seen[0, n) and allocates nothing: last = false, everything but the last byte; last = true, the last
//                   byte of what was filled before.  Between the two, and before bfq_texts_place, every caller refuses what it
//                   refuses, in its own words and order.
//   bfq_texts_place the text buffer for plan.bufNeed; what moves uploaded or copied there, with its LF where the plan adds one;
//                   the arena reserved for counting; the lines of every present text counted.  out[k]: where text k stands,
//                   its staged length, its lines (newlines + 1); an absent text: nullptr, 0, 0.
struct TextIn {
    HostRef ref; const u8 *d = nullptr; u64 len = 0;
    bool present() const { return d || !ref.null(); }
};
struct TextPlaced { const u8 *d = nullptr; u64 len = 0, lines = 0; };
#define BFQ_LOCAL __attribute__((visibility("hidden")))            // (the library's dynamic symbols stay as they were)
BFQ_LOCAL void bfq_text_peek(bfq_ctx *c, const TextIn &in, u64 off, u8 *dst, size_t n);
BFQ_LOCAL void bfq_texts_look(bfq_ctx *c, const TextIn *in, int n, BfqTextSeen *seen, bool last);
BFQ_LOCAL void bfq_texts_place(bfq_ctx *c, const TextIn *in, const BfqTextPlan &plan, int n, TextPlaced *out);
// the texts of an entry point's arguments: host or device pointers (nullptr: absent), or open files (< 0: absent) mapped into
// map[] (an empty file: a text of no bytes)
static inline void bfq_texts_of(const uint8_t *const *text, const uint64_t *len, bool device, TextIn X[3])
{
    for (int k = 0; k < 3; k++) {
        X[k] = TextIn{};
        if (device) X[k].d = text[k]; else X[k].ref = HostRef::mem(text[k]);
        X[k].len = text[k] ? len[k] : 0;
    }
}
BFQ_LOCAL void bfq_texts_map(const int fd[3], MappedInput map[3], TextIn X[3]);
static inline bool bfq_seen_gzip(const BfqTextSeen &s) { return s.len >= 2 && s.first[0] == 0x1F && s.first[1] == 0x8B; }
// the refusal of a call whose texts, outputs and index do not fit under the workspace cap
[[noreturn]] static inline void bfq_nomem_cap(bfq_ctx *c, const char *whatNeeds, const char *whatItHolds, size_t need)
{
    char b[240];
    snprintf(b, sizeof b, "%s needs %.2f GiB of device memory (%s), above the cap of %.2f GiB (bfq_params.ws_cap_mib / BFQ_WS_CAP)", whatNeeds,
             need / 1073741824.0, whatItHolds, c->wsLimit() / 1073741824.0);
    throw BfqError{BFQ_E_NOMEM, b};
}
void bfq_upload(bfq_ctx *c, void *d_dst, const void *h_src, size_t len);
void bfq_download(bfq_ctx *c, void *h_dst, const void *d_src, size_t len);
// a sink's download to host memory: in the d2h_write phase, and back to gpu
static inline void bfq_download_phase(bfq_ctx *c, void *h_dst, const void *d_src, size_t len)
{
    bfq_phase("d2h_write");
    bfq_download(c, h_dst, d_src, len);
    bfq_phase("gpu");
}
// background writes: the bytes [d_src, d_src + len) as they are once the work queued so far on the context's stream has
// finished go to dst (memory -- e.g. an output mapping -- or a file offset) through the writer's own staging workers; the
// call returns at once.  bfq_write_wait(): all of them have arrived (throws what went wrong).  d_src must stay valid till then.
void bfq_write_async(bfq_ctx *c, HostRef dst, const void *d_src, size_t len);
void bfq_write_wait(bfq_ctx *c);
// upload on a helper thread while the caller goes on launching kernels; join() waits and rethrows
struct BfqAsyncUpload;
BfqAsyncUpload *bfq_upload_begin(bfq_ctx *c, void *d_dst, HostRef src, size_t len);
void bfq_upload_join(BfqAsyncUpload *u);

#define KLAUNCH(ctx, kid, bytes, kernel, grid, block, ...)                                     \
    do {                                                                                       \
        (ctx)->profBegin((kid), (double)(bytes));                                              \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (ctx)->stream, __VA_ARGS__);    \
        (ctx)->profEnd();                                                                      \
        HIP_CHECK(hipGetLastError());                                                          \
    } while (0)

// run `body` of a C-ABI entry point with the usual prologue/epilogue; maps exceptions to error codes
template <class F> static int guarded(bfq_ctx *c, F body)
{
    if (!c) return BFQ_E_ARG;
    try {
        HIP_CHECK(hipSetDevice(c->device));
        c->err.clear();
        c->call = CallState{};
        body();
        return BFQ_OK;
    } catch (const BfqError &e) {
        c->err = e.msg;
        c->call = CallState{};
        (void)hipStreamSynchronize(c->stream);
        if (c->copyStream) (void)hipStreamSynchronize(c->copyStream);   // copies into the caller's buffers have landed or failed
        (void)hipGetLastError();
        c->recs.clear(); c->evUsed = 0;
        return e.code;
    } catch (const std::bad_alloc &) {
        c->err = "host out of memory";
        c->call = CallState{};
        return BFQ_E_NOMEM;
    }
}

static inline u64 ceil_div(u64 a, u64 b) { return (a + b - 1) / b; }
// HIP caps gridDim.x * blockDim.x below 2^32: every kernel is launched on at most
// BFQ_MAX_GRID workgroups and strides over its work items.
#define BFQ_MAX_GRID (1u << 19)
static inline unsigned bfq_grid(u64 items, u64 perBlock)
{
    u64 b = ceil_div(items, perBlock);
    return (unsigned)(b < 1 ? 1 : (b > BFQ_MAX_GRID ? BFQ_MAX_GRID : b));
}

// the suffix records being sorted: three 32-bit arrays (layout: bfq_common.h)
struct SortRec { u32 *w0; u64 *w12; };   // w12 = w2 << 32 | w1
struct KeySrc { const u8 *T8, *Q8; const u64 *text3; };   // what the records of the unsorted rows are a function of: byte text, its qualities, packed text

// ---- stage entry points (each in its own .hip file) --------------------------------
// scan: out[i] = sum(in[0..i)) ; T in {u8,u32,u64}; total (device u64) optional
void bfq_exscan_u8(bfq_ctx *c, const u8 *in, u64 *out, u64 n, u64 *d_total);
void bfq_exscan_u32(bfq_ctx *c, const u32 *in, u64 *out, u64 n, u64 *d_total);
void bfq_exscan_u64(bfq_ctx *c, const u64 *in, u64 *out, u64 n, u64 *d_total);

u64 *bfq_line_index(bfq_ctx *c, const u8 *d_buf, u64 len, u64 *nlines);   // k_fastq.hip: positions of the line ends (arena)
// bfq_deflate.hip: the BGZF form of a text that lies on the device (d_text) or on the host (h_src) to dst; held: the arena is
// the caller's, sized with bfq_deflate_need() beside what it holds.  Returns the length of the output.
size_t bfq_deflate_need(bfq_ctx *c, u64 len, bool hostSrc, size_t beside);
u64 bfq_deflate_core(bfq_ctx *c, const u8 *d_text, HostRef h_src, u64 len, int level, HostRef dst, bool held, size_t beside);
u64 bfq_fastq_count_lines(bfq_ctx *c, const u8 *d_buf, u64 len);          // k_fastq.hip: newlines + 1
// stream codec (k_codec.hip)
u64 bfq_codec_bound(u64 n);
u64 bfq_codec_workspace(u64 n);
u64 bfq_codec_raw_len(const u8 *h_in, u64 len, u64 *nameWs = nullptr);   // all members of a file
u64 bfq_codec_member_len(const u8 *h_in, u64 len);                 // bytes of the first member
u64 bfq_codec_compress_device(bfq_ctx *c, const u8 *d_in, u64 n, u8 *d_out, u64 cap);
u64 bfq_codec_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap);
u64 bfq_codec_checksum_device(bfq_ctx *c, const u8 *d_in, u64 n, u64 *d_tmp);
u64 bfq_rans_compress_device(bfq_ctx *c, const u8 *d_in, u64 n, u8 *d_out, u64 cap, bool dry);
u64 bfq_rans_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap);
// DNA container (k_dnac.hip)
u64 bfq_dnac_workspace(u64 n);
u64 bfq_dnac_compress_device(bfq_ctx *c, const u8 *d_in, u64 n, u8 *d_out, u64 cap, u64 *nbases);
u64 bfq_dnac_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap);
u64 bfq_dnac_member_len(const u8 *h_in, u64 len);
// tokenised read names (k_names.hip): the BFQNAME1 container.  The encoder is sized first (bfq_names_size: line index, the
// lines' shares of the three streams, eligibility), so that a caller that owns the reservation can grow the arena by
// bfq_names_rest_bytes() before bfq_names_finish() writes, codes and chooses (flags as bfq_names_compress).
struct NamesSized { bool eligible = false; u64 nl = 0; const u64 *lineEnd = nullptr; u64 *offO = nullptr, *offN = nullptr, *offT = nullptr; u64 total[3] = {0, 0, 0}; };
bool bfq_names_size(bfq_ctx *c, const u8 *d_in, u64 n, NamesSized *S);
u64 bfq_names_sized_bytes(u64 n, u64 nl);
u64 bfq_names_rest_bytes(u64 n, const NamesSized &S);
u64 bfq_names_finish(bfq_ctx *c, const u8 *d_in, u64 n, const NamesSized &S, u32 flags, u8 *d_out, u64 cap);
u64 bfq_names_member_len(const u8 *h_in, u64 len);
u64 bfq_names_decode_extra(const u8 *h_in, u64 len, u64 *maxInner);   // arena bytes beside the codec's workspace for the largest inner member
u64 bfq_names_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap);
// quality lines by their place in the read (k_quals.hip): the BFQQUAL1 container.  bfq_quals_finish: what bfq_quals_compress
// gives for a stream on the device (flags as there); bfq_quals_workspace: arena bytes beside the general codec's.
u64 bfq_quals_workspace(u64 n, u64 nl);
u64 bfq_quals_finish(bfq_ctx *c, const u8 *d_in, u64 n, u32 flags, u8 *d_out, u64 cap);
u64 bfq_quals_member_len(const u8 *h_in, u64 len);
u64 bfq_quals_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap);
void bfq_codec_normalise(const u32 *cnt, u32 A, u16 *f);           // k_codec.hip: a row of counts -> frequencies that sum to 2^12
u32 bfq_codec_bit_cost(u32 f);                                     // (12 - log2 f) * 256

// step 1 pieces
void bfq_build_text(bfq_ctx *c, const u8 *d_bases, const u8 *d_quals, const u64 *d_roff, u64 N, u64 n,
                    u8 *T8, u8 *Q8, u64 *text3, u64 nwords);
// rows per radix workgroup (k_radix.hip); k_build_keys works on the same blocks to leave the first pass's digit counts
#define BFQ_RS_BLOCK_ELEMS 98304                        // rows per radix block (and per text block of the pile counts) for large inputs
#define BFQ_RS_TILE 3072                                // rows per scatter tile
// rows per radix block of an n-row sort: a workgroup runs through its block tile by tile, so small inputs get smaller
// blocks -- at least ~4 rounds of workgroups over the device instead of one round and a tail (1 M x 100 bp: 1028 blocks of
// 98 304 rows on 1024 workgroup slots took two rounds)
static inline u64 bfq_radix_block_elems(u64 n)
{
    u64 tpb = BFQ_RS_BLOCK_ELEMS / BFQ_RS_TILE;
    while (tpb > 1 && n / (BFQ_RS_TILE * tpb) < 4096) tpb >>= 1;   // more, smaller blocks change nothing measurable (30 M x 150: 32, 8 or 4 tiles per block alike)
    return BFQ_RS_TILE * tpb;
}
void bfq_build_keys(bfq_ctx *c, const u8 *T8, const u8 *Q8, const u64 *text3, u64 n, SortRec out, u32 *hist0);   // hist0: [256][ceil(n / bfq_radix_block_elems(n))]
// LSD radix sort of the records on their 48-bit key; result ends in A
void bfq_count_keys(bfq_ctx *c, const u64 *text3, u64 n, u32 *hist0);   // hist0 alone, no records: for a sort whose first pass generates them
SortRec bfq_radix_sort(bfq_ctx *c, SortRec in, SortRec tmp, u64 n, int passes = BFQ_KEY_PASSES, const u32 *hist0 = nullptr, const KeySrc *gen = nullptr);   // returns the buffer holding the result (in: even passes, tmp: odd); fewer passes = low digits only; hist0: pass-0 counts already made; gen: pass 0 makes the records of rows = text positions itself and does not read `in`
// tie refinement: sorts vals inside equal-key segments by the remaining suffix, fills lcp
void bfq_refine(bfq_ctx *c, SortRec rec, const u64 *text3, u64 n, u16 *lcp, bfq_stats *st);
// segments above BFQ_HUGE_SEG rows (listed by k_refine_big): whole-device radix rounds on the following symbols
#define BFQ_HUGE_SEG 2048
void bfq_refine_huge(bfq_ctx *c, SortRec rec, const u64 *text3, u64 n, u16 *lcp, const u64 *hugeStart, const u64 *hugeLen);
void bfq_refine_bitonic(bfq_ctx *c, SortRec rec, const u64 *text3, u64 n, u16 *lcp, const u64 *d_start, const u64 *d_len, u64 count);   // k_refine.hip
void bfq_emit_bwt(bfq_ctx *c, SortRec rec, u64 n, int termOut, u8 *bwt, u8 *qs, u32 *gcnt);   // gcnt: [6][n/256+1] symbol counts
// whole step 1 on device-resident reads; leaves c->d_bwt/d_qual/d_lcp
void bfq_step1_device(bfq_ctx *c, const u8 *d_bases, const u8 *d_quals, const u64 *d_roff, u64 N, u64 total,
                      int termOut, bfq_stats *st);
// the same, one first-symbol pile at a time (k_piles.hip); workspace bound for pile records of at most `cap` rows
struct PileText { u8 *T8, *Q8; u64 *text3; };
void bfq_step1_piles(bfq_ctx *c, const u8 *d_bases, const u8 *d_quals, const u64 *d_roff, u64 N, u64 total, int termOut, bfq_stats *st,
                     const PileText *pre = nullptr, u64 capTarget = 0);
size_t bfq_ws_need_piles(u64 n, u64 N, u64 cap, u64 extra, bool lean = false);
// one pile on its own (global mode): pile-local eBWT / QS / LCP + the sorted records' (w1, w2) words, all in the arena
struct PileRows { u64 m; u8 *bwt, *qs; u16 *lcp; const u64 *w12; };
u64 bfq_run_one_pile(bfq_ctx *c, const u8 *T8, const u8 *Q8, const u64 *text3, u64 n, u32 s, u32 s2, int termOut, PileRows *out);
void bfq_pile_pair_counts(bfq_ctx *c, const u8 *T8, u64 n, u64 *counts36);
void bfq_pack_text(bfq_ctx *c, const u8 *T8, u64 n, u64 *text3, u64 nwords);

// steps 2-4 pieces
RankIndex bfq_rank_build(bfq_ctx *c, const u8 *bwt, const u8 *qs, u64 n, int term, const u32 *gcnt = nullptr);
u64 *bfq_symbol_scans(bfq_ctx *c, const u8 *bwt, u64 n, int term, const u32 *gcntIn, u32 *gcntOut);   // k_rank.hip
void bfq_rank_blocks(bfq_ctx *c, const u8 *bwt, u64 n, int term, const u64 *scanned, u64 *rank);          // k_bfs.hip
void bfq_lcp_flags(bfq_ctx *c, const u16 *lcp, u64 n, int K, u8 *in);
// LCP array from the eBWT alone (k_bfs.hip): lcp has n + 1 entries
void bfq_lcp_from_bwt(bfq_ctx *c, const u8 *bwt, u64 n, u64 N, int term, u16 *lcp, u32 *gcntOut = nullptr,   // gcntOut: [6][n/256+1] symbol counts, kept
                      const u64 *rankGiven = nullptr, u64 ringEntries = 0);
// pm != nullptr: position mode -- no LF table (R.lfq may be null): edits go to the output line streams at the text position
// each row's sort record carries (k_cluster.hip)
// outSym == nullptr: the edits stay row-local instead -- the smoothed quality replaces editQual[row] (unbinned), a replaced
// base goes to repl[row] -- and the position bins carry every row to its text position afterwards (k_posbin.hip)
struct ClusterPos { const u64 *w12; const u64 *text3; u8 *outSym, *outQual; int B; u8 *editQual = nullptr, *repl = nullptr; };
// rm != nullptr: rank mode -- no LF table either: LF from the rank blocks, qualities edited in place (qual == the array the
// statistics are read from), replaced bases into repl[] (k_compact.hip)
struct ClusterRank { const u64 *rankBlk; u64 F[6]; u8 *qual, *repl; };
void bfq_clusters(bfq_ctx *c, const RankIndex &R, const u8 *bwt, const u8 *qual, const u8 *in, u64 n, const ClusterPos *pm = nullptr,
                  const ClusterRank *rm = nullptr);
// steps 2-4 on a given eBWT without the LF table (k_compact.hip): rank blocks + qualities in place + replacement array
#define BFQ_COMPACT_LCP_WIN (256ull << 20)                // rows of the LCP file in flight (one upload by all staging workers)
size_t bfq_ws_need_compact(bfq_ctx *c, u64 n, u64 N, u64 extra, bool haveLcp, size_t resident);   // resident: the caller's eBWT + qualities
void bfq_steps234_compact(bfq_ctx *c, const u8 *bwt, u8 *qual, HostRef lcp, int lcp_bytes, u64 n, u64 N, u64 *d_roff, u32 *lens,
                          u8 **ob, u8 **oq, u64 extra, size_t resident);
// LF walks: lengths only, then emission at given offsets
void bfq_invert_count(bfq_ctx *c, const RankIndex &R, u64 N, u32 *lens);
void bfq_fixed_offsets(bfq_ctx *c, u64 N, u64 L, u64 *d_roff);   // d_roff[i] = i * L, i <= N
// reads [first, first + count) (count ~0: all from first); lines: outputs are line streams (read i at roff[i] + i, then '\n')
void bfq_invert(bfq_ctx *c, const RankIndex &R, u64 N, const u64 *d_roff, int B, u8 *out_bases, u8 *out_quals, u64 first = 0,
                u64 count = ~0ull, bool lines = false);
bool bfq_is_pinned(const void *p);
// the rows back in text order by position bins instead of LF walks (k_posbin.hip): w12 = the sorted records' (w1, w2) words
// (overwritten), repl / editQual = k_cluster's row-local edits; the reads go out back to back (read i at roff[i])
size_t bfq_posbins_need(u64 n);                   // arena bytes it takes; ~0: more rows than two partition levels hold
void bfq_posbins(bfq_ctx *c, u64 *w12, const u8 *repl, const u8 *editQual, u64 n, const u64 *d_roff, u64 N, int B, const u8 *inSym, const u8 *inQual,
                 u8 *outSym, u8 *outQual);

void bfq_synth_launch(bfq_ctx *c, const bfq_synth *s, u8 *d_bases, u8 *d_quals, u64 *d_roff);
u8 *bfq_synth_headers(bfq_ctx *c, const bfq_synth *s, u64 *len);   // k_synth.hip

// FASTQ text on the device (k_fastq.hip)
struct FqRec { u64 hdrStart, seqStart, qualStart; u32 hdrLen, len; };   // one record: where its lines start (len: CR dropped)
struct DevFastq { u64 N, total; void *rec; u64 *roff; u8 *bases, *quals; u64 *lineEnd; };
void bfq_fastq_index(bfq_ctx *c, const u8 *d_fastq, u64 len, DevFastq *fq);   // lines, records, read offsets, the checks: no gather (bases / quals nullptr)
void bfq_fastq_parse(bfq_ctx *c, const u8 *d_fastq, u64 len, DevFastq *fq);   // ... and lines 2 and 4 gathered back to back
u64 bfq_fastq_format(bfq_ctx *c, const u8 *d_bases, const u8 *d_quals, const u64 *d_roff, u64 N, int mode, const u8 *d_hdr,
                     u64 hdrLen, const DevFastq *fq, u8 **d_out, u64 **recOffOut = nullptr, bool lines = false);
void bfq_fastq_hdr_stream(bfq_ctx *c, u64 N, const u8 *d_fastq, const DevFastq *fq, u8 **d_hdr, u64 *hdrLen, u64 **hOffOut = nullptr);
// records from two line streams and an index made elsewhere (bfq_restore.hip): k_fq_format with lines = 1; d_hdr == nullptr: "@"
void bfq_fastq_format_lines(bfq_ctx *c, const u8 *d_dna, const u8 *d_qs, const u64 *d_roff, const u8 *d_hdr, const u64 *hStart,
                            const u32 *hLen, const u64 *recOff, u64 N, u64 outLen, u8 *d_out);
// ... record i of the text being read inv[i] of the streams (bfq_fastq_restore_ordered): k_fq_format_ordered
void bfq_fastq_format_ordered(bfq_ctx *c, const u8 *d_dna, const u8 *d_qs, const u64 *d_roff, const u8 *d_hdr, const u64 *hStart,
                              const u32 *hLen, const u64 *recOff, const u64 *inv, u64 N, u64 outLen, u8 *d_out);
void bfq_restore_sizes_ordered(bfq_ctx *c, const u32 *sizes, const u64 *inv, u64 N, u32 *sizesOut);   // sizesOut[i] = sizes[inv[i]]
void bfq_fastq_part_index(bfq_ctx *c, const DevFastq *fq, const u64 *h_pstart, int nparts, u64 *d_idx);
void bfq_pick_u64(bfq_ctx *c, const u64 *d_src, const u64 *d_idx, int count, u64 addIdx, u64 *d_out);

// eBWT-domain containers (bfq_api.hip): the body of bfq_stream_ebwt_decode.  Both line streams (n bytes each) stay in the
// arena and are returned in *res when res != nullptr; the arena is reserved here, once, with extraWs bytes for the caller's
// own use after the walk (the LF table's space is handed back to the caller as well).  h_dna / h_qs may be nullptr.
// CallState::arenaHeld: no reservation -- the arena is the caller's, who sized it with bfq_ebwt_decode_need() for the same
// extraWs; the walk's buffers go above the current top.
struct EbwtLines { u8 *dna = nullptr, *qs = nullptr; u64 n = 0, N = 0; };
size_t bfq_ebwt_decode_need(const u8 *h_bwtz, u64 len_b, u64 len_q, size_t extraWs, bool keepLines);   // what bfq_ebwt_decode_lines reserves (header fields as they stand)
void bfq_ebwt_decode_lines(bfq_ctx *c, const u8 *h_bwtz, u64 len_b, const u8 *h_qsz, u64 len_q, u8 *h_dna, u8 *h_qs, u64 cap,
                           uint64_t *stream_len, uint64_t *n_reads, size_t extraWs, EbwtLines *res);

// records in another order (k_reorder.hip; bfq_reorder.hip drives them).  A text of the call: its bytes, its record index,
// its length.  The sort records carry the 40-bit key where bfq_radix_sort() reads its digits (w0 = key >> 8, bits 24..31 of
// w1 = key & 255) and the read index in the 56 bits that are left.
struct RoText { const u8 *buf; const FqRec *rec; u64 len; };
void bfq_reorder_keys(bfq_ctx *c, const RoText *mates, int nmates, u64 N, int mode, int k, u64 seed, SortRec out);
void bfq_reorder_perm(bfq_ctx *c, SortRec sorted, const RoText *mates, int nmates, u64 N, u64 *perm, u64 *const *sizes);
void bfq_reorder_gather(bfq_ctx *c, const RoText &t, const u64 *perm, const u64 *newOff, u64 N, u8 *d_out);
// the way back: the permutation as a BFQPERM1 payload (bfq_perm.h) and its inverse (k_reorder.hip)
void bfq_perm_pack(bfq_ctx *c, const u64 *perm, u64 N, u64 *d_words);                            // d_words: bfq_perm_words() of them
u64 bfq_perm_unpack_invert(bfq_ctx *c, const u64 *d_words, u64 N, u64 *perm, u64 *inv);         // the first offending position, ~0: none; synchronises
void bfq_reorder_sizes(bfq_ctx *c, const u64 *order, const RoText *mates, int nmates, u64 N, u64 *const *sizes);   // sizes[p][j] = size of record order[j]

// interleaved paired FASTQ (k_pairs.hip; bfq_pairs.hip drives them; the definition: bfq_pairs.h).  A text of the call: its bytes,
// its record index, its length (with its final LF) and its records.
struct PrText { const u8 *buf; const FqRec *rec; u64 len, N; };
void bfq_pairs_compare(bfq_ctx *c, const PrText &a, const PrText *b, u64 P, u32 suffix, u64 *d_firstBad);   // *d_firstBad preset to all-ones
void bfq_pairs_run_starts(bfq_ctx *c, const PrText &a, u32 suffix, u64 *start);
void bfq_pairs_roles(bfq_ctx *c, const PrText &a, const u64 *start, u8 *role, u64 *const sz[3], u64 *d_cnt);   // d_cnt[0, 2) zeroed: singles, pairs
void bfq_pairs_pair_sizes(bfq_ctx *c, const PrText &a, u64 P, u64 *sz);
void bfq_pairs_split(bfq_ctx *c, const PrText &a, const u64 *off1, u8 *o1, u8 *o2);
void bfq_pairs_split_roles(bfq_ctx *c, const PrText &a, const u8 *role, const u64 *const off[3], u8 *const o[3]);
void bfq_pairs_merge(bfq_ctx *c, const PrText &a, const PrText &b, u8 *out);
// ... the repair (k_pairs.hip, its last section).  t[3]: the texts of the call, N: their records, numbered 1, 2, 0.
void bfq_repair_sort(bfq_ctx *c, const PrText t[3], u64 N, const bfq_repair_opts &O, u64 *h, u8 *hint, SortRec a, SortRec b, u64 *sg, u64 *sh, u64 *start,
                     u64 *d_stat);   // d_stat[0, 2): the longest run, the smallest global number in a run that is too long (~0: none)
void bfq_repair_group(bfq_ctx *c, const PrText t[3], u64 N, u32 suffix, const u64 *start, const u64 *sg, const u64 *sh, u8 *role, u64 *anchor, u8 *f1, u8 *f0,
                      u64 *d_cnt);   // d_cnt[0, 2) zeroed: dup_groups, mixed_runs
void bfq_repair_place(bfq_ctx *c, const PrText t[3], u64 N, const u8 *role, const u64 *anchor, const u64 *rank1, const u64 *rank0, u64 *slot, u64 *const sz[3]);
void bfq_repair_move(bfq_ctx *c, const PrText t[3], u64 N, const u8 *role, const u64 *slot, const u64 *const off[3], u8 *const o[3]);
void bfq_maxscan_u64(bfq_ctx *c, const u64 *in, u64 *out, u64 n);   // out[i] = max(in[0..i]); in == out is allowed
// the texts of a call staged and indexed (bfq_pairs.hip)
BFQ_LOCAL void bfq_pairs_stage(bfq_ctx *c, const TextIn src[3], const std::function<void(const u8 *, u64, u32)> &gzip, const char *what, size_t perRec,
                               bool arenaOut, PrText t[3]);
// exact duplicate removal (k_dedup.hip; bfq_dedup.hip drives them; the definition: bfq_dedup.h).  T: the one or two texts of
// the call (nt), N: their units.
struct DdTexts { PrText t[2]; u32 nt; };
struct DdGroups { u64 *sg, *sh, *start, *head, *next, *rep; u8 *mixed; };   // per sorted position (head, next, mixed: read at run starts)
void bfq_dedup_sort(bfq_ctx *c, const DdTexts &T, u64 N, const bfq_dedup_opts &O, u64 *h, u64 *score, SortRec a, SortRec b, const DdGroups &G, u64 *d_stat);
// d_stat, in u64: the longest run, mixed runs, the round's unresolved, kept, the largest group, its first, levels
enum { DD_S_MAXRUN = 0, DD_S_MIXED, DD_S_UNRES, DD_S_KEPT, DD_S_MAXGROUP, DD_S_FIRST, DD_S_LGROUPS, DD_S_LUNITS = DD_S_LGROUPS + 32, DD_S_NUM = DD_S_LUNITS + 32 };
u64 bfq_dedup_round(bfq_ctx *c, const DdTexts &T, u64 N, const DdGroups &G, u64 *d_stat, bool first);   // one round; returns the unresolved positions; synchronises
void bfq_dedup_first_bad(bfq_ctx *c, u64 N, const DdGroups &G, u64 *d_firstBad);           // *d_firstBad preset to all-ones
void bfq_dedup_winners(bfq_ctx *c, u64 N, u32 keep, const DdGroups &G, const u64 *score, u64 *gsize, u64 *best, u64 *win, u8 *kept, u64 *d_stat);
void bfq_dedup_sizes(bfq_ctx *c, const DdTexts &T, u64 N, const u8 *kept, u64 *const sz[2]);
void bfq_dedup_move(bfq_ctx *c, const DdTexts &T, u64 N, const u8 *kept, const u64 *const off[2], u8 *const out[2], u8 *const dup[2]);

// two FASTQ texts compared where they lie (k_compare.hip; bfq_compare.hip drives them).  inv == nullptr: read i of A pairs with
// read i of B, else with read inv[i].  d_rep: a zeroed report on the device whose first_changed_read is all-ones.
struct CmpText { const u8 *buf; const FqRec *rec; };
void bfq_compare_check(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, bfq_compare_report *d_rep, u64 *d_badRead);   // *d_badRead preset to all-ones
void bfq_compare_pass(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, u64 total, bfq_compare_report *d_rep, u32 *readDiffs);
void bfq_compare_emit(bfq_ctx *c, CmpText A, CmpText B, const u64 *inv, u64 N, u64 total, const u32 *readDiffs, const u64 *diffOff, u64 cap,
                      bfq_compare_diff *d_out);

// the k-mer spectrum of one or two FASTQ texts (k_kmers.hip; bfq_kmers.hip drives them; the constants: bfq_kmers.h).  A text of
// the call: its bytes, its record index, its records.  bases: the text's sequence bytes (for the profile's byte counts).
struct KmText { const u8 *buf; const FqRec *rec; u64 N; };
void bfq_kmers_hist(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u64 bases, u64 *d_hist, u64 *d_scal);   // d_hist[4096] and d_scal[3] (short reads, valid, skipped) are added to
void bfq_kmers_count(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u32 binLo, u32 binHi, u64 bases, u32 *cnt);
void bfq_kmers_emit(bfq_ctx *c, const KmText &T, u32 k, u32 canonical, u32 binLo, u32 binHi, u32 src, u64 bases, u64 records, const u64 *off, SortRec out);
SortRec bfq_kmers_sort(bfq_ctx *c, SortRec a, SortRec b, u64 n, u32 k);   // the records start in a; returns the buffer that holds the result
size_t bfq_kmers_seg_bytes(u64 n);                                        // arena bytes of bfq_kmers_runs
void bfq_kmers_runs(bfq_ctx *c, SortRec S, u64 n, u32 k, u32 solid, u64 *heads, struct bfq_kmer_report *d_rep, struct bfq_kmer_entry *d_list, u64 capList);

// a run's base edits as the container BFQEDIT1 (k_edits.hip; bfq_edits.hip drives them; layout: bfq_edits.h).  One side of a
// make, or the target of an apply: where read r's bases lie -- rec != nullptr: at buf + rec[r].seqStart (a FASTQ text and its
// record index), else at buf + roff[r] (+ r when `lines`: a line stream).  roff: N + 1 entries, the g of every read's first base.
struct EdSide { const u8 *buf; const FqRec *rec; u32 lines; };
void bfq_edit_check(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 rBase, u64 n, u64 *d_badRead, u64 *d_shape);   // *d_badRead preset to all-ones, *d_shape to 0
void bfq_edit_count(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 total, u32 *cnt, u64 *d_sums);           // d_sums[0] += reads touched
void bfq_edit_write(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 E, u32 *cnt, const u64 *off, u64 *pos, u8 *byte, u64 *d_sums);   // d_sums[1] += target_sum
void bfq_edit_segw(bfq_ctx *c, const u64 *pos, const u8 *byte, u64 E, u64 *first, u8 *wt, u64 *words, u64 *d_badEdit);
void bfq_edit_pack(bfq_ctx *c, const u64 *pos, u64 E, const u8 *wt, const u64 *wordOff, u64 *gaps);
void bfq_edit_unpack(bfq_ctx *c, const u64 *first, const u8 *wt, const u64 *gaps, const u64 *wordOff, u64 E, u64 *pos, u64 *d_badEdit);
void bfq_edit_locate(bfq_ctx *c, const u64 *pos, const u8 *byte, u64 E, u64 T, u64 gBase, EdSide X, const u64 *roff, u64 N, u64 *addr, u64 *d_badEdit,
                     u64 *d_sums);
void bfq_edit_apply(bfq_ctx *c, const u64 *addr, const u8 *byte, u64 E, u8 *buf);
// bfq_edits.hip.  The arena is the caller's: what they allocate stays above the current top.
//   bfq_edits_make : the member of the edits between A ("before") and B ("after") at *d_member, its length returned.  cap: the
//                    room the caller has for it; a member that does not fit is not made: *d_member = nullptr and the return
//                    is a size that suffices (exact when at least its bytes fit).  Sides that are texts are held against each
//                    other read by read first (BFQ_E_ARG naming the first read whose length differs).
//   bfq_edits_apply: every member of [h_edits, h_edits + len) unpacked and held against the target (N reads, roff, `total`
//                    bases); only then are the bytes written to d_buf.  Any refusal: BFQ_E_ARG, nothing written.
size_t bfq_edits_make_need(u64 N, u64 total, u64 cap);
u64 bfq_edits_make(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 total, u64 cap, u8 **d_member, bfq_edit_stats *st);
size_t bfq_edits_apply_need(const u8 *h_edits, u64 len);           // throws BFQ_E_ARG when the bytes are no members
void bfq_edits_apply(bfq_ctx *c, const u8 *h_edits, u64 len, u8 *d_buf, EdSide X, const u64 *roff, u64 N, u64 total, bfq_edit_stats *st);
