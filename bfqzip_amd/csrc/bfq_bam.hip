// bfq_bam.hip -- BAM input (include/bfqzip_hip.h, bfq_bam_*): the host side of the conversion of BAM records to FASTQ text.
// The format, the algorithm and every bound are bfq_bam.h's; the kernels are k_bam.hip's.  One call:
//   1  the file's stream into the arena: BGZF inflated there (bfq_bgzf.hip), or a source that begins with "BAM\1" uploaded
//   2  the header, walked on the host from bytes copied back, a window at a time
//   3  candidates and the counting walk; the pieces' records down; the chain (bfq_bam_chain), a launch per repaired piece
//   4  the chain's jobs up -- the host's prefix sums over the pieces place the text --; the placing walk; the pairing check
//   arena   the compressed bytes and the stream, 168 bytes per piece, 8 bytes per record of outputs 1 and 2 for the pairing
//           check and -- unless the caller brings device buffers -- 4/3 of the stream for the texts; all reserved at once,
//           since growing the arena would lose the stream.  With tags asked for (bfq_bam_tag_opts): 24 bytes more per piece,
//           and 5/2 of the stream for the texts (bfq_bam.h derives the bound); a call without them reserves what it did
// bfq_bam_to_fastq_host is the host form of bfq_bam.h, for tests and as the statement of the algorithm: no entry point here
// falls back to it.
#include <string.h>
#include <stdio.h>
#include <sys/mman.h>
#include <functional>
#include "bfq_internal.h"
#include "bfq_bgzf.h"
#include "bfq_bam.h"

static_assert(sizeof(bfq_bam_piece) == 96 && sizeof(bfq_bam_job) == 64, "168 bytes per piece with its candidate");
static_assert(sizeof(bfq_bam_opts) == 32 && sizeof(bfq_bam_stats) == 120, "the C-ABI's structures");

u64 bfq_bgzf_inflate_arena(bfq_ctx *c, const u8 *h_in, u64 len, const std::function<size_t(u64)> &more, u8 **where);   // bfq_bgzf.hip
void bfq_bam_launch_walk(bfq_ctx *c, const u8 *d_s, u64 len, u64 hdrEnd, u64 piece, u64 np, u32 nref, const bfq_bam_opts &O, u64 only, u64 from,
                         bfq_bam_piece *d_recs, const bfq_bam_tagsel &G, bfq_bam_tagcnt *d_tagc);                           // k_bam.hip
void bfq_bam_launch_place(bfq_ctx *c, const u8 *d_s, u64 len, const bfq_bam_job *d_jobs, u64 nj, u32 nref, const bfq_bam_opts &O, const bfq_bam_outs &out, u64 bytes,
                          const bfq_bam_tagsel &G);
void bfq_bam_launch_pairs(bfq_ctx *c, const u8 *d_s, const u64 *d_a, const u64 *d_b, u64 n, u64 *d_firstBad);

static const char *const BAM_SMALL = "output buffer too small for the FASTQ text";
static void bam_refuse(const bfq_bam_err &E) { throw BfqError{E.reason == BFQ_BAM_E_TOO_LONG ? BFQ_E_TOO_LONG : BFQ_E_ARG, bfq_bam_message(E)}; }
static bfq_bam_opts bam_opts(const bfq_bam_opts *in)
{
    bfq_bam_opts O;
    const char *why = nullptr;
    if (!bfq_bam_resolve(in, &O, &why)) throw BfqError{BFQ_E_ARG, why};
    return O;
}
// the tag selection of a call (off without the extension) and where its counts go
static bfq_bam_tagsel bam_tags(const bfq_bam_opts *in, bfq_bam_tag_stats **stats)
{
    bfq_bam_tagsel G;
    const char *why = nullptr;
    if (!bfq_bam_tags_resolve(in, &G, stats, &why)) throw BfqError{BFQ_E_ARG, why};
    return G;
}
static bool is_gzip(const u8 *h, u64 len) { return len >= 2 && h[0] == 0x1F && h[1] == 0x8B; }
void bfq_bam_refuse(const bfq_bam_err &E) { bam_refuse(E); }                       // (declared in bfq_bam.h, for bfq_bam_patch.hip)
bfq_bam_opts bfq_bam_opts_of(const bfq_bam_opts *in) { return bam_opts(in); }

extern "C" void bfq_bam_default_opts(bfq_bam_opts *o)
{
    const char *why;
    if (o) { bfq_bam_resolve(nullptr, o, &why); o->piece = 0; }
}

extern "C" int bfq_bam_probe(const uint8_t *h, uint64_t len)
{
    if (!h || len < 4) return 0;
    if (!memcmp(h, "BAM\1", 4)) return 1;
    bfq_bgzf_hdr hd;
    if (bfq_bgzf_member_header(h, len, &hd) != BFQ_BGZF_OK || hd.isize < 4) return 0;
    std::vector<u8> text(hd.isize);
    std::vector<bfq_bgzf_tables> T(1);
    u32 crcTab[256];
    for (u32 i = 0; i < 256; i++) crcTab[i] = bfq_crc32_entry(i);
    if (bfq_bgzf_inflate_payload(h + hd.payOff, hd.payLen, text.data(), hd.isize, hd.crc, T.data(), crcTab, 0, 1) != BFQ_BGZF_OK) return 0;
    return !memcmp(text.data(), "BAM\1", 4) ? 1 : 0;
}

static thread_local std::string g_bamHostErr;
extern "C" const char *bfq_bam_host_error(void) { return g_bamHostErr.c_str(); }
void bfq_bam_host_error_set(const std::string &msg) { g_bamHostErr = msg; }
extern "C" int bfq_bam_to_fastq_host(const uint8_t *raw, uint64_t raw_len, const bfq_bam_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                                     uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats)
{
    if (out_len) out_len[0] = out_len[1] = out_len[2] = 0;
    if (n_reads) n_reads[0] = n_reads[1] = n_reads[2] = 0;
    return host_guarded(g_bamHostErr, [&] {
        if (!out_len || !n_reads || (!raw && raw_len) || (h_out && !cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const bfq_bam_opts O = bam_opts(opts);
        bfq_bam_tag_stats *tagStats = nullptr, TS{};
        const bfq_bam_tagsel G = bam_tags(opts, &tagStats);
        static const u8 none = 0;
        u8 *const no[3] = {nullptr, nullptr, nullptr};
        const u64 caps[3] = {h_out ? cap[0] : 0, h_out ? cap[1] : 0, h_out ? cap[2] : 0};
        bfq_bam_stats S{};
        bfq_bam_err E;
        u64 ol[3], nr[3];
        const int r = bfq_bam_host(raw_len ? raw : &none, raw_len, O, h_out ? h_out : no, caps, !h_out, ol, nr, &S, &E, &G, &TS);
        if (stats) *stats = S;
        if (tagStats) *tagStats = TS;
        if (r == 1) bam_refuse(E);
        for (int o = 0; o < 3; o++) { out_len[o] = ol[o]; n_reads[o] = nr[o]; }
        if (r == 2) throw BfqError{BFQ_E_ARG, BAM_SMALL};
    });
}

// Steps 1-3, shared by both directions (bfq_bam.h states what it leaves).
void bfq_bam_chain_device(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts &O, const std::function<size_t(u64)> &more, bfq_bam_stats *stats, bfq_bam_chain_dev *C,
                          const bfq_bam_tagsel *Gin)
{
    bfq_bam_tagsel G{};
    if (Gin) G = *Gin;
    if (!h_in && len) throw BfqError{BFQ_E_ARG, "null argument"};
    u8 *d_s = nullptr;
    u64 raw = len;
    if (is_gzip(h_in, len)) raw = bfq_bgzf_inflate_arena(c, h_in, len, more, &d_s);
    else {
        bfq_phase("alloc");
        c->reserve((size_t)len + 16 + more(len) + (1u << 20));
        d_s = c->alloc<u8>(len + 16);
        bfq_phase("read_h2d");
        bfq_upload(c, d_s, h_in, len);
        bfq_phase("gpu");
    }
    bfq_bam_stats &S = C->S;
    S = bfq_bam_stats{};
    bfq_bam_err E;
    u32 nref = 0;
    u64 hdrEnd = 0, bad = 0;
    const int hr = bfq_bam_header([&](u64 off, u64 n, u8 *dst) {
        HIP_CHECK(hipMemcpyAsync(dst, d_s + off, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        c->sync();
    }, raw, &nref, &hdrEnd, &bad);
    if (hr) { E.reason = hr; E.header = true; E.off = bad; bam_refuse(E); }
    S.n_ref = nref; S.header_bytes = hdrEnd;
    const u64 piece = O.piece, np = bfq_bam_pieces(raw, hdrEnd, piece);
    bfq_bam_piece *d_recs = c->alloc<bfq_bam_piece>(np);
    bfq_bam_tagcnt *d_tagc = G.on ? c->alloc<bfq_bam_tagcnt>(np) : nullptr;
    std::vector<bfq_bam_tagcnt> T(G.on ? np : 0);
    bfq_bam_launch_walk(c, d_s, raw, hdrEnd, piece, np, nref, O, BFQ_BAM_NONE, 0, d_recs, G, d_tagc);
    std::vector<bfq_bam_piece> &P = C->P;
    P.resize(np);
    HIP_CHECK(hipMemcpyAsync(P.data(), d_recs, sizeof(bfq_bam_piece) * np, hipMemcpyDeviceToHost, c->stream));
    if (G.on) HIP_CHECK(hipMemcpyAsync(T.data(), d_tagc, sizeof(bfq_bam_tagcnt) * np, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    bfq_bam_chain(P, hdrEnd, raw, piece, [&](u64 k, u64 start) {
        bfq_bam_piece w;
        bfq_bam_launch_walk(c, d_s, raw, hdrEnd, piece, np, nref, O, k, start, d_recs, G, d_tagc);
        HIP_CHECK(hipMemcpyAsync(&w, d_recs + k, sizeof w, hipMemcpyDeviceToHost, c->stream));
        if (G.on) HIP_CHECK(hipMemcpyAsync(&T[k], d_tagc + k, sizeof(bfq_bam_tagcnt), hipMemcpyDeviceToHost, c->stream));
        c->sync();
        return w;
    }, C->jobs, &S, &E);
    if (stats) *stats = S;
    if (E.reason) { c->profCollect(); bam_refuse(E); }
    if (G.on) C->T = bfq_bam_tag_totals(T, C->jobs, hdrEnd, piece);
    C->d_s = d_s; C->raw = raw; C->nref = nref; C->hdrEnd = hdrEnd;
}

enum BamMode { BAM_MEASURE, BAM_DEVICE, BAM_ARENA };
// The texts of h_in[0, len) at d_out[] (BAM_DEVICE) or in the arena (BAM_ARENA; *where), or steps 1-3 only (BAM_MEASURE).
// outLen / nReads: set once the chain stands, also when a capacity is then found short (*isShort).
static void bam_core(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts *opts, BamMode mode, u8 *const d_out[3], const u64 cap[3], u64 outLen[3],
                     u64 nReads[3], bfq_bam_stats *stats, u8 *where[3], bool *isShort)
{
    const bfq_bam_opts O = bam_opts(opts);
    bfq_bam_tag_stats *tagStats = nullptr;
    const bfq_bam_tagsel G = bam_tags(opts, &tagStats);
    if (tagStats) *tagStats = bfq_bam_tag_stats{};                  // (a refused call leaves them 0)
    const std::function<size_t(u64)> more = [&](u64 raw) {
        const size_t np = (size_t)(raw / O.piece + 2);
        return np * (sizeof(bfq_bam_piece) + sizeof(bfq_bam_job) + 8 + (G.on ? sizeof(bfq_bam_tagcnt) : 0)) + (O.paired_check ? (size_t)raw / 4 + 1024 : 0) +
               (mode == BAM_ARENA ? (size_t)(G.on ? BFQ_BAM_TEXT_BOUND_TAGS(raw) : BFQ_BAM_TEXT_BOUND(raw)) + 1024 : 0) + 8192;
    };
    bfq_bam_chain_dev C;
    bfq_bam_chain_device(c, h_in, len, O, more, stats, &C, &G);
    if (tagStats) *tagStats = C.T;
    u8 *const d_s = C.d_s;
    const u64 raw = C.raw, hdrEnd = C.hdrEnd, piece = O.piece;
    const u32 nref = C.nref;
    const std::vector<bfq_bam_piece> &P = C.P;
    const std::vector<bfq_bam_job> &jobs = C.jobs;
    const bfq_bam_stats &S = C.S;
    bfq_bam_err E;
    bfq_bam_totals(P, jobs, hdrEnd, piece, outLen);
    for (int o = 0; o < 3; o++) nReads[o] = S.written[o];
    if (mode == BAM_MEASURE) { c->profCollect(); return; }
    for (int o = 0; o < 3; o++)
        if (outLen[o] > cap[o]) { c->profCollect(); *isShort = true; throw BfqError{BFQ_E_ARG, BAM_SMALL}; }
    if (O.paired_check && !bfq_bam_pair_counts(S, &E)) { c->profCollect(); bam_refuse(E); }
    bfq_bam_outs W{};
    for (int o = 0; o < 3; o++) {
        W.text[o] = mode == BAM_ARENA ? c->alloc<u8>(outLen[o] + 16) : d_out[o];
        if (outLen[o] && !W.text[o]) throw BfqError{BFQ_E_ARG, "null argument"};
        if (O.paired_check && o) W.names[o] = c->alloc<u64>(S.written[o] + 1);
    }
    const u64 nj = jobs.size();
    bfq_bam_job *d_jobs = c->alloc<bfq_bam_job>(nj + 1);
    u64 *d_bad = c->alloc<u64>(1);
    bfq_upload(c, d_jobs, jobs.data(), sizeof(bfq_bam_job) * nj);
    bfq_bam_launch_place(c, d_s, raw, d_jobs, nj, nref, O, W, outLen[0] + outLen[1] + outLen[2], G);
    u64 firstBad = BFQ_BAM_NONE;
    if (O.paired_check) {
        HIP_CHECK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
        bfq_bam_launch_pairs(c, d_s, W.names[1], W.names[2], S.written[1], d_bad);
        HIP_CHECK(hipMemcpyAsync(&firstBad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    }
    c->sync();
    c->profCollect();
    if (firstBad != BFQ_BAM_NONE) { E.reason = BFQ_BAM_E_PAIR_NAME; E.rec = firstBad; bam_refuse(E); }
    for (int o = 0; o < 3; o++) where[o] = W.text[o];
}

// runs bam_core and leaves out_len / n_reads as the header states: the lengths on success and on a short capacity, else 0
template <class After> static int bam_call(bfq_ctx *c, const u8 *h_in, u64 len, const bfq_bam_opts *opts, BamMode mode, u8 *const d_out[3], const uint64_t capIn[3],
                                           uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats, After after)
{
    zero3(out_len); zero3(n_reads);
    return guarded(c, [&] {
        const u64 cap[3] = {capIn ? capIn[0] : 0, capIn ? capIn[1] : 0, capIn ? capIn[2] : 0};
        if (!out_len || !n_reads || (mode != BAM_MEASURE && !capIn) || (mode == BAM_DEVICE && !d_out)) throw BfqError{BFQ_E_ARG, "null argument"};
        u64 ol[3] = {0, 0, 0}, nr[3] = {0, 0, 0};
        u8 *where[3] = {nullptr, nullptr, nullptr};
        bool isShort = false;
        try {
            bam_core(c, h_in, len, opts, mode, d_out, cap, ol, nr, stats, where, &isShort);
            after(where, ol);
        } catch (...) {
            if (isShort) for (int o = 0; o < 3; o++) out_len[o] = ol[o];
            throw;
        }
        for (int o = 0; o < 3; o++) { out_len[o] = ol[o]; n_reads[o] = nr[o]; }
    });
}

extern "C" int bfq_bam_measure(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint64_t out_len[3], uint64_t n_reads[3],
                               bfq_bam_stats *stats)
{
    return bam_call(c, h_in, len, opts, BAM_MEASURE, nullptr, nullptr, out_len, n_reads, stats, [](u8 *const *, const u64 *) {});
}

extern "C" int bfq_bam_to_fastq(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint8_t *const h_out[3], const uint64_t cap[3],
                                uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats)
{
    return bam_call(c, h_in, len, opts, BAM_ARENA, nullptr, cap, out_len, n_reads, stats, [&](u8 *const *where, const u64 *ol) {
        bfq_phase("d2h_write");
        for (int o = 0; o < 3; o++) {
            if (!ol[o]) continue;
            if (!h_out || !h_out[o]) throw BfqError{BFQ_E_ARG, "null argument"};
            bfq_download(c, h_out[o], where[o], ol[o]);
        }
        c->sync();
    });
}

extern "C" int bfq_bam_to_fastq_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, const bfq_bam_opts *opts, uint8_t *const d_out[3], const uint64_t cap[3],
                                       uint64_t out_len[3], uint64_t n_reads[3], bfq_bam_stats *stats)
{
    return bam_call(c, h_in, len, opts, BAM_DEVICE, d_out, cap, out_len, n_reads, stats, [](u8 *const *, const u64 *) {});
}

extern "C" int bfq_bam_to_fastq_fd(bfq_ctx *c, int in_fd, uint64_t len, const bfq_bam_opts *opts, const int out_fd[3], uint64_t out_len[3],
                                   uint64_t n_reads[3], bfq_bam_stats *stats)
{
    // the BGZF directory is read from headers and trailers all over the file: the file is mapped, and uploaded from the mapping
    MappedInput map;
    if (in_fd < 0 || !map.open(in_fd, (size_t)len)) {
        zero3(out_len); zero3(n_reads);
        return guarded(c, [&] {
            if (in_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
            throw BfqError{BFQ_E_IO, std::string("cannot map the input file: ") + strerror(errno)};
        });
    }
    const uint64_t cap[3] = {~0ull, ~0ull, ~0ull};
    return bam_call(c, map.data(), len, opts, BAM_ARENA, nullptr, cap, out_len, n_reads, stats,
                    [&](u8 *const *where, const u64 *ol) {
        bfq_phase("d2h_write");
        for (int o = 0; o < 3; o++) {
            if (!out_fd || out_fd[o] < 0) continue;
            bfq_download(c, HostRef::file(out_fd[o], 0), where[o], ol[o]);
            c->sync();
            bfq_fd_size(out_fd[o], ol[o], "cannot size the output file: ", true);
        }
    });
}
