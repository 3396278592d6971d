// bfq_gzip.hip -- plain gzip input (include/bfqzip_hip.h, bfq_gzip_*): the host side of the side-by-side inflate.  The format,
// the algorithm and every bound are bfq_gzip.h's; the kernels are k_gzip.hip's.  One call is two trips to the device:
//   1  compressed bytes up; candidate search and pass 1; candidates and decoder records down; the chain (bfq_gzip_plan)
//   2  the chain's jobs up; pass 2, windows, resolve, CRC32; the far-distance word, the member ends and their CRC32 down
//   arena   the compressed bytes, 8 + 48 bytes per piece, then 2 x raw of symbols, 32 KiB and 48 bytes per chain decoder,
//           28 bytes per member and -- unless the caller brings a device buffer -- the text.  The second part is known only
//           after the first: when the arena has to grow for it, the compressed bytes and the candidates are uploaded again.
// bfq_gzip_inflate_host is the host form of bfq_gzip.h, for tests and as the statement of the algorithm: no entry point here
// falls back to it.
#include <string.h>
#include <stdio.h>
#include <sys/mman.h>
#include "bfq_internal.h"
#include "bfq_gzip.h"

void bfq_gzip_launch_pass1(bfq_ctx *c, const u8 *d_in, u64 len, u64 chunk, u64 np, u64 *d_cand, bfq_gzip_rec *d_recs);   // k_gzip.hip
void bfq_gzip_launch_pass2(bfq_ctx *c, const u8 *d_in, u64 len, u64 chunk, u64 np, const u64 *d_cand, const bfq_gzip_job *d_jobs, u64 nj, u64 raw,
                           u16 *d_sym, bfq_gzip_end *d_ends, u8 *d_win, u8 *d_out, u64 *d_far);
void bfq_gzip_launch_crc(bfq_ctx *c, const u8 *d_text, u64 raw, const bfq_gzip_end *d_ends, u64 nEnds, u32 *d_crc);

static std::string gzip_message(const bfq_gzip_err &E)
{
    char b[256];
    snprintf(b, sizeof b, "damaged gzip input: member %llu at byte %llu: %s", E.member, E.off, bfq_gzip_reason(E.reason));
    return b;
}
static const char *const GZIP_SMALL = "output buffer too small for the inflated text";
// the piece size of a call: the caller's, else $BFQ_GZIP_CHUNK, else the default
static u64 gzip_chunk(u64 chunk)
{
    if (!chunk) {
        const char *e = getenv("BFQ_GZIP_CHUNK");
        chunk = e && *e ? strtoull(e, nullptr, 10) : BFQ_GZIP_DEF_CHUNK;
    }
    if (!bfq_gzip_chunk_ok(chunk)) throw BfqError{BFQ_E_ARG, "gzip chunk: a power of two of at least 512 bytes"};
    return chunk;
}

extern "C" int bfq_gzip_probe(const uint8_t *h, uint64_t len)
{
    u64 data = 0;
    return h && len && bfq_gzip_member_header(h, len, 0, &data) == BFQ_BGZF_OK ? 1 : 0;
}

static thread_local std::string g_gzipHostErr;
extern "C" const char *bfq_gzip_host_error(void) { return g_gzipHostErr.c_str(); }
extern "C" int bfq_gzip_inflate_host(const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                                     bfq_gzip_stats *stats)
{
    if (out_len) *out_len = 0;
    return host_guarded(g_gzipHostErr, [&] {
        if (!out_len || (!h_in && len) || (cap && !h_out)) throw BfqError{BFQ_E_ARG, "null argument"};
        chunk = gzip_chunk(chunk);
        static const u8 none = 0;
        bfq_gzip_stats S{};
        bfq_gzip_err E;
        u64 raw = 0;
        u8 dummy = 0;
        const int r = bfq_gzip_host(len ? h_in : &none, len, chunk, h_out ? h_out : &dummy, cap, false, &raw, &S, &E);
        if (stats) *stats = S;
        if (r == 3) throw BfqError{BFQ_E_NOMEM, "host out of memory"};
        if (r == 2) { *out_len = raw; throw BfqError{BFQ_E_ARG, GZIP_SMALL}; }
        if (r == 1) throw BfqError{BFQ_E_ARG, gzip_message(E)};
        *out_len = raw;
    });
}

// The text of h_in[0, len) at d_out (cap bytes; nullptr: in the arena), or steps 1-2 only (measure).  Returns the raw length
// and, through *where, the place of the text; *needed = the raw length when cap is below it.
static u64 gzip_core(bfq_ctx *c, const u8 *h_in, u64 len, u64 chunk, bool measure, u8 *d_out, u64 cap, u64 *needed, bfq_gzip_stats *stats, u8 **where)
{
    if (!h_in && len) throw BfqError{BFQ_E_ARG, "null argument"};
    chunk = gzip_chunk(chunk);
    const u64 np = bfq_gzip_pieces(len, chunk);
    bfq_phase("alloc");
    const size_t first = (size_t)len + 16 + (size_t)np * (sizeof(u64) + sizeof(bfq_gzip_rec)) + (1u << 20);
    c->reserve(first);
    u8 *d_in = c->alloc<u8>(len + 16);
    u64 *d_cand = c->alloc<u64>(np);
    bfq_gzip_rec *d_recs = c->alloc<bfq_gzip_rec>(np);
    bfq_phase("read_h2d");
    bfq_upload(c, d_in, h_in, len);
    bfq_phase("gpu");
    bfq_gzip_launch_pass1(c, d_in, len, chunk, np, d_cand, d_recs);
    std::vector<u64> cand(np);
    std::vector<bfq_gzip_rec> recs(np);
    HIP_CHECK(hipMemcpyAsync(cand.data(), d_cand, sizeof(u64) * np, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(recs.data(), d_recs, sizeof(bfq_gzip_rec) * np, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    std::vector<bfq_gzip_job> jobs;
    bfq_gzip_stats S{};
    bfq_gzip_err E;
    u64 raw = 0, nEnds = 0;
    bfq_gzip_plan(recs.data(), cand.data(), np, chunk, jobs, &S, &raw, &nEnds, &E);
    if (stats) *stats = S;
    if (measure) {
        c->profCollect();
        if (E.reason) throw BfqError{BFQ_E_ARG, gzip_message(E)};
        return raw;
    }
    if (!E.reason && raw > cap) {
        c->profCollect();
        *needed = raw;
        throw BfqError{BFQ_E_ARG, GZIP_SMALL};
    }
    // the second trip.  A chain that ended in an error is still decoded and resolved, into no text: a far distance in front
    // of the error lies lower in the stream and is the one to name.
    const u64 nj = jobs.size();
    const bool own = !d_out && !E.reason;
    const size_t second = 2 * ((size_t)raw + 8) + (size_t)nj * (BFQ_GZIP_WIN + sizeof(bfq_gzip_job)) + ((size_t)nEnds + 1) * (sizeof(bfq_gzip_end) + 4) +
                          (own ? (size_t)raw + 16 : 0) + (1u << 20);
    if (c->ws.room() < second) {
        bfq_phase("alloc");
        c->reserve(first + second);
        d_in = c->alloc<u8>(len + 16);
        d_cand = c->alloc<u64>(np);
        d_recs = c->alloc<bfq_gzip_rec>(np);
        bfq_phase("read_h2d");
        bfq_upload(c, d_in, h_in, len);
        bfq_upload(c, d_cand, cand.data(), sizeof(u64) * np);
        bfq_phase("gpu");
    }
    bfq_gzip_job *d_jobs = c->alloc<bfq_gzip_job>(nj);
    u16 *d_sym = c->alloc<u16>(raw + 8);
    bfq_gzip_end *d_ends = c->alloc<bfq_gzip_end>(nEnds + 1);
    u8 *d_win = c->alloc<u8>(nj * (u64)BFQ_GZIP_WIN);
    u32 *d_crc = c->alloc<u32>(nEnds + 1);
    u64 *d_far = c->alloc<u64>(1);
    if (own) d_out = c->alloc<u8>(raw + 16);
    bfq_upload(c, d_jobs, jobs.data(), sizeof(bfq_gzip_job) * nj);
    HIP_CHECK(hipMemsetAsync(d_far, 0xFF, 8, c->stream));
    HIP_CHECK(hipMemsetAsync(d_crc, 0, 4 * (nEnds + 1), c->stream));
    bfq_gzip_launch_pass2(c, d_in, len, chunk, np, d_cand, d_jobs, nj, raw, d_sym, d_ends, d_win, E.reason ? nullptr : d_out, d_far);
    if (!E.reason) bfq_gzip_launch_crc(c, d_out, raw, d_ends, nEnds, d_crc);
    u64 far = BFQ_GZIP_NONE;
    std::vector<bfq_gzip_end> ends(nEnds + 1);
    std::vector<u32> crc(nEnds + 1);
    HIP_CHECK(hipMemcpyAsync(&far, d_far, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(ends.data(), d_ends, sizeof(bfq_gzip_end) * nEnds, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(crc.data(), d_crc, 4 * nEnds, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    c->profCollect();
    if (far != BFQ_GZIP_NONE) {
        E.reason = BFQ_BGZF_E_DIST_FAR;
        bfq_gzip_locate(ends.data(), nEnds, far, &E.member, &E.off);
    } else if (!E.reason) bfq_gzip_check_members(ends.data(), nEnds, crc.data(), &E);
    if (E.reason) throw BfqError{BFQ_E_ARG, gzip_message(E)};
    *where = d_out;
    return raw;
}

extern "C" int bfq_gzip_measure(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint64_t *raw_len, uint64_t *n_members,
                                bfq_gzip_stats *stats)
{
    if (raw_len) *raw_len = 0;
    if (n_members) *n_members = 0;
    return guarded(c, [&] {
        bfq_gzip_stats S{};
        u64 needed = 0;
        u8 *where = nullptr;
        const u64 raw = gzip_core(c, h_in, len, chunk, true, nullptr, 0, &needed, &S, &where);
        if (stats) *stats = S;
        if (raw_len) *raw_len = raw;
        if (n_members) *n_members = S.members;
    });
}

extern "C" int bfq_gzip_inflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                                bfq_gzip_stats *stats)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || (cap && !h_out)) throw BfqError{BFQ_E_ARG, "null argument"};
        u8 *d_text = nullptr;
        u64 needed = 0;
        try {
            const u64 raw = gzip_core(c, h_in, len, chunk, false, nullptr, cap, &needed, stats, &d_text);
            bfq_phase("d2h_write");
            bfq_download(c, h_out, d_text, raw);
            c->sync();
            *out_len = raw;
        } catch (...) { *out_len = needed; throw; }
    });
}

extern "C" int bfq_gzip_inflate_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint64_t chunk, uint8_t *d_out, uint64_t cap, uint64_t *out_len,
                                       bfq_gzip_stats *stats)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || !d_out) throw BfqError{BFQ_E_ARG, "null argument"};
        u8 *d_text = nullptr;
        u64 needed = 0;
        try {
            *out_len = gzip_core(c, h_in, len, chunk, false, d_out, cap, &needed, stats, &d_text);
        } catch (...) { *out_len = needed; throw; }
    });
}

extern "C" int bfq_gzip_inflate_fd(bfq_ctx *c, int in_fd, uint64_t len, uint64_t chunk, int out_fd, uint64_t *out_len, bfq_gzip_stats *stats)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        if (in_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        // the decoders' records are walked between two uploads of the same bytes at most: the file is mapped
        MappedInput map;
        if (!map.open(in_fd, (size_t)len)) throw BfqError{BFQ_E_IO, std::string("cannot map the input file: ") + strerror(errno)};
        u8 *d_text = nullptr;
        u64 needed = 0;
        const u64 raw = gzip_core(c, map.data(), len, chunk, false, nullptr, ~0ull, &needed, stats, &d_text);
        if (out_fd >= 0) {
            bfq_phase("d2h_write");
            bfq_download(c, HostRef::file(out_fd, 0), d_text, raw);
            c->sync();
            bfq_fd_size(out_fd, raw, "cannot size the output file: ", true);
        }
        *out_len = raw;
    });
}
