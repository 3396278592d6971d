// bfq_bgzf.hip -- bgzip-compressed input (include/bfqzip_hip.h, bfq_bgzf_*): the directory of a BGZF file on the host, the
// members inflated on the device (k_bgzf.hip).  The format and every bound are bfq_bgzf.h's.
//   arena   the compressed bytes, the directory (24 bytes per member), the status word, and -- unless the caller brings a
//           device buffer -- the text
// There is no host inflate: plain gzip (one member, no block structure) is refused by name.
#include <string.h>
#include <stdio.h>
#include <sys/mman.h>
#include <algorithm>
#include <functional>
#include "bfq_internal.h"
#include "bfq_bgzf.h"

static_assert(sizeof(bfq_bgzf_member) == 24, "the directory entry is 24 bytes");

void bfq_bgzf_launch(bfq_ctx *c, const u8 *d_in, const void *d_dir, u64 nm, u8 *d_out, u64 rawLen, u64 *d_status);   // k_bgzf.hip
void bfq_bgzf_newline(bfq_ctx *c, u8 *d_text, u64 len, u64 *d_flag);

static void bgzf_refuse(u64 member, u64 off, int reason)
{
    if (member == 0 && (reason == BFQ_BGZF_E_FLG || reason == BFQ_BGZF_E_NO_BC))
        throw BfqError{BFQ_E_ARG, "gzip input that is not BGZF: a plain gzip member has no blocks to inflate side by side; recompress it with bgzip"};
    char b[256];
    snprintf(b, sizeof b, "damaged BGZF input: member %llu at byte %llu: %s", (unsigned long long)member, (unsigned long long)off, bfq_bgzf_reason(reason));
    throw BfqError{BFQ_E_ARG, b};
}

extern "C" int bfq_bgzf_probe(const uint8_t *h, uint64_t len)
{
    bfq_bgzf_hdr hd;
    return h && bfq_bgzf_member_header(h, len, &hd) == BFQ_BGZF_OK ? 1 : 0;
}

extern "C" int bfq_bgzf_index(const uint8_t *h_in, uint64_t len, bfq_bgzf_member *m, uint64_t cap, uint64_t *n_members, uint64_t *raw_len,
                              uint64_t *bad_off)
{
    u64 n = 0, raw = 0, bad = 0;
    if (!h_in && len) return BFQ_E_ARG;
    const int r = bfq_bgzf_walk(h_in, len, m, m ? cap : 0, &n, &raw, &bad);
    if (n_members) *n_members = n;
    if (raw_len) *raw_len = raw;
    if (bad_off) *bad_off = bad;
    return r ? BFQ_E_ARG : BFQ_OK;
}

// The text of h_in[0, len) at d_out (cap bytes; nullptr: in the arena, behind the compressed bytes).  Returns the raw length
// and, through *where, the place of the text.
// `more`: bytes to reserve behind the text for the caller's own allocations, from the raw length.
static u64 bgzf_inflate_core(bfq_ctx *c, const u8 *h_in, u64 len, u8 *d_out, u64 cap, u8 **where, const std::function<size_t(u64)> *more = nullptr)
{
    if (!h_in && len) throw BfqError{BFQ_E_ARG, "null argument"};
    u64 n = 0, raw = 0, bad = 0;
    const int hr = bfq_bgzf_walk(h_in, len, nullptr, 0, &n, &raw, &bad);
    if (!len) bgzf_refuse(0, 0, BFQ_BGZF_E_SHORT);
    if (hr && n == 0) bgzf_refuse(0, bad, hr);
    if (raw > cap) {
        if (hr) bgzf_refuse(n, bad, hr);
        throw BfqError{BFQ_E_ARG, "output buffer too small for the inflated text"};
    }
    // a header that is refused ends the directory: the members before it are still inflated, so that the lowest failing
    // member is the one named
    std::vector<bfq_bgzf_member> dir(n);
    bfq_bgzf_walk(h_in, len, dir.data(), n, &n, &raw, &bad);
    const u64 used = hr ? bad : len;
    bfq_phase("alloc");
    c->reserve((size_t)used + 24 * (size_t)n + (d_out ? 0 : (size_t)raw) + (more ? (*more)(raw) : 0) + (1u << 20));
    u8 *d_in = c->alloc<u8>(used + 16);
    bfq_bgzf_member *d_dir = c->alloc<bfq_bgzf_member>(n + 1);
    u64 *d_status = c->alloc<u64>(1);
    if (!d_out) d_out = c->alloc<u8>(raw + 16);
    bfq_phase("read_h2d");
    bfq_upload(c, d_in, h_in, used);
    bfq_upload(c, d_dir, dir.data(), sizeof(bfq_bgzf_member) * n);
    bfq_phase("gpu");
    HIP_CHECK(hipMemsetAsync(d_status, 0xFF, 8, c->stream));
    bfq_bgzf_launch(c, d_in, d_dir, n, d_out, raw, d_status);
    u64 status = ~0ull;
    HIP_CHECK(hipMemcpyAsync(&status, d_status, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    c->profCollect();
    if (status != ~0ull) bgzf_refuse(status >> 8, dir[status >> 8].in_off, (int)(status & 0xFF));
    if (hr) bgzf_refuse(n, bad, hr);
    *where = d_out;
    return raw;
}

// bfq_bam.hip: the inflated stream of a BGZF file in the arena, with room for more(raw) bytes behind it
u64 bfq_bgzf_inflate_arena(bfq_ctx *c, const u8 *h_in, u64 len, const std::function<size_t(u64)> &more, u8 **where)
{
    return bgzf_inflate_core(c, h_in, len, nullptr, ~0ull, where, &more);
}

extern "C" int bfq_bgzf_inflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *h_out, uint64_t cap, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || (cap && !h_out)) throw BfqError{BFQ_E_ARG, "null argument"};
        u8 *d_text = nullptr;
        const u64 raw = bgzf_inflate_core(c, h_in, len, nullptr, cap, &d_text);
        bfq_phase("d2h_write");
        bfq_download(c, h_out, d_text, raw);
        c->sync();
        *out_len = raw;
    });
}

extern "C" int bfq_bgzf_inflate_device(bfq_ctx *c, const uint8_t *h_in, uint64_t len, uint8_t *d_out, uint64_t cap, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || !d_out) throw BfqError{BFQ_E_ARG, "null argument"};
        u8 *d_text = nullptr;
        *out_len = bgzf_inflate_core(c, h_in, len, d_out, cap, &d_text);
    });
}

extern "C" int bfq_bgzf_inflate_fd(bfq_ctx *c, int in_fd, uint64_t len, int out_fd, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        if (in_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        // the directory is read from the headers and trailers all over the file: the file is mapped, and uploaded from the mapping
        MappedInput map;
        if (!map.open(in_fd, (size_t)len)) throw BfqError{BFQ_E_IO, std::string("cannot map the input file: ") + strerror(errno)};
        u8 *d_text = nullptr;
        const u64 raw = bgzf_inflate_core(c, map.data(), len, nullptr, ~0ull, &d_text);
        if (out_fd >= 0) {
            bfq_phase("d2h_write");
            bfq_download(c, HostRef::file(out_fd, 0), d_text, raw);
            c->sync();
            bfq_fd_size(out_fd, raw, "cannot size the output file: ", true);
        }
        *out_len = raw;
    });
}

// ---------------------------------------------------------------- text sources: plain or BGZF, measured and placed once
// (fastq_upload_and_reserve and fastq_build_ebwt_oneshot of bfq_api.hip, both sides of bfq_compare.hip)
static TextIn src_in(const TextSrc &t) { TextIn in; in.ref = t.ref; in.len = t.len; return in; }
bool bfq_text_is_gzip(const TextSrc &t)
{
    const TextIn in = src_in(t);
    BfqTextSeen s;
    bfq_texts_look(nullptr, &in, 1, &s, false);
    return bfq_seen_gzip(s);
}
// staging of one BGZF part behind the text: compressed bytes | directory | status word, newline flag
static u64 stage_dir_off(u64 len) { return (len + 16 + 255) & ~255ull; }
static u64 stage_bytes(u64 len, u64 members) { return stage_dir_off(len) + ((24 * (members + 1) + 255) & ~255ull) + 256; }

void bfq_text_measure(const TextSrc *parts, int nparts, TextMeasure *M)
{
    M->nparts = nparts;
    M->bound = M->stage = 0;
    for (int p = 0; p < nparts; p++) {
        TextMeasure::Part &P = M->part[p];
        P = TextMeasure::Part{};
        if (parts[p].len && parts[p].ref.null()) throw BfqError{BFQ_E_ARG, "null FASTQ text"};
        const TextIn in = src_in(parts[p]);
        BfqTextSeen seen;                                          // one look: the first two bytes, then, of a plain part, the last
        bfq_texts_look(nullptr, &in, 1, &seen, false);
        if (!bfq_seen_gzip(seen)) {
            bfq_texts_look(nullptr, &in, 1, &seen, true);
            P.raw = parts[p].len;
            P.addNl = seen.last == 10 ? 0 : 1;
            M->bound += P.raw + P.addNl;
            continue;
        }
        // the directory is read from headers and trailers all over the file: a file is mapped for it
        const u8 *h = (const u8 *)parts[p].ref.ptr;
        void *map = MAP_FAILED;
        if (!h) {
            const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
            const u64 a0 = parts[p].ref.off / pg * pg;
            map = mmap(nullptr, (size_t)(parts[p].ref.off - a0 + parts[p].len), PROT_READ, MAP_PRIVATE, parts[p].ref.fd, (off_t)a0);
            if (map == MAP_FAILED) throw BfqError{BFQ_E_IO, std::string("cannot map the BGZF input: ") + strerror(errno)};
            h = (const u8 *)map + (parts[p].ref.off - a0);
        }
        u64 n = 0, raw = 0, bad = 0;
        int r = bfq_bgzf_walk(h, parts[p].len, nullptr, 0, &n, &raw, &bad);
        if (!r) {
            P.dir.resize(n);
            r = bfq_bgzf_walk(h, parts[p].len, P.dir.data(), n, &n, &raw, &bad);
        }
        if (map != MAP_FAILED) {
            const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
            munmap(map, (size_t)(parts[p].ref.off % pg + parts[p].len));
        }
        if (r) bgzf_refuse(n, bad, r);
        P.bgzf = true;
        P.raw = raw;
        P.addNl = raw ? 1 : 0;                                     // room for it; bfq_text_put settles it
        M->bound += raw + P.addNl;
        M->stage = std::max(M->stage, stage_bytes(parts[p].len, n));
    }
}

void bfq_text_put(bfq_ctx *c, const TextSrc *parts, TextMeasure *M, u8 *d_dst, u8 *d_stage, u64 *pstart)
{
    u64 at = 0;
    for (int p = 0; p < M->nparts; p++) {
        TextMeasure::Part &P = M->part[p];
        pstart[p] = at;
        if (!P.bgzf) {
            bfq_upload(c, d_dst + at, parts[p].ref, parts[p].len);
            if (P.addNl) HIP_CHECK(hipMemsetAsync(d_dst + at + parts[p].len, '\n', 1, c->stream));
            at += P.raw + P.addNl;
            continue;
        }
        const u64 n = P.dir.size();
        bfq_bgzf_member *d_dir = (bfq_bgzf_member *)(d_stage + stage_dir_off(parts[p].len));
        u64 *d_status = (u64 *)((u8 *)d_dir + ((24 * (n + 1) + 255) & ~255ull));
        bfq_upload(c, d_stage, parts[p].ref, parts[p].len);
        bfq_upload(c, d_dir, P.dir.data(), 24 * n);
        HIP_CHECK(hipMemsetAsync(d_status, 0xFF, 8, c->stream));
        HIP_CHECK(hipMemsetAsync(d_status + 1, 0, 8, c->stream));
        bfq_bgzf_launch(c, d_stage, d_dir, n, d_dst + at, P.raw, d_status);
        bfq_bgzf_newline(c, d_dst + at, P.raw, d_status + 1);
        u64 st[2] = {~0ull, 0};
        HIP_CHECK(hipMemcpyAsync(st, d_status, 16, hipMemcpyDeviceToHost, c->stream));
        c->sync();                                                // the next part starts behind this one's newline, if it got one
        if (st[0] != ~0ull) bgzf_refuse(st[0] >> 8, P.dir[st[0] >> 8].in_off, (int)(st[0] & 0xFF));
        P.addNl = (u8)st[1];
        at += P.raw + P.addNl;
    }
    pstart[M->nparts] = at;
}
