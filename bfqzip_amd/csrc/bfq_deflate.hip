// bfq_deflate.hip -- bgzip-compressed output (include/bfqzip_hip.h, bfq_bgzf_deflate*): a text cut into members of 65 280
// bytes, every member deflated on the device (k_deflate.hip).  The format and every bound are bfq_deflate.h's.
// The text goes through in batches of whole members; per batch:
//   1. every member is written into a worst-case slot (piece + 31, in whole words) of the arena,
//   2. the members' sizes are scanned,
//   3. the slots are gathered into contiguous output (the last batch: the EOF member behind them),
//   4. the output leaves through the background writers of bfq_io.hip while the next batch is uploaded and deflated (two
//      output buffers).
//   arena   one batch of text (unless it already lies on the device), its slots, sizes and offsets, the token rows of the
//           launch's workgroups, two output buffers: device memory does not grow with the length of the text
// bfq_bgzf_deflate_host is the host form of bfq_deflate.h, for tests and as the statement of the format: no entry point here
// falls back to it.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_deflate.h"

unsigned bfq_deflate_grid(u64 nm);                               // k_deflate.hip
u64 bfq_deflate_tok_words(u64 nm);
void bfq_deflate_launch(bfq_ctx *c, const u8 *d_in, u64 len, int level, u8 *d_slots, u32 *d_sizes, u32 *d_tok);
void bfq_deflate_gather(bfq_ctx *c, const u8 *d_slots, const u32 *d_sizes, const u64 *d_offs, u64 nm, u8 *d_out, bool eof);

#define DEFL_BATCH_MEMBERS 6144u                                 // four rounds of the launch's 1536 workgroups: 401 MB of text

static size_t defl_out_bytes(u64 mb) { return (size_t)mb * (BFQ_DEFL_PIECE + BFQ_DEFL_OVER) + BFQ_BGZF_EOF_LEN + 256; }
static size_t defl_need(u64 mb, bool hostSrc)
{
    return (hostSrc ? (size_t)mb * BFQ_DEFL_PIECE + 512 : 0) + (size_t)mb * BFQ_DEFL_SLOT + 12 * (size_t)(mb + 64) + 4 * (size_t)bfq_deflate_tok_words(mb) +
           2 * defl_out_bytes(mb) + 64 * (size_t)(mb / 1024 + 64) + (1u << 20);
}
// members per batch: BFQ_BGZF_BATCH (bytes of text, whole members), else the default, cut to what a capped arena holds
static u64 defl_batch_members(bfq_ctx *c, u64 len, bool hostSrc, size_t beside)
{
    u64 mb = c->env.bgzfBatch ? std::max<u64>(1, c->env.bgzfBatch / BFQ_DEFL_PIECE) : DEFL_BATCH_MEMBERS;
    mb = std::min(mb, std::max<u64>(1, bfq_defl_members(len)));
    while (!c->env.bgzfBatch && mb > 1 && c->wsLimit() && defl_need(mb, hostSrc) + beside > c->wsLimit()) mb = (mb + 1) / 2;
    return mb;
}
size_t bfq_deflate_need(bfq_ctx *c, u64 len, bool hostSrc, size_t beside) { return defl_need(defl_batch_members(c, len, hostSrc, beside), hostSrc); }

static void defl_check_level(int level)
{
    if (level != 0 && level != 1) throw BfqError{BFQ_E_ARG, "level: 0 (every member stored) or 1 (the compressor)"};
}
static void defl_refuse_gzip(const u8 first[2], u64 len)
{
    if (len >= 2 && first[0] == 0x1F && first[1] == 0x8B)
        throw BfqError{BFQ_E_ARG, "the input is already compressed (it begins with 1f 8b, a gzip member): nothing to deflate"};
}

// The BGZF form of a text of `len` bytes -- at d_text on the device, else at h_src -- to `dst` (memory or a file offset).
// held: the arena is the caller's, sized with bfq_deflate_need() beside what it holds; buffers go above the current top.
// Returns the length of the output.
u64 bfq_deflate_core(bfq_ctx *c, const u8 *d_text, HostRef h_src, u64 len, int level, HostRef dst, bool held, size_t beside)
{
    const bool hostSrc = d_text == nullptr;
    const u64 mb = defl_batch_members(c, len, hostSrc, beside);
    u8 eof[BFQ_BGZF_EOF_LEN];
    for (u32 i = 0; i < BFQ_BGZF_EOF_LEN; i++) eof[i] = bfq_defl_eof_byte(i);
    auto host_at = [](HostRef h, u64 off) { if (h.ptr) h.ptr = (char *)h.ptr + off; else h.off += off; return h; };
    if (!len) {                                                   // no member but the EOF one: nothing for the device
        if (dst.ptr) memcpy(dst.ptr, eof, sizeof eof);
        else if (pwrite(dst.fd, eof, sizeof eof, (off_t)dst.off) != (ssize_t)sizeof eof) throw BfqError{BFQ_E_IO, std::string("cannot write the output file: ") + strerror(errno)};
        return sizeof eof;
    }
    if (!held) {
        bfq_phase("alloc");
        c->reserve(defl_need(mb, hostSrc));
    }
    const size_t mk = c->mark();
    u8 *d_in = hostSrc ? c->alloc<u8>(mb * BFQ_DEFL_PIECE + 256) : nullptr;
    u8 *d_slots = c->alloc<u8>(mb * BFQ_DEFL_SLOT);
    u32 *d_sizes = c->alloc<u32>(mb + 1);
    u64 *d_offs = c->alloc<u64>(mb + 2);
    u32 *d_tok = c->alloc<u32>(bfq_deflate_tok_words(mb));
    u8 *d_out[2] = {c->alloc<u8>(defl_out_bytes(mb)), c->alloc<u8>(defl_out_bytes(mb))};
    c->call.writeHint = std::max(c->call.writeHint, (size_t)(len / 2));
    u64 at = 0;
    try {
        int buf = 0;
        for (u64 off = 0; off < len; off += mb * BFQ_DEFL_PIECE, buf ^= 1) {
            const u64 n = std::min<u64>(mb * BFQ_DEFL_PIECE, len - off), m = bfq_defl_members(n);
            const bool last = off + n == len;
            const u8 *text = d_text ? d_text + off : d_in;
            if (hostSrc) {
                bfq_phase("read_h2d");
                bfq_upload(c, d_in, host_at(h_src, off), n);
            }
            bfq_phase("gpu");
            bfq_deflate_launch(c, text, n, level, d_slots, d_sizes, d_tok);
            bfq_exscan_u32(c, d_sizes, d_offs, m, d_offs + m);
            bfq_deflate_gather(c, d_slots, d_sizes, d_offs, m, d_out[buf], last);
            u64 total = 0;
            HIP_CHECK(hipMemcpyAsync(&total, d_offs + m, 8, hipMemcpyDeviceToHost, c->stream));
            c->sync();
            if (total > m * (u64)(BFQ_DEFL_PIECE + BFQ_DEFL_OVER)) throw BfqError{BFQ_E_HIP, "BGZF writer: a batch above its bound"};
            if (last) total += BFQ_BGZF_EOF_LEN;
            bfq_phase("d2h_write");
            bfq_write_wait(c);                                    // the batch before: its buffer is the next one to be filled
            bfq_write_async(c, host_at(dst, at), d_out[buf], total);
            at += total;
        }
        bfq_write_wait(c);
    } catch (...) {
        try { bfq_write_wait(c); } catch (...) {}
        throw;
    }
    c->profCollect();
    c->release(mk);
    return at;
}

extern "C" uint64_t bfq_bgzf_deflate_bound(uint64_t len) { return bfq_defl_bound(len); }

extern "C" int bfq_bgzf_deflate_host(const uint8_t *h_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    if (!out_len || (!h_in && len) || !h_out || (level != 0 && level != 1) || cap < bfq_defl_bound(len)) return BFQ_E_ARG;
    if (len >= 2 && h_in[0] == 0x1F && h_in[1] == 0x8B) return BFQ_E_ARG;
    u64 ol = 0;
    const int r = bfq_defl_host(h_in, len, level, h_out, cap, &ol);
    if (r) return r == 2 ? BFQ_E_NOMEM : BFQ_E_ARG;
    *out_len = ol;
    return BFQ_OK;
}

extern "C" int bfq_bgzf_deflate(bfq_ctx *c, const uint8_t *h_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || (!h_in && len) || !h_out) throw BfqError{BFQ_E_ARG, "null argument"};
        defl_check_level(level);
        if (cap < bfq_defl_bound(len)) throw BfqError{BFQ_E_ARG, "output buffer below bfq_bgzf_deflate_bound(len)"};
        defl_refuse_gzip(h_in, len);
        *out_len = bfq_deflate_core(c, nullptr, HostRef::mem(h_in), len, level, HostRef::mem(h_out), false, 0);
    });
}

extern "C" int bfq_bgzf_deflate_device(bfq_ctx *c, const uint8_t *d_in, uint64_t len, int level, uint8_t *h_out, uint64_t cap, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len || (!d_in && len) || !h_out) throw BfqError{BFQ_E_ARG, "null argument"};
        defl_check_level(level);
        if (cap < bfq_defl_bound(len)) throw BfqError{BFQ_E_ARG, "output buffer below bfq_bgzf_deflate_bound(len)"};
        u8 first[2] = {0, 0};
        if (len >= 2) {
            HIP_CHECK(hipMemcpyAsync(first, d_in, 2, hipMemcpyDeviceToHost, c->stream));
            c->sync();
        }
        defl_refuse_gzip(first, len);
        *out_len = bfq_deflate_core(c, d_in, HostRef{}, len, level, HostRef::mem(h_out), false, 0);
    });
}

extern "C" int bfq_bgzf_deflate_fd(bfq_ctx *c, int in_fd, uint64_t len, int level, int out_fd, uint64_t *out_len)
{
    if (out_len) *out_len = 0;
    return guarded(c, [&] {
        if (!out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        if (in_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        defl_check_level(level);
        u8 first[2] = {0, 0};
        if (len >= 2 && pread(in_fd, first, 2, 0) != 2) throw BfqError{BFQ_E_IO, std::string("cannot read the input file: ") + strerror(errno)};
        defl_refuse_gzip(first, len);
        const u64 ol = bfq_deflate_core(c, nullptr, HostRef::file(in_fd, 0), len, level, HostRef::file(out_fd, 0), false, 0);
        bfq_fd_size(out_fd, ol, "cannot size the output file: ", true);
        *out_len = ol;
    });
}
