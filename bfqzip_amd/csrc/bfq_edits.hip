// bfq_edits.hip -- a run's base edits as the container BFQEDIT1 (include/bfqzip_hip.h): the entry points that make a member
// from the bases before and after a run and that write a member's bytes back.  The kernels are k_edits.hip's; this file moves
// the bytes and sizes the memory:
//   text buffer  the texts of a call (A then B, 256-byte aligned), uploaded through the staging workers
//   arena        their indexes; per read the count of its edits and the scan; per edit its position and byte (make) or its
//                position, byte and address in the target (apply); the member
// Nothing is written to the caller's outputs before every check has passed.
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_edits.h"

typedef unsigned long long ull;

[[noreturn]] static void ed_refuse(const char *fmt, ull a = 0, ull b = 0, ull c = 0)
{
    char m[280];
    snprintf(m, sizeof m, fmt, a, b, c);
    throw BfqError{BFQ_E_ARG, m};
}

// ---- make --------------------------------------------------------------------------------------------------------------------
// per read 4 (count) + 8 (scan) bytes; per edit 8 + 1 and the member; E <= cap whenever the member is going to fit
size_t bfq_edits_make_need(u64 N, u64 total, u64 cap)
{
    const u64 e = std::min(total, cap);
    return 12 * (size_t)(N + 64) + 9 * (size_t)(e + 64) + (size_t)bfq_edits_bound_of(e, std::max(total, e)) + 24 * (size_t)(bfq_edit_nseg(e) + 64) + (1u << 20);
}

u64 bfq_edits_make(bfq_ctx *c, EdSide A, EdSide B, const u64 *roff, u64 N, u64 total, u64 cap, u8 **d_member, bfq_edit_stats *st)
{
    *d_member = nullptr;
    if (total > BFQ_EDIT_TMAX) ed_refuse("more than 2^56 bases");
    u64 *d_s = c->alloc<u64>(8);                                  // bad read, shape, reads touched, target_sum, bad edit, edits, words
    u32 *cnt = c->alloc<u32>(N + 1);
    u64 *off = c->alloc<u64>(N + 1);
    HIP_CHECK(hipMemsetAsync(d_s, 0, 64, c->stream));
    HIP_CHECK(hipMemsetAsync(d_s, 0xFF, 8, c->stream));
    HIP_CHECK(hipMemsetAsync(d_s + 4, 0xFF, 8, c->stream));
    bfq_edit_check(c, A, B, roff, 0, N, d_s, d_s + 1);
    u64 h[8];
    {   // before a base is read: the offsets start at 0, end at `total`, and no read is longer than BFQ_MAX_READ_LEN (offsets
        // that are not ascending show as such a read); sides that are texts agree read by read
        u64 ends[2] = {0, total};
        HIP_CHECK(hipMemcpyAsync(h, d_s, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(ends, roff, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(ends + 1, roff + N, 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        if (ends[0] != 0 || ends[1] != total) ed_refuse("the read offsets run from %llu to %llu, not from 0 to the %llu bases stated", ends[0], ends[1], total);
        if (h[0] != ~0ull && !A.rec && !B.rec)
            ed_refuse("read %llu: longer than BFQ_MAX_READ_LEN, or the read offsets are not ascending", h[0]);
        if (h[0] != ~0ull) {
            const u64 r = h[0];
            u64 ro[2];
            FqRec ra, rb;
            memset(&ra, 0, sizeof ra); memset(&rb, 0, sizeof rb);
            HIP_CHECK(hipMemcpyAsync(ro, roff + r, 16, hipMemcpyDeviceToHost, c->stream));
            if (A.rec) HIP_CHECK(hipMemcpyAsync(&ra, A.rec + r, sizeof ra, hipMemcpyDeviceToHost, c->stream));
            if (B.rec) HIP_CHECK(hipMemcpyAsync(&rb, B.rec + r, sizeof rb, hipMemcpyDeviceToHost, c->stream));
            c->sync();
            const u64 l = ro[1] - ro[0];
            ed_refuse("read %llu: its sequence has %llu bases in A and %llu in B", r, A.rec ? ra.len : l, B.rec ? rb.len : l);
        }
    }
    bfq_edit_count(c, A, B, roff, N, total, cnt, d_s + 2);
    bfq_exscan_u32(c, cnt, off, N, d_s + 5);
    HIP_CHECK(hipMemcpyAsync(h, d_s, 64, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const u64 E = h[5], shape = h[1], touched = h[2];
    if (st) { st->reads = N; st->bases = total; st->edits = E; st->reads_touched = touched; st->bytes = 0; }
    if (E > cap) return bfq_edits_bound_of(E, total);             // not even its bytes fit
    const u64 nseg = bfq_edit_nseg(E), bound = bfq_edits_bound_of(E, total);
    u64 *pos = c->alloc<u64>(E + 1);
    u8 *byte = c->alloc<u8>(E + 8);
    u64 *words = c->alloc<u64>(nseg + 1), *wordOff = c->alloc<u64>(nseg + 1);
    u8 *z = c->alloc<u8>(bound + 8);
    HIP_CHECK(hipMemsetAsync(z, 0, bound, c->stream));
    bfq_edit_write(c, A, B, roff, N, E, cnt, off, pos, byte, d_s + 2);
    u64 *first = (u64 *)(z + BFQ_EDIT_HDR);
    u8 *wt = z + BFQ_EDIT_HDR + 8 * nseg;
    bfq_edit_segw(c, pos, byte, E, first, wt, words, d_s + 4);
    bfq_exscan_u64(c, words, wordOff, nseg, d_s + 6);
    HIP_CHECK(hipMemcpyAsync(h, d_s, 64, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (h[4] != ~0ull) {
        u64 g = 0;
        HIP_CHECK(hipMemcpyAsync(&g, pos + h[4], 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        ed_refuse("edit %llu (base %llu of the collection): A's byte there is outside 33..126", h[4], g);
    }
    const u64 nwords = h[6], payload = 8 * nseg + bfq_edit_pad8(nseg) + 8 * nwords + bfq_edit_pad8(E), len = BFQ_EDIT_HDR + payload;
    if (len > cap) return len;
    u64 *gaps = (u64 *)(wt + bfq_edit_pad8(nseg));
    bfq_edit_pack(c, pos, E, wt, wordOff, gaps);
    if (E) HIP_CHECK(hipMemcpyAsync(gaps + nwords, byte, E, hipMemcpyDeviceToDevice, c->stream));
    u8 hdr[BFQ_EDIT_HDR];
    bfq_edits_put_header(hdr, N, total, E, shape, h[3], payload);
    HIP_CHECK(hipMemcpyAsync(z, hdr, BFQ_EDIT_HDR, hipMemcpyHostToDevice, c->stream));
    c->sync();                                                    // (hdr is a stack variable)
    if (st) st->bytes = len;
    *d_member = z;
    return len;
}

[[noreturn]] static void ed_cap_refuse(u64 need, u64 cap)
{
    ed_refuse("the edits container needs %llu bytes, the buffer has %llu (cap_edits)", need, cap);
}

extern "C" int bfq_edits_make_device(bfq_ctx *c, const uint8_t *d_in_bases, const uint8_t *d_out_bases, const uint64_t *d_read_off, uint64_t N,
                                     uint64_t total, uint8_t *d_out, uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if (!d_read_off || !d_out || !out_len || (total && (!d_in_bases || !d_out_bases))) throw BfqError{BFQ_E_ARG, "null argument"};
        bfq_phase("alloc");
        c->reserve(bfq_edits_make_need(N, total, cap));
        bfq_phase("gpu");
        bfq_edit_stats S;
        u8 *z = nullptr;
        const u64 len = bfq_edits_make(c, EdSide{d_in_bases, nullptr, 0}, EdSide{d_out_bases, nullptr, 0}, (const u64 *)d_read_off, N, total, cap, &z, &S);
        if (!z) { if (stats) { *stats = S; stats->bytes = len; } ed_cap_refuse(len, cap); }
        HIP_CHECK(hipMemcpyAsync(d_out, z, len, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        c->profCollect();
        *out_len = len;
        if (stats) *stats = S;
    });
}

// ---- two FASTQ texts -> the member
using EdSrc = TextSrc;
struct EdInput { const EdSrc *parts; int nparts; u64 len; TextMeasure M; };

static void ed_measure(EdInput &in, const char *which)
{
    try { bfq_text_measure(in.parts, in.nparts, &in.M); }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw BfqError{e.code, std::string(which) + e.msg}; }
    in.len = in.M.bound;
}
static void ed_upload(bfq_ctx *c, EdInput &in, const char *which, u8 *d_dst, u8 *d_stage)
{
    u64 ps[BFQ_MAX_PARTS + 1];
    try { bfq_text_put(c, in.parts, &in.M, d_dst, d_stage, ps); }
    catch (const BfqError &e) { if (e.code != BFQ_E_ARG) throw; throw BfqError{e.code, std::string(which) + e.msg}; }
    in.len = ps[in.nparts];
}
static void ed_index(bfq_ctx *c, const char *which, const u8 *d_text, u64 len, DevFastq *fq)
{
    c->zeroCounters();
    try { bfq_fastq_index(c, d_text, len, fq); }
    catch (const BfqError &e) { throw BfqError{e.code, std::string(which) + e.msg}; }
    c->sync();                                                    // fq->total has arrived
}
static void ed_nomem(bfq_ctx *c, size_t need) { bfq_nomem_cap(c, "the edits", "the texts + index + edits", need); }

// both texts on the device -> the member in the arena; returns its length (the member at *z), or refuses
// needOut != nullptr: a member that does not fit `cap` is no refusal: *needOut = the size that suffices, *z stays nullptr
static u64 edits_of_texts(bfq_ctx *c, const u8 *d_a, u64 lenA, const u8 *d_b, u64 lenB, size_t resident, u64 cap, u8 **z, bfq_edit_stats *S,
                          u64 *needOut = nullptr)
{
    const u64 maxLen = std::max(lenA, lenB);
    bfq_phase("alloc");
    c->reserve(bfq_count_lines_bytes(maxLen) + (64u << 20));
    bfq_phase("gpu");
    const u64 nlA = bfq_fastq_count_lines(c, d_a, lenA), nlB = bfq_fastq_count_lines(c, d_b, lenB);
    const u64 Nb = std::max(nlA, nlB) / 4 + 1;
    const size_t perText = bfq_fastq_index_bytes(maxLen, std::max(nlA, nlB)) + 16 * (size_t)(Nb + 64) + 4 * (size_t)(maxLen / BFQ_NL_CHUNK) + 4096;
    const size_t need = 2 * perText + bfq_edits_make_need(Nb, lenA / 2, cap) + (8u << 20);
    if (c->wsLimit() && resident + need > c->wsLimit()) ed_nomem(c, resident + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    DevFastq fa, fb;
    ed_index(c, "A: ", d_a, lenA, &fa);
    ed_index(c, "B: ", d_b, lenB, &fb);
    if (fb.N != fa.N) ed_refuse("the texts differ in their number of records: %llu in A, %llu in B", fa.N, fb.N);
    const u64 len = bfq_edits_make(c, EdSide{d_a, (const FqRec *)fa.rec, 0}, EdSide{d_b, (const FqRec *)fb.rec, 0}, fa.roff, fa.N, fa.total, cap, z, S);
    if (!*z && needOut) { *needOut = len; return 0; }
    if (!*z) ed_cap_refuse(len, cap);
    return len;
}

// sink(z, len): the member, on the device, to wherever it goes; capOf(): the room there (known before the upload)
template <class Sink> static bool edits_core(bfq_ctx *c, EdInput A, EdInput B, u64 cap, bfq_edit_stats *stats, Sink sink, u64 *needOut = nullptr)
{
    ed_measure(A, "A: ");
    ed_measure(B, "B: ");
    const u64 offB = (A.len + 64 + 255) & ~255ull, sum = offB + ((B.len + 64 + 255) & ~255ull);
    const u64 stage = std::max(A.M.stage, B.M.stage);
    if (c->wsLimit() && sum + stage > c->wsLimit()) ed_nomem(c, sum + stage);
    bfq_phase("alloc");
    u8 *d_a = c->textBuf(sum + stage + 64), *d_b = d_a + offB;
    bfq_phase("read_h2d");
    ed_upload(c, A, "A: ", d_a, d_a + sum);
    ed_upload(c, B, "B: ", d_b, d_a + sum);
    bfq_edit_stats S;
    memset(&S, 0, sizeof S);
    u8 *z = nullptr;
    const u64 len = edits_of_texts(c, d_a, A.len, d_b, B.len, sum, cap, &z, &S, needOut);
    if (!z) return false;
    sink(z, len);
    c->sync();
    c->profCollect();
    if (stats) *stats = S;
    return true;
}

static void ed_parts(const bfq_text_part *p, int n, EdSrc *s)
{
    if (!p || n < 1 || n > BFQ_MAX_PARTS) throw BfqError{BFQ_E_ARG, "bfq_fastq_edits: 1..BFQ_MAX_PARTS parts for each of A and B"};
    for (int k = 0; k < n; k++) s[k] = EdSrc{HostRef::mem(p[k].data), p[k].len};
}

extern "C" int bfq_fastq_edits(bfq_ctx *c, const bfq_text_part *a, int na, const bfq_text_part *b, int nb, uint8_t *h_out, uint64_t cap,
                               uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if (!h_out || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        EdSrc sa[BFQ_MAX_PARTS], sb[BFQ_MAX_PARTS];
        ed_parts(a, na, sa);
        ed_parts(b, nb, sb);
        edits_core(c, EdInput{sa, na, 0, {}}, EdInput{sb, nb, 0, {}}, cap, stats, [&](const u8 *z, u64 len) {
            bfq_download_phase(c, h_out, z, len);
            *out_len = len;
        });
    });
}

extern "C" int bfq_fastq_edits_fd(bfq_ctx *c, int a_fd, uint64_t a_len, int b_fd, uint64_t b_len, int out_fd, uint64_t *out_len,
                                  bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if (a_fd < 0 || b_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        if (!out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });
        const EdSrc sa{HostRef::file(a_fd), a_len}, sb{HostRef::file(b_fd), b_len};
        u64 fin = 0, need = 0;
        auto sink = [&](const u8 *z, u64 len) {
            bfq_phase("d2h_write");
            F.open(0, len + 4096, len);
            bfq_download(c, F.at(0, 0), z, len);
            fin = len;
        };
        // the file has no capacity of its own: a member that outgrows the room reserved at first (input length / 8 + 4096:
        // enough while fewer than about a tenth of the bases differ) is made again in the room it asked for
        if (!edits_core(c, EdInput{&sa, 1, 0, {}}, EdInput{&sb, 1, 0, {}}, a_len / 8 + 4096, stats, sink, &need))
            edits_core(c, EdInput{&sa, 1, 0, {}}, EdInput{&sb, 1, 0, {}}, need, stats, sink);
        F.commit(&fin);
        *out_len = fin;
    });
}

extern "C" int bfq_fastq_edits_device(bfq_ctx *c, const uint8_t *d_a, uint64_t a_len, const uint8_t *d_b, uint64_t b_len, uint8_t *d_out,
                                      uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if ((!d_a && a_len) || (!d_b && b_len) || !d_out || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        bfq_edit_stats S;
        memset(&S, 0, sizeof S);
        u8 *z = nullptr;
        const u64 len = edits_of_texts(c, d_a, a_len, d_b, b_len, 0, cap, &z, &S);
        HIP_CHECK(hipMemcpyAsync(d_out, z, len, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        c->profCollect();
        *out_len = len;
        if (stats) *stats = S;
    });
}

// ---- apply -------------------------------------------------------------------------------------------------------------------
struct EdMembers { std::vector<BfqEditMember> m; std::vector<u64> at; u64 N = 0, T = 0, E = 0, maxE = 0, maxBytes = 0; };
static EdMembers ed_members(const u8 *h, u64 len)
{
    EdMembers R;
    if (!h || !len) ed_refuse("edits: not a BFQEDIT1 container (magic)");
    for (u64 at = 0; at < len;) {
        BfqEditMember M;
        u64 badSeg = ~0ull;
        if (const char *e = bfq_edits_member(h + at, len - at, &M, &badSeg)) {
            if (badSeg != ~0ull) ed_refuse("edits member %llu: damaged BFQEDIT1 container: edit %llu is the first bad one (a gap width above 56)", R.m.size(), badSeg * BFQ_EDIT_SEG);
            ed_refuse((std::string("edits member %llu: ") + e).c_str(), R.m.size());
        }
        R.m.push_back(M); R.at.push_back(at);
        R.N = R.N + M.N < R.N ? ~0ull : R.N + M.N;                  // (N is bounded by nothing in the file: the sums saturate)
        R.T = R.T + M.T < R.T ? ~0ull : R.T + M.T;
        R.E += M.E;                                                // (a member holds a byte per edit: bounded by len)
        R.maxE = std::max(R.maxE, M.E); R.maxBytes = std::max(R.maxBytes, M.bytes());
        at += M.bytes();
    }
    return R;
}
// the largest member + its segments' word offsets; per edit its position, byte and address
size_t bfq_edits_apply_need(const u8 *h_edits, u64 len)
{
    const EdMembers R = ed_members(h_edits, len);
    return (size_t)R.maxBytes + 8 * (size_t)(bfq_edit_nseg(R.maxE) + 64) + 17 * (size_t)(R.E + 64) + (1u << 20);
}

void bfq_edits_apply(bfq_ctx *c, const u8 *h_edits, u64 len, u8 *d_buf, EdSide X, const u64 *roff, u64 N, u64 total, bfq_edit_stats *st)
{
    const EdMembers R = ed_members(h_edits, len);
    if (R.N != N) ed_refuse("edits of %llu reads for a text of %llu reads", R.N, N);
    if (R.T != total) ed_refuse("edits of a collection of %llu bases for a text of %llu bases", R.T, total);
    u64 *d_s = c->alloc<u64>(8);                                  // bad read, shape, reads touched, target_sum, bad edit
    u64 *pos = c->alloc<u64>(R.E + 1), *addr = c->alloc<u64>(R.E + 1);
    u8 *byte = c->alloc<u8>(R.E + 8);
    u8 *z = c->alloc<u8>(R.maxBytes + 8);
    u64 *wordOff = c->alloc<u64>(bfq_edit_nseg(R.maxE) + 1);
    std::vector<u64> hw;
    u64 r0 = 0, g0 = 0, e0 = 0, touched = 0;
    for (size_t m = 0; m < R.m.size(); m++) {
        const BfqEditMember &M = R.m[m];
        const u8 *hz = h_edits + R.at[m];
        // what the member states is held against what is left of the target before it sizes a copy or a launch
        if (M.N > N - r0) ed_refuse("edits member %llu: %llu reads where the text has %llu left", m, M.N, N - r0);
        if (M.T > total - g0) ed_refuse("edits member %llu: a block of %llu bases where the text has %llu left", m, M.T, total - g0);
        u64 ro[2] = {0, 0};
        HIP_CHECK(hipMemcpyAsync(ro, roff + r0, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(ro + 1, roff + r0 + M.N, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemsetAsync(d_s, 0, 64, c->stream));
        HIP_CHECK(hipMemsetAsync(d_s, 0xFF, 8, c->stream));
        HIP_CHECK(hipMemsetAsync(d_s + 4, 0xFF, 8, c->stream));
        bfq_edit_check(c, EdSide{nullptr, nullptr, 0}, EdSide{nullptr, nullptr, 0}, roff, r0, M.N, d_s, d_s + 1);
        hw.assign(M.nseg + 1, 0);
        for (u64 s = 0; s < M.nseg; s++) hw[s + 1] = hw[s] + bfq_edit_seg_words(bfq_edit_seg_count(M.E, s), hz[M.offW + s]);
        bfq_upload(c, z, hz, M.bytes());
        if (M.nseg) bfq_upload(c, wordOff, hw.data(), 8 * M.nseg);
        u64 h[8];
        HIP_CHECK(hipMemcpyAsync(h, d_s, 64, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        if (ro[0] != g0 || ro[1] - ro[0] != M.T)
            ed_refuse("edits member %llu: a block of %llu bases where the text has %llu", m, M.T, ro[1] - ro[0]);
        if (h[0] != ~0ull) ed_refuse("read %llu: longer than BFQ_MAX_READ_LEN, or the read offsets are not ascending", h[0]);
        if (h[1] != M.shape)
            ed_refuse("edits member %llu: the read lengths are not those of the collection these edits were made from (shape %llu against %llu)", m, M.shape, h[1]);
        if (M.E) HIP_CHECK(hipMemcpyAsync(byte + e0, z + M.offBytes, M.E, hipMemcpyDeviceToDevice, c->stream));
        bfq_edit_unpack(c, (const u64 *)(z + M.offFirst), z + M.offW, (const u64 *)(z + M.offGaps), wordOff, M.E, pos + e0, d_s + 4);
        bfq_edit_locate(c, pos + e0, byte + e0, M.E, M.T, g0, X, roff, N, addr + e0, d_s + 4, d_s + 2);
        HIP_CHECK(hipMemcpyAsync(h, d_s, 64, hipMemcpyDeviceToHost, c->stream));
        c->sync();                                                // (z and wordOff are free for the next member)
        if (h[4] != ~0ull) ed_refuse("edits member %llu: damaged BFQEDIT1 container: edit %llu is the first bad one", m, h[4]);
        if (h[3] != M.targetSum) ed_refuse("edits member %llu: the text is not the output these edits were made from", m);
        touched += h[2];
        r0 += M.N; g0 += M.T; e0 += M.E;
    }
    bfq_edit_apply(c, addr, byte, R.E, d_buf);
    if (st) { st->reads = N; st->bases = total; st->edits = R.E; st->reads_touched = touched; st->bytes = len; }
}

extern "C" int bfq_edits_apply_device(bfq_ctx *c, const uint8_t *h_edits, uint64_t edits_len, uint8_t *d_bases, const uint64_t *d_read_off,
                                      uint64_t N, uint64_t total, int lines, bfq_edit_stats *stats)
{
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if (!d_read_off || (total && !d_bases)) throw BfqError{BFQ_E_ARG, "null argument"};
        const size_t need = bfq_edits_apply_need(h_edits, edits_len);
        bfq_phase("alloc");
        c->reserve(need);
        bfq_phase("gpu");
        bfq_edit_stats S;
        bfq_edits_apply(c, h_edits, edits_len, d_bases, EdSide{d_bases, nullptr, lines ? 1u : 0u}, (const u64 *)d_read_off, N, total, &S);
        c->sync();
        c->profCollect();
        if (stats) *stats = S;
    });
}

// one text + its edits -> the text with the input's bases.  sink(d_text, len)
template <class Sink> static void unedit_core(bfq_ctx *c, const EdSrc &src, const u8 *h_edits, u64 edits_len, bfq_edit_stats *stats, Sink sink)
{
    EdInput X{&src, 1, 0, {}};
    ed_measure(X, "");
    const size_t applyNeed = bfq_edits_apply_need(h_edits, edits_len);
    const u64 sum = (X.len + 64 + 255) & ~255ull;
    if (c->wsLimit() && sum + X.M.stage > c->wsLimit()) ed_nomem(c, sum + X.M.stage);
    bfq_phase("alloc");
    u8 *d_t = c->textBuf(sum + X.M.stage + 64);
    bfq_phase("read_h2d");
    ed_upload(c, X, "", d_t, d_t + sum);
    bfq_phase("alloc");
    c->reserve(bfq_count_lines_bytes(X.len) + (64u << 20));
    bfq_phase("gpu");
    const u64 nl = bfq_fastq_count_lines(c, d_t, X.len);
    const size_t need = bfq_fastq_index_bytes(X.len, nl) + 16 * (size_t)(nl / 4 + 64) + 4 * (size_t)(X.len / BFQ_NL_CHUNK) + 4096 + applyNeed + (8u << 20);
    if (c->wsLimit() && sum + need > c->wsLimit()) ed_nomem(c, sum + need);
    bfq_phase("alloc");
    c->reserve(need);
    bfq_phase("gpu");
    DevFastq fq;
    ed_index(c, "", d_t, X.len, &fq);
    bfq_edit_stats S;
    bfq_edits_apply(c, h_edits, edits_len, d_t, EdSide{d_t, (const FqRec *)fq.rec, 0}, fq.roff, fq.N, fq.total, &S);
    sink(d_t, X.len - X.M.part[0].addNl);                         // (the newline a text lacked is not handed back)
    c->sync();
    c->profCollect();
    if (stats) *stats = S;
}

extern "C" int bfq_fastq_unedit(bfq_ctx *c, const uint8_t *h_text, uint64_t len, const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out,
                                uint64_t cap, uint64_t *out_len, bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if ((!h_text && len) || !h_out || !out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        unedit_core(c, EdSrc{HostRef::mem(h_text), len}, h_edits, edits_len, stats, [&](const u8 *d_t, u64 n) {
            if (n > cap) ed_refuse("the output needs %llu bytes, the buffer has %llu", n, cap);
            bfq_download_phase(c, h_out, d_t, n);
            *out_len = n;
        });
    });
}

extern "C" int bfq_fastq_unedit_fd(bfq_ctx *c, int text_fd, uint64_t len, int edits_fd, uint64_t edits_len, int out_fd, uint64_t *out_len,
                                   bfq_edit_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) memset(stats, 0, sizeof *stats);
    return guarded(c, [&] {
        if (text_fd < 0 || edits_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        if (!out_len) throw BfqError{BFQ_E_ARG, "null argument"};
        std::vector<u8> ez(edits_len);                            // a few bytes per edit: read whole
        u64 got = 0;
        while (got < edits_len) {
            const ssize_t r = pread(edits_fd, ez.data() + got, (size_t)(edits_len - got), (off_t)got);
            if (r < 0 && errno == EINTR) continue;
            if (r <= 0) break;
            got += (u64)r;
        }
        if (got != edits_len) throw BfqError{BFQ_E_ARG, "edits: the file is shorter than edits_len"};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });
        u64 fin = 0;
        unedit_core(c, EdSrc{HostRef::file(text_fd), len}, ez.data(), edits_len, stats, [&](const u8 *d_t, u64 n) {
            bfq_phase("d2h_write");
            F.open(0, n + 4096, n);
            bfq_download(c, F.at(0, 0), d_t, n);
            fin = n;
        });
        F.commit(&fin);
        *out_len = fin;
    });
}
