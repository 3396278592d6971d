// bfq_restore.hip -- the way back: compressed streams in, FASTQ text out, in one call (include/bfqzip_hip.h,
// bfq_fastq_restore*).  The reference leaves this to `7z x` / `bsc d` and `paste` (BFQzip.py writes OUT.fq.dna / OUT.fq.qs /
// OUT.h and compresses each, :192-275); the record layout is bfq_int's (bfq_int.cpp:797-810).
//   host    the members of every input are walked and their raw lengths summed; the arena is reserved once from them
//   device  every member is decoded into its slice of two (three) stream buffers (k_codec.hip / k_dnac.hip; eBWT-domain
//           containers through the LF walk of bfq_ebwt_decode_lines), the line ends of each stream are compacted
//           (k_nl_count / k_nl_write), k_restore_index checks that the streams describe the same reads and builds the
//           record index, k_fq_format writes the text
// The decoded streams never leave the device: the containers go up, the text comes down.
// bfq_fastq_restore_ordered* also take the BFQPERM1 container of a reordering (bfq_perm.h) and write the records in the order
// the reads had before it: after k_restore_index the container is unpacked, validated and inverted (k_reorder.hip), the
// record sizes are scanned through the inverse and k_fq_format_ordered reads line inv[i] for record i -- no second pass over
// the text.
// bfq_fastq_restore_grouped* restore an archive block by block: rs_groups() cuts the members of the inputs into groups that
// decode on their own (one per block of a sharded run), the arena is reserved once for the largest group of the range, and
// every group goes through the pipeline above on its slices of the inputs; its text leaves the device from one of two
// buffers while the next group is decoded into the streams' space.
#include <string.h>
#include <stdio.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <algorithm>
#include "bfq_internal.h"
#include "bfq_device.h"
#include "bfq_perm.h"

// what k_restore_index found: (read index << 3) | reason, the smallest of all (so: the first offending read, and of two
// reasons at one read the one with the smaller code); RS_NONE: the streams fit
#define RS_NONE      (~0ull)
#define RS_LEN       1u      // DNA line i and quality line i differ in length
#define RS_LONG      2u      // line i is longer than BFQ_MAX_READ_LEN
#define RS_COUNT     3u      // the streams have different numbers of lines (index: the first read without a partner)
#define RS_HDR_COUNT 4u      // the header stream has another number of lines than there are reads

// One pass over the line-end arrays of the DNA, quality and (optional) header stream.  DNA line i and quality line i
// must be equally long, so the two arrays must be identical.  Per read: roff[i] = start of DNA line i minus i (= bases
// before it: read i lies at roff[i] + i in both line streams), the header span, the size of the record for the scan.
__global__ __launch_bounds__(256) void k_restore_index(const u64 *__restrict__ endD, u64 nD, const u64 *__restrict__ endQ, u64 nQ,
                                                       const u64 *__restrict__ endH, u64 nH, int haveHdr, u64 *__restrict__ roff,
                                                       u64 *__restrict__ hStart, u32 *__restrict__ hLen, u32 *__restrict__ sizes,
                                                       unsigned long long *__restrict__ err)
{
    const u64 N = nD < nQ ? nD : nQ;
    const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 bad = RS_NONE;
    if (tid == 0) {
        if (nD != nQ) bad = (N << 3) | RS_COUNT;
        if (haveHdr && nH != N) { const u64 b = ((nH < N ? nH : N) << 3) | RS_HDR_COUNT; if (b < bad) bad = b; }
        if (N == 0) roff[0] = 0;
    }
    for (u64 i = tid; i < N; i += (u64)gridDim.x * blockDim.x) {
        const u64 e = endD[i], s = i ? endD[i - 1] + 1 : 0;
        u64 L = e - s;
        if (endQ[i] != e) { const u64 b = (i << 3) | RS_LEN; if (b < bad) bad = b; }
        if (L > BFQ_MAX_READ_LEN) { const u64 b = (i << 3) | RS_LONG; if (b < bad) bad = b; L = 0; }
        roff[i] = s - i;
        if (i == N - 1) roff[N] = e + 1 - N;
        u32 hl = 1;                                              // "@"
        if (haveHdr) {
            u64 hs = 0;
            hl = 0;
            if (i < nH) { hs = i ? endH[i - 1] + 1 : 0; hl = (u32)(endH[i] - hs); }
            hStart[i] = hs; hLen[i] = hl;
        }
        sizes[i] = hl + 2u * (u32)L + 5u;
    }
    if (bad != RS_NONE && bad < *(volatile unsigned long long *)err) atomicMin(err, (unsigned long long)bad);
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct RsSrc { const u8 *h = nullptr; u64 len = 0; };          // a compressed input as host memory (its headers are parsed there)
struct RsPlan {
    bool ebwt = false;
    u64 rawD = 0, rawQ = 0, rawH = 0;       // decoded bytes of every stream (all members)
    u64 maxMember = 0;                      // ... of the largest single member (sizes the codec's workspace); a BFQNAME1 member's inner members count
    u64 hdrMember = 0;                      // ... of the header stream alone
    u64 nameExtra = 0;                      // the four decoded members of the largest BFQNAME1 member
    u64 readsBound = 0;                     // upper bound of the number of reads
    u64 textBound = 0;                      // ... and of the text
};

static u64 rs_get64(const u8 *p) { u64 v; memcpy(&v, p, 8); return v; }

// members of one input, back to back: raw length of all of them; *reads: the read count when every member states one
// (BFQDNAC1), else ~0
static u64 rs_walk(const RsSrc &s, const char *what, u64 *maxMember, u64 *reads, u64 *nameExtra = nullptr)
{
    if (!s.h || !s.len) throw BfqError{BFQ_E_ARG, std::string(what) + ": not a container (empty input)"};
    u64 raw = 0, nr = 0;
    for (u64 pos = 0; pos < s.len;) {
        u64 ml = 0, n = 0;
        try {
            ml = bfq_codec_member_len(s.h + pos, s.len - pos);
            n = bfq_codec_raw_len(s.h + pos, ml);
            if (!memcmp(s.h + pos, "BFQNAME1", 8)) {
                const u64 x = bfq_names_decode_extra(s.h + pos, ml, maxMember);
                if (nameExtra && x > *nameExtra) *nameExtra = x;
            }
        } catch (const BfqError &e) {
            char b[96];
            snprintf(b, sizeof b, ": not a container at byte %llu (", (unsigned long long)pos);
            throw BfqError{BFQ_E_ARG, std::string(what) + b + e.msg + ")"};
        }
        if (nr != ~0ull && ml >= 72 && !memcmp(s.h + pos, "BFQDNAC1", 8) && rs_get64(s.h + pos + 16) <= n) nr += rs_get64(s.h + pos + 16);
        else nr = ~0ull;
        if (n > (1ull << 46) || raw + n < raw) throw BfqError{BFQ_E_ARG, std::string(what) + ": not a container (raw length)"};
        raw += n;
        if (n > *maxMember) *maxMember = n;
        pos += ml;
    }
    if (reads) *reads = nr;
    return raw;
}

static void rs_plan(const RsSrc &dna, const RsSrc &qs, const RsSrc &hdr, bool haveHdr, RsPlan &P)
{
    if (!dna.h || !qs.h) throw BfqError{BFQ_E_ARG, "null argument"};
    u64 reads = ~0ull;
    if (dna.len >= 8 && !memcmp(dna.h, "BFQEBWT1", 8)) {
        // "BFQEBWT1" | rows | reads | terminator | flags | bytes of the symbols' container | that container | the patches' container
        const BfqError bad{BFQ_E_ARG, "dna: damaged BFQEBWT1 stream"};
        if (dna.len < 40) throw bad;
        const u64 n = rs_get64(dna.h + 8), N = rs_get64(dna.h + 16), symLen = rs_get64(dna.h + 32);
        if (symLen > dna.len - 40 || N > n) throw bad;
        u64 mm = 0;
        const RsSrc sym{dna.h + 40, symLen};
        if (rs_walk(sym, "dna (eBWT symbols)", &mm, nullptr) != n) throw bad;
        const u8 *pat = dna.h + 40 + symLen;
        const u64 patLen = dna.len - 40 - symLen;
        u64 pm = 0;
        try { pm = bfq_codec_member_len(pat, patLen); } catch (const BfqError &) { throw bad; }
        if (pm < patLen) {
            if (patLen - pm >= 8 && !memcmp(pat + pm, "BFQEBWT1", 8))
                throw BfqError{BFQ_E_ARG, "dna: more than one BFQEBWT1 member (eBWT-domain containers of several blocks are not supported)"};
            throw bad;
        }
        if (bfq_codec_raw_len(pat, patLen) != n) throw bad;
        P.ebwt = true;
        P.rawD = n;
        reads = N;
        P.rawQ = rs_walk(qs, "qs", &mm, nullptr);
        if (P.rawQ != n) {
            char b[160];
            snprintf(b, sizeof b, "qs: the quality container decodes to %llu bytes, the eBWT has %llu rows: not of the same collection",
                     (unsigned long long)P.rawQ, (unsigned long long)n);
            throw BfqError{BFQ_E_ARG, b};
        }
        if (bfq_codec_member_len(qs.h, qs.len) != qs.len) throw BfqError{BFQ_E_ARG, "qs: one member expected beside a BFQEBWT1 stream"};
        P.maxMember = n;
    } else {
        P.rawD = rs_walk(dna, "dna", &P.maxMember, &reads, &P.nameExtra);
        P.rawQ = rs_walk(qs, "qs", &P.maxMember, nullptr, &P.nameExtra);
    }
    if (haveHdr) {
        P.rawH = rs_walk(hdr, "hdr", &P.hdrMember, nullptr, &P.nameExtra);
        if (!P.ebwt) P.maxMember = std::max(P.maxMember, P.hdrMember);
    }
    // every line costs its stream one byte at least (a last line without '\n' gets one)
    const u64 byBytes = std::min(P.rawD, P.rawQ) + 1;
    P.readsBound = reads != ~0ull && reads < byBytes ? reads + 1 : byBytes;
    P.textBound = P.rawD + P.rawQ + 2 + 2 * P.readsBound + (haveHdr ? P.rawH + 1 : 2 * P.readsBound);   // "+\n", and "@\n" without headers
}

extern "C" int64_t bfq_fastq_restore_bound(const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                           const uint8_t *h_hdr, uint64_t hdr_len)
{
    try {
        RsPlan P;
        rs_plan(RsSrc{h_dna, dna_len}, RsSrc{h_qs, qs_len}, RsSrc{h_hdr, hdr_len}, h_hdr != nullptr, P);
        return (int64_t)P.textBound;
    } catch (const BfqError &) { return -1; }
}

// ---- the group plan -----------------------------------------------------------------------------------------------------
// one member at byte `pos` of an input: its bytes, its raw bytes, the reads it states (~0: none); a BFQEBWT1 member counts
// as one member of `rows` raw bytes
struct RsMember { u64 len = 0, raw = 0, reads = ~0ull; bool ebwt = false; };
static RsMember rs_member(const RsSrc &s, u64 pos, const char *what, u64 *maxMember, u64 *nameExtra)
{
    RsMember m;
    const u8 *p = s.h + pos;
    const u64 avail = s.len - pos;
    try {
        if (avail >= 8 && !memcmp(p, "BFQEBWT1", 8)) {
            const BfqError bad{BFQ_E_ARG, "damaged BFQEBWT1 stream"};
            if (avail < 40) throw bad;
            const u64 n = rs_get64(p + 8), N = rs_get64(p + 16), symLen = rs_get64(p + 32);
            if (symLen > avail - 40 || N > n) throw bad;
            u64 mm = 0;
            if (rs_walk(RsSrc{p + 40, symLen}, "eBWT symbols", &mm, nullptr) != n) throw bad;
            const u64 pm = bfq_codec_member_len(p + 40 + symLen, avail - 40 - symLen);
            if (bfq_codec_raw_len(p + 40 + symLen, pm) != n) throw bad;
            m.len = 40 + symLen + pm; m.raw = n; m.reads = N; m.ebwt = true;
        } else {
            m.len = bfq_codec_member_len(p, avail);
            m.raw = bfq_codec_raw_len(p, m.len);
            if (!memcmp(p, "BFQNAME1", 8)) {
                const u64 x = bfq_names_decode_extra(p, m.len, maxMember);
                if (nameExtra && x > *nameExtra) *nameExtra = x;
            }
            if (m.len >= 72 && !memcmp(p, "BFQDNAC1", 8) && rs_get64(p + 16) <= m.raw) m.reads = rs_get64(p + 16);
        }
    } catch (const BfqError &e) {
        char b[96];
        snprintf(b, sizeof b, ": not a container at byte %llu (", (unsigned long long)pos);
        throw BfqError{BFQ_E_ARG, std::string(what) + b + e.msg + ")"};
    }
    if (!m.len || m.raw > (1ull << 46)) throw BfqError{BFQ_E_ARG, std::string(what) + ": not a container (raw length)"};
    if (m.raw > *maxMember) *maxMember = m.raw;
    return m;
}

// a group of the plan: what the caller sees, and what sizes its share of the arena
struct RsGroup {
    bfq_restore_group g;
    u64 nD = 0, nQ = 0;                     // members
    bool ebwt = false;
    u64 maxMember = 0, hdrMember = 0, nameExtra = 0;   // as in RsPlan, for this group
    RsPlan plan(bool haveHdr) const
    {
        RsPlan P;
        P.ebwt = ebwt; P.rawD = P.rawQ = g.raw_stream; P.rawH = g.raw_hdr;
        P.maxMember = maxMember; P.hdrMember = hdrMember; P.nameExtra = nameExtra;
        const u64 byBytes = g.raw_stream + 1;
        P.readsBound = g.reads != ~0ull && g.reads < byBytes ? g.reads + 1 : byBytes;
        P.textBound = g.text_bound;
        return P;
    }
};

static u64 rs_rest(const RsSrc &s, u64 pos, const char *what)          // raw bytes of the members from `pos` on
{
    u64 raw = 0, mm = 0;
    while (pos < s.len) { const RsMember m = rs_member(s, pos, what, &mm, nullptr); raw += m.raw; pos += m.len; }
    return raw;
}

static std::vector<RsGroup> rs_groups(const RsSrc &dna, const RsSrc &qs, const RsSrc &hdr, bool haveHdr)
{
    if (!dna.h || !qs.h) throw BfqError{BFQ_E_ARG, "null argument"};
    for (const auto &pr : {std::make_pair(&dna, "dna"), std::make_pair(&qs, "qs"), std::make_pair(&hdr, "hdr")})
        if ((pr.first != &hdr || haveHdr) && (!pr.first->h || !pr.first->len))
            throw BfqError{BFQ_E_ARG, std::string(pr.second) + ": not a container (empty input)"};
    std::vector<RsGroup> G;
    u64 pD = 0, pQ = 0, totD = 0, totQ = 0;
    auto unequal = [&]() {
        char b[200];
        snprintf(b, sizeof b, "the DNA members decode to %llu bytes, the quality members to %llu: not of the same collection",
                 (unsigned long long)(totD + rs_rest(dna, pD, "dna")), (unsigned long long)(totQ + rs_rest(qs, pQ, "qs")));
        return BfqError{BFQ_E_ARG, b};
    };
    while (pD < dna.len || pQ < qs.len) {
        RsGroup r;
        memset(&r.g, 0, sizeof r.g);
        r.g.dna_off = pD; r.g.qs_off = pQ;
        u64 rawD = 0, rawQ = 0, reads = 0;
        auto takeD = [&]() {
            if (pD >= dna.len) throw unequal();
            const RsMember m = rs_member(dna, pD, "dna", &r.maxMember, &r.nameExtra);
            pD += m.len; rawD += m.raw; totD += m.raw; r.nD++;
            r.ebwt = r.ebwt || m.ebwt;
            reads = (reads == ~0ull || m.reads == ~0ull) ? ~0ull : reads + m.reads;
        };
        auto takeQ = [&]() {
            if (pQ >= qs.len) throw unequal();
            const RsMember m = rs_member(qs, pQ, "qs", &r.maxMember, &r.nameExtra);
            if (m.ebwt) throw BfqError{BFQ_E_ARG, "qs: a BFQEBWT1 member in the quality input"};
            pQ += m.len; rawQ += m.raw; totQ += m.raw; r.nQ++;
        };
        takeD(); takeQ();
        while (rawD != rawQ) { if (rawD < rawQ) takeD(); else takeQ(); }
        if (r.ebwt && (r.nD != 1 || r.nQ != 1)) {
            char b[200];
            snprintf(b, sizeof b, "group %llu: one DNA member and one quality member of the same raw length expected where the DNA member is a BFQEBWT1",
                     (unsigned long long)G.size());
            throw BfqError{BFQ_E_ARG, b};
        }
        r.g.dna_len = pD - r.g.dna_off; r.g.qs_len = pQ - r.g.qs_off;
        r.g.raw_stream = rawD; r.g.reads = reads;
        G.push_back(r);
    }
    if (haveHdr) {
        u64 pH = 0, k = 0;
        while (pH < hdr.len) {
            RsGroup scratch;
            RsGroup &r = k < G.size() ? G[k] : scratch;
            const RsMember m = rs_member(hdr, pH, "hdr", &r.hdrMember, &r.nameExtra);
            if (m.ebwt) throw BfqError{BFQ_E_ARG, "hdr: a BFQEBWT1 member in the header input"};
            if (k < G.size()) { r.g.hdr_off = pH; r.g.hdr_len = m.len; r.g.raw_hdr = m.raw; if (!r.ebwt) r.maxMember = std::max(r.maxMember, r.hdrMember); }
            pH += m.len; k++;
        }
        if (k != G.size()) {
            char b[240];
            snprintf(b, sizeof b, "hdr: %llu header members for %llu groups of DNA and quality members: the header stream was not cut with the blocks; "
                                  "restore the archive in one piece", (unsigned long long)k, (unsigned long long)G.size());
            throw BfqError{BFQ_E_ARG, b};
        }
    }
    for (auto &r : G) {                                           // the bound of rs_plan, group by group
        const u64 byBytes = r.g.raw_stream + 1;
        const u64 rb = r.g.reads != ~0ull && r.g.reads < byBytes ? r.g.reads + 1 : byBytes;
        r.g.text_bound = 2 * r.g.raw_stream + 2 + 2 * rb + (haveHdr ? r.g.raw_hdr + 1 : 2 * rb);
    }
    return G;
}

extern "C" int64_t bfq_fastq_restore_groups(const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                            const uint8_t *h_hdr, uint64_t hdr_len, bfq_restore_group *groups, uint64_t cap,
                                            char *why, int why_cap)
{
    if (why && why_cap > 0) why[0] = 0;
    try {
        const std::vector<RsGroup> G = rs_groups(RsSrc{h_dna, dna_len}, RsSrc{h_qs, qs_len}, RsSrc{h_hdr, hdr_len}, h_hdr != nullptr);
        for (u64 k = 0; groups && k < G.size() && k < cap; k++) groups[k] = G[k].g;
        return (int64_t)G.size();
    } catch (const BfqError &e) {
        if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "%s", e.msg.c_str());
        return e.code;
    } catch (const std::bad_alloc &) {
        if (why && why_cap > 0) snprintf(why, (size_t)why_cap, "host out of memory");
        return BFQ_E_NOMEM;
    }
}

extern "C" int64_t bfq_stream_members(const uint8_t *h_in, uint64_t len)
{
    try {
        int64_t k = 0;
        u64 mm = 0;
        const RsSrc s{h_in, len};
        for (u64 pos = 0; h_in && pos < len; k++) pos += rs_member(s, pos, "stream", &mm, nullptr).len;
        return k;
    } catch (const BfqError &) { return -1; }
}

// all members of `s` into d_out (raw bytes in all); d_z: room for the compressed bytes
static void rs_decode(bfq_ctx *c, const RsSrc &s, u8 *d_z, u8 *d_out, u64 raw)
{
    bfq_upload(c, d_z, s.h, s.len);
    u64 got = 0;
    for (u64 pos = 0; pos < s.len;) {
        const u64 ml = bfq_codec_member_len(s.h + pos, s.len - pos);
        got += bfq_codec_decompress_device(c, s.h + pos, d_z + pos, ml, d_out + got, raw - got);
        pos += ml;
    }
    if (got != raw) throw BfqError{BFQ_E_ARG, "damaged container (raw length)"};
}

static size_t rs_index_bytes(const RsPlan &P, bool ordered)
{
    // line ends of three streams, roff, hStart, hLen, sizes, recOff per read; chunk counts of the line index and of the scans;
    // ordered: the container's payload, the unpacked permutation, its inverse (8 bytes each) and the sizes in output order
    return (ordered ? 64 + 32 : 64) * (size_t)(P.readsBound + 64) + 3 * 32 * (size_t)((std::max(P.rawD, std::max(P.rawQ, P.rawH)) >> 12) + 64) + (1u << 20);
}

// what k_restore_index found, as the error of the call.  base: reads before the first one of these streams (a group of an
// archive), where: what to add to the sentence (the group)
static BfqError rs_read_error(u64 err, u64 nD, u64 nQ, u64 nH, u64 N, u64 base, const char *where)
{
    const unsigned long long i = base + (err >> 3);
    char b[320];
    switch ((u32)(err & 7)) {
    case RS_LEN:
        snprintf(b, sizeof b, "read %llu%s: its DNA line and its quality line differ in length (streams of different collections?)", i, where);
        break;
    case RS_LONG:
        snprintf(b, sizeof b, "read %llu%s: line longer than BFQ_MAX_READ_LEN (%d)", i, where, BFQ_MAX_READ_LEN);
        break;
    case RS_COUNT:
        snprintf(b, sizeof b, "read %llu%s has no partner: the DNA stream has %llu lines, the quality stream %llu", i, where, (unsigned long long)nD,
                 (unsigned long long)nQ);
        break;
    default:
        snprintf(b, sizeof b, "read %llu%s: the header stream has %llu lines for %llu reads", i, where, (unsigned long long)nH, (unsigned long long)N);
        break;
    }
    return BfqError{BFQ_E_ARG, b};
}

// sink: where the text goes once it is known to be good.  put(d_text, len) is called at most once.
struct RsSink {
    u64 cap = ~0ull;
    std::function<void(u64)> sized;                 // the length of the text is known (before it is formatted)
    std::function<void(const u8 *, u64)> put;
    std::function<size_t(u64)> extraWs;             // arena bytes put() takes above a text of at most this length (unset: none)
};

// permz != nullptr: the records leave in the order before the reordering whose BFQPERM1 container this is
// edits != nullptr: the BFQEDIT1 members of the run's base edits: the decoded DNA lines get the input's bytes back, in the
// order of the run, before the text is formatted (no second pass over it)
static void restore_core(bfq_ctx *c, const RsSrc &dna, const RsSrc &qs, const RsSrc &hdr, bool haveHdr, const RsSink &sink,
                         uint64_t *out_len, uint64_t *n_reads, const RsSrc *permz = nullptr, const RsSrc *edits = nullptr)
{
    if (out_len) *out_len = 0;
    if (n_reads) *n_reads = 0;
    RsPlan P;
    rs_plan(dna, qs, hdr, haveHdr, P);
    size_t editsWs = 0;                                           // bytes that are no members take no room: they are refused where the
    if (edits) {                                                  // edits are applied, after the streams have had their say
        try { editsWs = bfq_edits_apply_need(edits->h, edits->len); } catch (const BfqError &) {}
    }
    const size_t afterDecode = rs_index_bytes(P, permz != nullptr) + P.textBound + 4096 + (sink.extraWs ? sink.extraWs(P.textBound) : 0) + editsWs;
    u8 *dD = nullptr, *dQ = nullptr, *dH = nullptr;
    u64 lenD = P.rawD, lenQ = P.rawQ;
    if (P.ebwt) {
        const size_t hdrPart = haveHdr ? P.rawH + hdr.len + bfq_codec_workspace(std::max(P.rawH, P.hdrMember)) + P.nameExtra : 0;
        EbwtLines r;
        bfq_phase("alloc");
        bfq_ebwt_decode_lines(c, dna.h, dna.len, qs.h, qs.len, nullptr, nullptr, ~0ull, nullptr, nullptr, afterDecode + hdrPart + 4096, &r);
        if (!r.n) { c->reserve(afterDecode + hdrPart + (64u << 20)); r.dna = c->alloc<u8>(64); r.qs = c->alloc<u8>(64); }
        dD = r.dna; dQ = r.qs;
        if (haveHdr) {
            dH = c->alloc<u8>(P.rawH + 64);
            const size_t mk = c->mark();
            rs_decode(c, hdr, c->alloc<u8>(hdr.len + 64), dH, P.rawH);
            c->release(mk);
        }
    } else {
        const size_t streams = (size_t)P.rawD + P.rawQ + P.rawH + 3 * 320;
        const size_t decode = (size_t)dna.len + qs.len + (haveHdr ? hdr.len : 0) + 3 * 320 + bfq_codec_workspace(P.maxMember) + P.nameExtra;
        bfq_phase("alloc");
        c->reserve(streams + std::max(decode, afterDecode) + (64u << 20));
        c->zeroCounters();
        dD = c->alloc<u8>(P.rawD + 64); dQ = c->alloc<u8>(P.rawQ + 64);
        if (haveHdr) dH = c->alloc<u8>(P.rawH + 64);
        const size_t mk = c->mark();
        u8 *zD = c->alloc<u8>(dna.len + 64), *zQ = c->alloc<u8>(qs.len + 64), *zH = haveHdr ? c->alloc<u8>(hdr.len + 64) : nullptr;
        bfq_phase("read_h2d");
        rs_decode(c, dna, zD, dD, P.rawD);
        bfq_phase("gpu");
        rs_decode(c, qs, zQ, dQ, P.rawQ);
        if (haveHdr) rs_decode(c, hdr, zH, dH, P.rawH);
        c->release(mk);
    }
    bfq_phase("gpu");
    // line ends (a last line without '\n' gets one) and the record index
    u64 nD = 0, nQ = 0, nH = 0;
    const u64 *endD = bfq_line_index(c, dD, lenD, &nD);
    const u64 *endQ = bfq_line_index(c, dQ, lenQ, &nQ);
    const u64 *endH = haveHdr ? bfq_line_index(c, dH, P.rawH, &nH) : nullptr;
    const u64 N = std::min(nD, nQ);
    u64 *roff = c->alloc<u64>(N + 2), *recOff = c->alloc<u64>(N + 2);
    u64 *hStart = haveHdr ? c->alloc<u64>(N + 1) : nullptr;
    u32 *hLen = haveHdr ? c->alloc<u32>(N + 1) : nullptr, *sizes = c->alloc<u32>(N + 1);
    unsigned long long *d_err = (unsigned long long *)c->alloc<u64>(1);
    HIP_CHECK(hipMemsetAsync(d_err, 0xFF, 8, c->stream));
    KLAUNCH(c, K_RESTORE, (haveHdr ? 48.0 : 28.0) * (double)N, k_restore_index, bfq_grid(N ? N : 1, 256), 256, endD, nD, endQ, nQ, endH, nH,
            haveHdr ? 1 : 0, roff, hStart, hLen, sizes, d_err);
    bfq_exscan_u32(c, sizes, recOff, N, recOff + N);
    u64 err = RS_NONE, ol = 0;
    HIP_CHECK(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&ol, recOff + N, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (err != RS_NONE) throw rs_read_error(err, nD, nQ, nH, N, 0, "");
    const u64 *inv = nullptr;
    if (permz) {
        u64 PN = 0;
        if (!bfq_perm_header(permz->h, permz->len, &PN, nullptr, nullptr))
            throw BfqError{BFQ_E_ARG, "perm: not a BFQPERM1 container (magic, entry width, length or padding)"};
        if (PN != N) {
            char b[200];
            snprintf(b, sizeof b, "perm: a permutation of %llu reads for streams of %llu reads", (unsigned long long)PN, (unsigned long long)N);
            throw BfqError{BFQ_E_ARG, b};
        }
        const u64 nw = bfq_perm_words(N, bfq_perm_width(N));
        u64 *words = c->alloc<u64>(nw + 1), *perm = c->alloc<u64>(N + 1), *iv = c->alloc<u64>(N + 1);
        if (nw) bfq_upload(c, words, permz->h + BFQ_PERM_HDR, 8 * nw);
        const u64 bad = bfq_perm_unpack_invert(c, words, N, perm, iv);
        if (bad != BFQ_PERM_NOPOS) {
            char b[200];
            snprintf(b, sizeof b, "perm: not a permutation: entry %llu is out of range or repeats an earlier one", (unsigned long long)bad);
            throw BfqError{BFQ_E_ARG, b};
        }
        inv = iv;
    }
    if (edits) {                                                  // every member is held against the streams before a base is written
        u64 total = 0;
        HIP_CHECK(hipMemcpyAsync(&total, roff + N, 8, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        bfq_edits_apply(c, edits->h, edits->len, dD, EdSide{dD, nullptr, 1u}, roff, N, total, nullptr);
    }
    if (ol > sink.cap) throw BfqError{BFQ_E_ARG, "output buffer smaller than the FASTQ text (see bfq_fastq_restore_bound)"};
    if (sink.sized) sink.sized(ol);
    if (inv) {                                                    // the same sizes in output order: the same total
        u32 *sizesOut = c->alloc<u32>(N + 1);
        bfq_restore_sizes_ordered(c, sizes, inv, N, sizesOut);
        bfq_exscan_u32(c, sizesOut, recOff, N, recOff + N);
    }
    u8 *d_out = c->alloc<u8>(ol + 64);
    if (inv) bfq_fastq_format_ordered(c, dD, dQ, roff, dH, hStart, hLen, recOff, inv, N, ol, d_out);
    else bfq_fastq_format_lines(c, dD, dQ, roff, dH, hStart, hLen, recOff, N, ol, d_out);
    sink.put(d_out, ol);
    c->profCollect();
    if (out_len) *out_len = ol;
    if (n_reads) *n_reads = N;
}

static int rs_run_mem(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len, const uint8_t *h_hdr,
                      uint64_t hdr_len, const RsSrc *permz, uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads,
                      const RsSrc *edits = nullptr)
{
    return guarded(c, [&] {
        if (!h_dna || !h_qs || (!h_out && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        RsSink sink;
        sink.cap = cap;
        sink.put = [&](const u8 *d_text, u64 len) {
            bfq_phase("d2h_write");
            bfq_download(c, h_out, d_text, len);
            c->sync();                                            // pinned destinations are written by asynchronous DMA
        };
        restore_core(c, RsSrc{h_dna, dna_len}, RsSrc{h_qs, qs_len}, RsSrc{h_hdr, hdr_len}, h_hdr != nullptr, sink, out_len, n_reads, permz, edits);
    });
}

extern "C" int bfq_fastq_restore(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                 const uint8_t *h_hdr, uint64_t hdr_len, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                                 uint64_t *n_reads)
{
    return rs_run_mem(c, h_dna, dna_len, h_qs, qs_len, h_hdr, hdr_len, nullptr, h_out, cap, out_len, n_reads);
}

extern "C" int bfq_fastq_restore_ordered(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                         const uint8_t *h_hdr, uint64_t hdr_len, const uint8_t *h_permz, uint64_t permz_len,
                                         uint8_t *h_out, uint64_t cap, uint64_t *out_len, uint64_t *n_reads)
{
    const RsSrc permz{h_permz, permz_len};
    return rs_run_mem(c, h_dna, dna_len, h_qs, qs_len, h_hdr, hdr_len, &permz, h_out, cap, out_len, n_reads);
}

// a compressed input file as read-only memory (its pages are the page cache's; the staging workers copy from them)
struct RsMap {
    void *p = nullptr; size_t len = 0;
    const u8 *open(int fd, u64 n)
    {
        if (!n) return nullptr;
        void *m = mmap(nullptr, (size_t)n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) throw BfqError{BFQ_E_IO, "cannot map an input file"};
        p = m; len = (size_t)n;
        (void)madvise(m, len, MADV_SEQUENTIAL);
        return (const u8 *)m;
    }
    ~RsMap() { if (p) munmap(p, len); }
};

static int rs_run_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len, bool ordered,
                     int perm_fd, uint64_t permz_len, int out_fd, uint64_t *out_len, uint64_t *n_reads, int edits_fd = -1, uint64_t edits_len = 0)
{
    if (out_len) *out_len = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (dna_fd < 0 || qs_fd < 0 || out_fd < 0 || (ordered && perm_fd < 0)) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        const bool haveHdr = hdr_fd >= 0;
        RsMap mD, mQ, mH, mP, mE;
        const bool edited = edits_fd >= 0;
        struct stat st;
        if (edited && fstat(edits_fd, &st) == 0 && S_ISREG(st.st_mode) && (u64)st.st_size < edits_len) edits_len = (u64)st.st_size;   // (refused as members below)
        const RsSrc editz{edited ? mE.open(edits_fd, edits_len) : nullptr, edited ? edits_len : 0};
        if (ordered && fstat(perm_fd, &st) == 0 && S_ISREG(st.st_mode) && (u64)st.st_size < permz_len) permz_len = (u64)st.st_size;   // (refused as a container below)
        const RsSrc permz{ordered ? mP.open(perm_fd, permz_len) : nullptr, ordered ? permz_len : 0};
        const RsSrc dna{mD.open(dna_fd, dna_len), dna_len}, qs{mQ.open(qs_fd, qs_len), qs_len};
        const RsSrc hdr{haveHdr ? mH.open(hdr_fd, hdr_len) : nullptr, haveHdr ? hdr_len : 0};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });
        RsPlan P;
        rs_plan(dna, qs, hdr, haveHdr, P);
        // mapped to the bound; what is certain of it (the bases, the qualities and their newlines) is pre-faulted beside
        // the upload and the decoding
        F.open(0, P.textBound + 4096, P.rawD + P.rawQ);
        RsSink sink;
        sink.sized = [&](u64 len) { F.extend(0, len); };
        sink.put = [&](const u8 *d_text, u64 len) {
            bfq_write_async(c, F.at(0, 0), d_text, len);
            c->sync();
            bfq_phase("d2h_write");
            bfq_write_wait(c);
        };
        uint64_t ol = 0;
        restore_core(c, dna, qs, hdr, haveHdr, sink, &ol, n_reads, ordered ? &permz : nullptr, edited ? &editz : nullptr);
        F.commit(&ol);
        if (out_len) *out_len = ol;
    });
}

extern "C" int bfq_fastq_restore_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                    int out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    return rs_run_fd(c, dna_fd, dna_len, qs_fd, qs_len, hdr_fd, hdr_len, false, -1, 0, out_fd, out_len, n_reads);
}

extern "C" int bfq_fastq_restore_ordered_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                            int perm_fd, uint64_t permz_len, int out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    return rs_run_fd(c, dna_fd, dna_len, qs_fd, qs_len, hdr_fd, hdr_len, true, perm_fd, permz_len, out_fd, out_len, n_reads);
}

// bfq_fastq_restore_ordered with an optional permutation and optional edits
extern "C" int bfq_fastq_restore_edited(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                        const uint8_t *h_hdr, uint64_t hdr_len, const uint8_t *h_permz, uint64_t permz_len,
                                        const uint8_t *h_edits, uint64_t edits_len, uint8_t *h_out, uint64_t cap, uint64_t *out_len,
                                        uint64_t *n_reads)
{
    const bool ordered = h_permz != nullptr || permz_len != 0, edited = h_edits != nullptr || edits_len != 0;
    const RsSrc permz{h_permz, permz_len}, editz{h_edits, edits_len};
    return rs_run_mem(c, h_dna, dna_len, h_qs, qs_len, h_hdr, hdr_len, ordered ? &permz : nullptr, h_out, cap, out_len, n_reads, edited ? &editz : nullptr);
}

extern "C" int bfq_fastq_restore_edited_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                           int perm_fd, uint64_t permz_len, int edits_fd, uint64_t edits_len, int out_fd, uint64_t *out_len,
                                           uint64_t *n_reads)
{
    return rs_run_fd(c, dna_fd, dna_len, qs_fd, qs_len, hdr_fd, hdr_len, perm_fd >= 0, perm_fd, permz_len, out_fd, out_len, n_reads, edits_fd, edits_len);
}

// The text deflated where it lies (bfq_deflate.hip): the FASTQ text never crosses to the host.
size_t bfq_deflate_need(bfq_ctx *c, u64 len, bool hostSrc, size_t beside);
u64 bfq_deflate_core(bfq_ctx *c, const u8 *d_text, HostRef h_src, u64 len, int level, HostRef dst, bool held, size_t beside);

extern "C" int bfq_fastq_restore_bgzf_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                         int perm_fd, uint64_t permz_len, int level, int out_fd, uint64_t *out_len, uint64_t *raw_len,
                                         uint64_t *n_reads)
{
    if (out_len) *out_len = 0;
    if (raw_len) *raw_len = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (dna_fd < 0 || qs_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        if (level != 0 && level != 1) throw BfqError{BFQ_E_ARG, "level: 0 (every member stored) or 1 (the compressor)"};
        const bool haveHdr = hdr_fd >= 0, ordered = perm_fd >= 0;
        RsMap mD, mQ, mH, mP;
        struct stat st;
        if (ordered && fstat(perm_fd, &st) == 0 && S_ISREG(st.st_mode) && (u64)st.st_size < permz_len) permz_len = (u64)st.st_size;
        const RsSrc permz{ordered ? mP.open(perm_fd, permz_len) : nullptr, ordered ? permz_len : 0};
        const RsSrc dna{mD.open(dna_fd, dna_len), dna_len}, qs{mQ.open(qs_fd, qs_len), qs_len};
        const RsSrc hdr{haveHdr ? mH.open(hdr_fd, hdr_len) : nullptr, haveHdr ? hdr_len : 0};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });         // never mapped: the deflated members go through the descriptor
        u64 zl = 0;
        RsSink sink;
        sink.extraWs = [&](u64 bound) { return bfq_deflate_need(c, bound, false, 0); };
        sink.put = [&](const u8 *d_text, u64 len) { zl = bfq_deflate_core(c, d_text, HostRef{}, len, level, F.at(0, 0), true, 0); };
        uint64_t ol = 0, nr = 0;
        restore_core(c, dna, qs, hdr, haveHdr, sink, &ol, &nr, ordered ? &permz : nullptr);
        F.commit(&zl);
        if (out_len) *out_len = zl;
        if (raw_len) *raw_len = ol;
        if (n_reads) *n_reads = nr;
    });
}

// The restored text turned into unaligned BAM records where it lies, and those deflated where they lie (bfq_ubam.hip).
size_t bfq_ubam_held_need(bfq_ctx *c, u64 bound, const bfq_ubam_opts *opts);
u64 bfq_ubam_held(bfq_ctx *c, const u8 *d_text, u64 len, const bfq_ubam_opts *opts, HostRef dst, bfq_ubam_stats *stats);

extern "C" int bfq_fastq_restore_bam_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len, int perm_fd,
                                        uint64_t permz_len, const bfq_ubam_opts *opts, int out_fd, uint64_t *out_len, bfq_ubam_stats *stats)
{
    if (out_len) *out_len = 0;
    if (stats) *stats = bfq_ubam_stats{};
    return guarded(c, [&] {
        if (dna_fd < 0 || qs_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        const bool haveHdr = hdr_fd >= 0, ordered = perm_fd >= 0;
        RsMap mD, mQ, mH, mP;
        struct stat st;
        if (ordered && fstat(perm_fd, &st) == 0 && S_ISREG(st.st_mode) && (u64)st.st_size < permz_len) permz_len = (u64)st.st_size;
        const RsSrc permz{ordered ? mP.open(perm_fd, permz_len) : nullptr, ordered ? permz_len : 0};
        const RsSrc dna{mD.open(dna_fd, dna_len), dna_len}, qs{mQ.open(qs_fd, qs_len), qs_len};
        const RsSrc hdr{haveHdr ? mH.open(hdr_fd, hdr_len) : nullptr, haveHdr ? hdr_len : 0};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });         // never mapped, as above
        u64 zl = 0;
        bfq_ubam_stats S{};
        RsSink sink;
        sink.extraWs = [&](u64 bound) { return bfq_ubam_held_need(c, bound, opts); };
        sink.put = [&](const u8 *d_text, u64 len) { zl = bfq_ubam_held(c, d_text, len, opts, F.at(0, 0), &S); };
        restore_core(c, dna, qs, hdr, haveHdr, sink, nullptr, nullptr, ordered ? &permz : nullptr);
        F.commit(&zl);
        if (out_len) *out_len = zl;
        if (stats) *stats = S;
    });
}

// ---- the grouped restore ------------------------------------------------------------------------------------------------
// where the texts of the groups go.  put(d_text, off, len, buf): the bytes of text buffer `buf` to offset `off` of the output,
// in the background where the destination allows it; wait(buf): the transfer that last read that buffer is over.
struct RsGroupSink {
    u64 cap = ~0ull;
    std::function<void(u64)> sized;                 // the output is known to reach this far (before the group is formatted)
    std::function<void(const u8 *, u64, u64, int)> put;
    std::function<void(int)> wait;
};

// arena bytes of one group beside the two text buffers: its decoded streams, then its compressed members and the codec's
// workspace or its index, whichever is larger (the eBWT-domain form: what the walk reserves)
static size_t rs_group_need(const RsGroup &r, const RsSrc &dna, bool haveHdr)
{
    const RsPlan P = r.plan(haveHdr);
    const size_t afterDecode = rs_index_bytes(P, false) + 4096;
    if (r.ebwt) {
        const size_t hdrPart = haveHdr ? P.rawH + r.g.hdr_len + bfq_codec_workspace(std::max(P.rawH, P.hdrMember)) + P.nameExtra + 8192 : 0;
        return r.g.raw_stream ? bfq_ebwt_decode_need(dna.h + r.g.dna_off, r.g.dna_len, r.g.qs_len, afterDecode + hdrPart + 4096, true) : afterDecode + hdrPart + 8192;
    }
    const size_t streams = (size_t)2 * r.g.raw_stream + r.g.raw_hdr + 3 * 320;
    const size_t decode = (size_t)r.g.dna_len + r.g.qs_len + r.g.hdr_len + 3 * 320 + bfq_codec_workspace(P.maxMember) + P.nameExtra;
    return streams + std::max(decode, afterDecode);
}

static void restore_grouped_core(bfq_ctx *c, const RsSrc &dna, const RsSrc &qs, const RsSrc &hdr, bool haveHdr, const std::vector<RsGroup> &G,
                                 u64 first, u64 count, const RsGroupSink &sink, uint64_t *out_len, uint64_t *n_reads)
{
    if (out_len) *out_len = 0;
    if (n_reads) *n_reads = 0;
    const u64 end = first + count;
    // one reservation, from the largest group of the range
    size_t needMax = 0, textMax = 0, worst = 0;
    u64 worstK = first;
    for (u64 k = first; k < end; k++) {
        const size_t need = rs_group_need(G[k], dna, haveHdr), text = (size_t)G[k].g.text_bound + 4096;
        needMax = std::max(needMax, need); textMax = std::max(textMax, text);
        if (need + 2 * text > worst) { worst = need + 2 * text; worstK = k; }
    }
    bfq_phase("alloc");
    try { c->reserve(needMax + 2 * textMax + (64u << 20)); }
    catch (const BfqError &e) {
        if (e.code != BFQ_E_NOMEM) throw;
        char b[160];
        snprintf(b, sizeof b, " (sized by group %llu, the largest of groups %llu..%llu)", (unsigned long long)worstK, (unsigned long long)first,
                 (unsigned long long)(end - 1));
        throw BfqError{BFQ_E_NOMEM, e.msg + b};
    }
    c->call.arenaHeld = true;
    u8 *text[2] = {c->alloc<u8>(textMax), c->alloc<u8>(textMax)};
    const size_t base = c->mark();
    // reads before the range: known where every earlier DNA member states them
    u64 readsBefore = 0;
    bool baseKnown = true;
    for (u64 k = 0; k < first; k++) { if (G[k].g.reads == ~0ull) baseKnown = false; else readsBefore += G[k].g.reads; }
    u64 off = 0, reads = 0;
    for (u64 k = first; k < end; k++) {
        const RsGroup &r = G[k];
        const int buf = (int)((k - first) & 1);
        const RsSrc gD{dna.h + r.g.dna_off, r.g.dna_len}, gQ{qs.h + r.g.qs_off, r.g.qs_len};
        const RsSrc gH{haveHdr ? hdr.h + r.g.hdr_off : nullptr, haveHdr ? r.g.hdr_len : 0};
        const u64 raw = r.g.raw_stream, rawH = r.g.raw_hdr;
        c->release(base);
        u8 *dD = nullptr, *dQ = nullptr, *dH = nullptr;
        if (r.ebwt) {
            EbwtLines e;
            bfq_phase("gpu");
            bfq_ebwt_decode_lines(c, gD.h, gD.len, gQ.h, gQ.len, nullptr, nullptr, ~0ull, nullptr, nullptr, 0, &e);
            if (!e.n) { e.dna = c->alloc<u8>(64); e.qs = c->alloc<u8>(64); }
            dD = e.dna; dQ = e.qs;
            if (haveHdr) {
                dH = c->alloc<u8>(rawH + 64);
                const size_t mk = c->mark();
                rs_decode(c, gH, c->alloc<u8>(gH.len + 64), dH, rawH);
                c->release(mk);
            }
        } else {
            c->zeroCounters();
            dD = c->alloc<u8>(raw + 64); dQ = c->alloc<u8>(raw + 64);
            if (haveHdr) dH = c->alloc<u8>(rawH + 64);
            const size_t mk = c->mark();
            u8 *zD = c->alloc<u8>(gD.len + 64), *zQ = c->alloc<u8>(gQ.len + 64), *zH = haveHdr ? c->alloc<u8>(gH.len + 64) : nullptr;
            bfq_phase("read_h2d");
            rs_decode(c, gD, zD, dD, raw);
            bfq_phase("gpu");
            rs_decode(c, gQ, zQ, dQ, raw);
            if (haveHdr) rs_decode(c, gH, zH, dH, rawH);
            c->release(mk);
        }
        bfq_phase("gpu");
        u64 nD = 0, nQ = 0, nH = 0;
        const u64 *endD = bfq_line_index(c, dD, raw, &nD);
        const u64 *endQ = bfq_line_index(c, dQ, raw, &nQ);
        const u64 *endH = haveHdr ? bfq_line_index(c, dH, rawH, &nH) : nullptr;
        const u64 N = std::min(nD, nQ);
        u64 *roff = c->alloc<u64>(N + 2), *recOff = c->alloc<u64>(N + 2);
        u64 *hStart = haveHdr ? c->alloc<u64>(N + 1) : nullptr;
        u32 *hLen = haveHdr ? c->alloc<u32>(N + 1) : nullptr, *sizes = c->alloc<u32>(N + 1);
        unsigned long long *d_err = (unsigned long long *)c->alloc<u64>(1);
        HIP_CHECK(hipMemsetAsync(d_err, 0xFF, 8, c->stream));
        KLAUNCH(c, K_RESTORE, (haveHdr ? 48.0 : 28.0) * (double)N, k_restore_index, bfq_grid(N ? N : 1, 256), 256, endD, nD, endQ, nQ, endH, nH,
                haveHdr ? 1 : 0, roff, hStart, hLen, sizes, d_err);
        bfq_exscan_u32(c, sizes, recOff, N, recOff + N);
        u64 err = RS_NONE, ol = 0;
        // the last byte of every stream of a group inside the archive: a line end, or a read was cut in two
        u8 last[3] = {'\n', '\n', '\n'};
        const bool inside = k + 1 < G.size();
        HIP_CHECK(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipMemcpyAsync(&ol, recOff + N, 8, hipMemcpyDeviceToHost, c->stream));
        if (inside && raw) {
            HIP_CHECK(hipMemcpyAsync(&last[0], dD + raw - 1, 1, hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipMemcpyAsync(&last[1], dQ + raw - 1, 1, hipMemcpyDeviceToHost, c->stream));
        }
        if (inside && haveHdr && rawH) HIP_CHECK(hipMemcpyAsync(&last[2], dH + rawH - 1, 1, hipMemcpyDeviceToHost, c->stream));
        c->sync();
        c->profCollect();
        for (int q = 0; q < 3; q++)
            if (last[q] != '\n') {
                char b[320];
                snprintf(b, sizeof b, "group %llu: its %s stream does not end with a line end: the members were not cut at reads; restore the archive in one piece",
                         (unsigned long long)k, q == 0 ? "DNA" : q == 1 ? "quality" : "header");
                throw BfqError{BFQ_E_ARG, b};
            }
        if (err != RS_NONE) {
            char w[96];
            if (baseKnown) snprintf(w, sizeof w, " (read %llu of group %llu)", (unsigned long long)(err >> 3), (unsigned long long)k);
            else snprintf(w, sizeof w, " of group %llu", (unsigned long long)k);
            throw rs_read_error(err, nD, nQ, nH, N, baseKnown ? readsBefore + reads : 0, w);
        }
        if (ol > (u64)G[k].g.text_bound) throw BfqError{BFQ_E_ARG, "damaged container (a group holds more reads than its DNA members state)"};
        if (off + ol > sink.cap) throw BfqError{BFQ_E_ARG, "output buffer smaller than the FASTQ text (see bfq_fastq_restore_groups: the sum of text_bound)"};
        if (sink.sized) sink.sized(off + ol);
        sink.wait(buf);                                          // the transfer of two groups ago read this buffer
        bfq_fastq_format_lines(c, dD, dQ, roff, dH, hStart, hLen, recOff, N, ol, text[buf]);
        sink.put(text[buf], off, ol, buf);
        off += ol; reads += N;
    }
    sink.wait(0); sink.wait(1);
    c->sync();
    c->profCollect();
    if (out_len) *out_len = off;
    if (n_reads) *n_reads = reads;
}

// the range [first, first + count) inside a plan of G groups; count ~0: to the end
static void rs_range(u64 G, u64 first, uint64_t *count)
{
    if (first >= G || (*count != ~0ull && (*count > G || first + *count > G))) {
        char b[200];
        snprintf(b, sizeof b, "groups %llu.. (count %lld) are outside the plan of %llu groups", (unsigned long long)first, (long long)*count, (unsigned long long)G);
        throw BfqError{BFQ_E_ARG, b};
    }
    if (*count == ~0ull) *count = G - first;
}

extern "C" int bfq_fastq_restore_grouped(bfq_ctx *c, const uint8_t *h_dna, uint64_t dna_len, const uint8_t *h_qs, uint64_t qs_len,
                                         const uint8_t *h_hdr, uint64_t hdr_len, uint64_t first, uint64_t count, uint8_t *h_out,
                                         uint64_t cap, uint64_t *out_len, uint64_t *n_reads)
{
    if (out_len) *out_len = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (!h_dna || !h_qs || (!h_out && cap)) throw BfqError{BFQ_E_ARG, "null argument"};
        const RsSrc dna{h_dna, dna_len}, qs{h_qs, qs_len}, hdr{h_hdr, hdr_len};
        const std::vector<RsGroup> G = rs_groups(dna, qs, hdr, h_hdr != nullptr);
        rs_range(G.size(), first, &count);
        // a pinned destination: direct DMA on the copy stream, behind the formatting kernel; each buffer has the event of the
        // copy that last read it
        const bool pinned = h_out && bfq_is_pinned(h_out);
        ScopedEvent formatted, copied[2];
        bool used[2] = {false, false};
        RsGroupSink sink;
        sink.cap = cap;
        sink.put = [&](const u8 *d_text, u64 off, u64 len, int buf) {
            bfq_phase("d2h_write");
            if (pinned) {
                if (!len) return;
                HIP_CHECK(hipEventRecord(formatted, c->stream));
                HIP_CHECK(hipStreamWaitEvent(c->copy(), formatted, 0));
                HIP_CHECK(hipMemcpyAsync(h_out + off, d_text, len, hipMemcpyDeviceToHost, c->copy()));
                HIP_CHECK(hipEventRecord(copied[buf], c->copy()));
                used[buf] = true;
            } else {
                bfq_download(c, h_out + off, d_text, len);      // pageable: in place when this returns (small pieces: queued on the stream)
                c->sync();
            }
        };
        sink.wait = [&](int buf) {
            if (used[buf]) HIP_CHECK(hipEventSynchronize(copied[buf]));
            used[buf] = false;
        };
        try { restore_grouped_core(c, dna, qs, hdr, h_hdr != nullptr, G, first, count, sink, out_len, n_reads); }
        catch (...) {
            if (c->copyStream) (void)hipStreamSynchronize(c->copyStream);   // the events go with this frame
            if (out_len) *out_len = 0;
            if (n_reads) *n_reads = 0;
            throw;
        }
    });
}

extern "C" int bfq_fastq_restore_grouped_fd(bfq_ctx *c, int dna_fd, uint64_t dna_len, int qs_fd, uint64_t qs_len, int hdr_fd, uint64_t hdr_len,
                                            uint64_t first, uint64_t count, int out_fd, uint64_t *out_len, uint64_t *n_reads)
{
    if (out_len) *out_len = 0;
    if (n_reads) *n_reads = 0;
    return guarded(c, [&] {
        if (dna_fd < 0 || qs_fd < 0 || out_fd < 0) throw BfqError{BFQ_E_ARG, "bad file descriptor"};
        const bool haveHdr = hdr_fd >= 0;
        RsMap mD, mQ, mH;
        const RsSrc dna{mD.open(dna_fd, dna_len), dna_len}, qs{mQ.open(qs_fd, qs_len), qs_len};
        const RsSrc hdr{haveHdr ? mH.open(hdr_fd, hdr_len) : nullptr, haveHdr ? hdr_len : 0};
        OutFiles F(out_fd, [c] { bfq_write_wait(c); });
        const std::vector<RsGroup> G = rs_groups(dna, qs, hdr, haveHdr);
        rs_range(G.size(), first, &count);
        u64 bound = 0, certain = 0;
        for (u64 k = first; k < first + count; k++) { bound += G[k].g.text_bound; certain += 2 * G[k].g.raw_stream; }
        F.open(0, bound + 4096, certain);
        c->call.writeHint = (size_t)bound;
        RsGroupSink sink;
        sink.sized = [&](u64 len) { F.extend(0, len); };
        // the background writers know one wait, for everything queued: it is made before a text is queued, so that the
        // text before it travels beside the decoding, the index and the formatting of this one
        sink.put = [&](const u8 *d_text, u64 off, u64 len, int) {
            bfq_phase("d2h_write");
            bfq_write_wait(c);
            bfq_write_async(c, F.at(0, off), d_text, len);
        };
        sink.wait = [&](int) {};
        uint64_t ol = 0, nr = 0;
        restore_grouped_core(c, dna, qs, hdr, haveHdr, G, first, count, sink, &ol, &nr);
        bfq_phase("d2h_write");
        F.commit(&ol);
        if (out_len) *out_len = ol;
        if (n_reads) *n_reads = nr;
    });
}
