// k_names.hip -- read names as tokens: the opt-in "BFQNAME1" container of the stream codec (include/bfqzip_hip.h states the
// format; tests/names_model.py is the statement the kernels are compared with, byte for byte).  A line is cut into runs of
// digits and runs of everything else, every token is coded against the token at the same place of the line before -- the
// same bytes (SAME, run-length coded), that number + 1 (INC), that number + d (DELTA), or spelled out (TEXT) -- and the
// three byte streams this leaves (operations, number payloads, text payloads) and a per-group index go through the general
// codec as four members.  Groups of 256 lines stand alone: the first line of a group is coded against the empty line.
//
//   k_nm_sizes  : a lane per line walks its line and the one before, token by token with two cursors, and sizes the line's
//                 shares of the three streams; bfq_exscan_u32 gives every line its offsets
//   k_nm_write  : the same walk, writing; the lane of a group's first line writes the group's index entry from the scanned
//                 offsets at the group boundaries
//   k_nm_decode : a lane per group, lines in order; it re-tokenises the line it has just written to find the tokens the
//                 next one refers to.  Every read and write is checked against the group's stated shares, so a container
//                 that parses but lies is refused and never leaves them.
// Byte-wise integer work on a few dozen bytes per line.
#include <string.h>
#include <stdio.h>
#include "bfq_internal.h"
#include "bfq_device.h"

#define NM_R 256u                                       // lines per group
#define NM_MAX_LINE 65535u
#define NM_HDR 64u
#define NM_LIMIT 1000000000000000000ull                 // numeric tokens are below 10^18
#define NM_OP_END 0u
#define NM_OP_INC 2u
#define NM_OP_DELTA 3u
#define NM_OP_TEXT 4u
#define NM_OP_SAME 15u                                  // + k, k = 1 .. 240

__device__ __forceinline__ bool nm_digit(u8 ch) { return (u8)(ch - (u8)'0') < 10u; }
// end of the token that starts at p < e
__device__ __forceinline__ u64 nm_tok_end(const u8 *t, u64 p, u64 e)
{
    const bool d = nm_digit(t[p]);
    u64 q = p + 1;
    while (q < e && nm_digit(t[q]) == d) q++;
    return q;
}
__device__ __forceinline__ bool nm_numeric(const u8 *t, u64 b, u64 e)
{
    return nm_digit(t[b]) && e - b <= 18 && (e - b == 1 || t[b] != (u8)'0');
}
__device__ __forceinline__ u64 nm_value(const u8 *t, u64 b, u64 e)
{
    u64 v = 0;
    for (; b < e; b++) v = v * 10 + (u64)(t[b] - (u8)'0');
    return v;
}

// where a line's shares go; W = false only counts
template <bool W> struct NmOut {
    u8 *ops, *num, *text;
    u32 no = 0, nn = 0, nt = 0;
    __device__ __forceinline__ void op(u32 b) { if (W) ops[no] = (u8)b; no++; }
    __device__ __forceinline__ void same(u32 run)
    {
        for (; run > 240u; run -= 240u) op(NM_OP_SAME + 240u);
        if (run) op(NM_OP_SAME + run);
    }
    __device__ __forceinline__ void lebNum(u64 z)
    {
        for (; z >= 128u; z >>= 7) { if (W) num[nn] = (u8)(z | 128u); nn++; }
        if (W) num[nn] = (u8)z;
        nn++;
    }
    __device__ __forceinline__ void bytes(const u8 *__restrict__ src, u64 len)                      // LEB128 of the length, then the bytes
    {
        u64 z = len;
        for (; z >= 128u; z >>= 7) { if (W) text[nt] = (u8)(z | 128u); nt++; }
        if (W) text[nt] = (u8)z;
        nt++;
        if (W) for (u64 j = 0; j < len; j++) text[nt + j] = src[j];
        nt += (u32)len;
    }
};

// the line [s, e) against the line [ps, pe) (ps == pe: the empty line)
template <bool W> __device__ __forceinline__ void nm_encode_line(const u8 *__restrict__ in, u64 s, u64 e, u64 ps, u64 pe, NmOut<W> &o)
{
    u64 p = s, q = ps;
    u32 run = 0;
    while (p < e) {
        const u64 te = nm_tok_end(in, p, e);
        const bool have = q < pe;
        const u64 qe = have ? nm_tok_end(in, q, pe) : q;
        bool same = have && qe - q == te - p;
        for (u64 j = 0; same && j < te - p; j++) same = in[p + j] == in[q + j];
        if (same) run++;
        else {
            o.same(run);
            run = 0;
            if (nm_numeric(in, p, te)) {
                const u64 v = nm_value(in, p, te), u = (have && nm_numeric(in, q, qe)) ? nm_value(in, q, qe) : 0;
                if (v == u + 1) o.op(NM_OP_INC);
                else { o.op(NM_OP_DELTA); o.lebNum(v >= u ? 2 * (v - u) : 2 * (u - v) - 1); }
            } else { o.op(NM_OP_TEXT); o.bytes(in + p, te - p); }
        }
        p = te; q = qe;
    }
    o.same(run);
    o.op(NM_OP_END);
}

__global__ __launch_bounds__(256) void k_nm_sizes(const u8 *__restrict__ in, const u64 *__restrict__ lineEnd, u64 nl, u32 *__restrict__ so,
                                                  u32 *__restrict__ sn, u32 *__restrict__ st, u32 *__restrict__ tooLong)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += (u64)gridDim.x * blockDim.x) {
        const u64 s = i ? lineEnd[i - 1] + 1 : 0, e = lineEnd[i];
        NmOut<false> o;
        if (e - s > NM_MAX_LINE) atomicAdd(tooLong, 1u);          // the stream is not eligible: nothing of this is used
        else {
            const u64 ps = (i % NM_R) ? (i >= 2 ? lineEnd[i - 2] + 1 : 0) : s, pe = (i % NM_R) ? s - 1 : s;
            nm_encode_line<false>(in, s, e, ps, pe, o);
        }
        so[i] = o.no; sn[i] = o.nn; st[i] = o.nt;
    }
}
// offO / offN / offT: nl + 1 entries each (the totals last); idx: four u32 per group
__global__ __launch_bounds__(256) void k_nm_write(const u8 *__restrict__ in, const u64 *__restrict__ lineEnd, u64 nl, const u64 *__restrict__ offO,
                                                  const u64 *__restrict__ offN, const u64 *__restrict__ offT, u8 *__restrict__ ops,
                                                  u8 *__restrict__ num, u8 *__restrict__ text, u32 *__restrict__ idx)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += (u64)gridDim.x * blockDim.x) {
        const u64 s = i ? lineEnd[i - 1] + 1 : 0, e = lineEnd[i];
        const u64 ps = (i % NM_R) ? (i >= 2 ? lineEnd[i - 2] + 1 : 0) : s, pe = (i % NM_R) ? s - 1 : s;
        NmOut<true> o;
        o.ops = ops + offO[i]; o.num = num + offN[i]; o.text = text + offT[i];
        nm_encode_line<true>(in, s, e, ps, pe, o);
        if (i % NM_R == 0) {
            const u64 i1 = (i + NM_R < nl) ? i + NM_R : nl;
            u32 *g = idx + 4 * (i / NM_R);
            g[0] = (u32)(offO[i1] - offO[i]); g[1] = (u32)(offN[i1] - offN[i]); g[2] = (u32)(offT[i1] - offT[i]);
            g[3] = (u32)(lineEnd[i1 - 1] + 1 - s);
        }
    }
}

// LEB128 of at most nine bytes from [*p, e); false: the share ends first, or a tenth byte would follow
__device__ __forceinline__ bool nm_leb(const u8 *__restrict__ t, u64 *p, u64 e, u64 *out)
{
    u64 z = 0;
    for (u32 k = 0; k < 9; k++) {
        if (*p >= e) return false;
        const u8 b = t[(*p)++];
        z |= (u64)(b & 127u) << (7u * k);
        if (!(b & 128u)) { *out = z; return true; }
    }
    return false;
}

// goff: four u64 per group, + the four totals: where the group's shares of ops / num / text / the raw bytes start
__global__ __launch_bounds__(256) void k_nm_decode(const u8 *__restrict__ ops, const u8 *__restrict__ num, const u8 *__restrict__ text,
                                                   const u64 *__restrict__ goff, u64 ngroups, u64 nl, u8 *out, u32 *__restrict__ bad)
{
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (u64)gridDim.x * blockDim.x) {
        u64 po = goff[4 * g], pn = goff[4 * g + 1], pt = goff[4 * g + 2], w = goff[4 * g + 3];
        const u64 eo = goff[4 * g + 4], en = goff[4 * g + 5], et = goff[4 * g + 6], ew = goff[4 * g + 7];
        const u64 want = (nl - g * NM_R < NM_R) ? nl - g * NM_R : NM_R;
        u64 prevS = w, prevE = w;                                  // the line before: out[prevS, prevE)
        bool ok = true;
        for (u64 line = 0; line < want && ok; line++) {
            const u64 ls = w;
            u64 q = prevS;
            for (;;) {
                if (po >= eo) { ok = false; break; }
                const u32 op = ops[po++];
                if (op == NM_OP_END) break;
                const bool have = q < prevE;
                const u64 qe = have ? nm_tok_end(out, q, prevE) : q;
                if (op > NM_OP_SAME) {                             // k tokens of the line before, as they are
                    u64 a = q;
                    for (u32 k = op - NM_OP_SAME; k; k--) {
                        if (a >= prevE) { ok = false; break; }
                        const u64 ae = nm_tok_end(out, a, prevE);
                        if (ae - a > ew - w) { ok = false; break; }
                        for (u64 j = a; j < ae; j++) out[w++] = out[j];
                        a = ae;
                    }
                    if (!ok) break;
                    q = a;
                    continue;
                }
                if (op == NM_OP_INC || op == NM_OP_DELTA) {
                    const u64 u = (have && nm_numeric(out, q, qe)) ? nm_value(out, q, qe) : 0;
                    u64 v = u + 1;
                    if (op == NM_OP_DELTA) {
                        u64 z = 0;
                        if (!nm_leb(num, &pn, en, &z)) { ok = false; break; }
                        const u64 m = (z >> 1) + (z & 1u);             // |d|
                        if ((z & 1u) ? m > u : m >= NM_LIMIT) { ok = false; break; }
                        v = (z & 1u) ? u - m : u + m;
                    }
                    if (v >= NM_LIMIT) { ok = false; break; }
                    u32 nd = 1;
                    for (u64 t = v; t >= 10; t /= 10) nd++;
                    if (nd > ew - w) { ok = false; break; }
                    for (u32 k = nd; k--; v /= 10) out[w + k] = (u8)('0' + (u32)(v % 10));
                    w += nd;
                } else if (op == NM_OP_TEXT) {
                    u64 len = 0;
                    if (!nm_leb(text, &pt, et, &len) || len == 0 || len > et - pt || len > ew - w) { ok = false; break; }
                    for (u64 j = 0; j < len; j++) out[w++] = text[pt++];
                } else { ok = false; break; }
                q = qe;
            }
            if (!ok || w >= ew || w - ls > NM_MAX_LINE) { ok = false; break; }
            prevS = ls; prevE = w;
            out[w++] = 10;
        }
        if (!ok || po != eo || pn != en || pt != et || w != ew) atomicAdd(bad, 1u);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------
static void nm_put32(u8 *p, u32 v) { memcpy(p, &v, 4); }
static void nm_put64(u8 *p, u64 v) { memcpy(p, &v, 8); }
static u32 nm_get32(const u8 *p) { u32 v; memcpy(&v, p, 4); return v; }
static u64 nm_get64(const u8 *p) { u64 v; memcpy(&v, p, 8); return v; }
static bool nm_magic(const u8 *h_in, u64 len) { return len >= 8 && !memcmp(h_in, "BFQNAME1", 8); }

// The header and the first bytes of the four members, on the host: lengths and raw lengths of the members.  Every field is
// checked against the others before anything is sized by it.  deep: the members' own headers are parsed too (the decoder).
struct NmHeader { u64 raw, nl, ng, mlen[4], mraw[4]; };
static void nm_parse(const u8 *h_in, u64 len, NmHeader &H, bool deep)
{
    const BfqError bad{BFQ_E_ARG, "damaged BFQNAME1 stream"};
    if (len < NM_HDR || !nm_magic(h_in, len)) throw bad;
    H.raw = nm_get64(h_in + 8); H.nl = nm_get64(h_in + 24);
    if (nm_get32(h_in + 16) != NM_R || nm_get32(h_in + 20) != 0 || H.nl == 0 || H.nl > H.raw || H.raw > (1ull << 46)) throw bad;
    H.ng = (H.nl + NM_R - 1) / NM_R;
    u64 pos = NM_HDR;
    for (int k = 0; k < 4; k++) {
        H.mlen[k] = nm_get64(h_in + 32 + 8 * k);
        if (H.mlen[k] > len - pos || H.mlen[k] < 32) throw bad;
        const u8 *m = h_in + pos;
        // members are what bfq_stream_compress writes: their raw length follows the magic
        if (memcmp(m, "BFQRANS2", 8) && memcmp(m, "BFQLINE1", 8) && memcmp(m, "BFQDNAC1", 8)) throw bad;
        H.mraw[k] = nm_get64(m + 8);
        if (deep) {
            u64 ml = 0;
            try { ml = bfq_codec_member_len(m, H.mlen[k]); } catch (const BfqError &) { throw bad; }
            if (ml != H.mlen[k]) throw bad;
        }
        pos += H.mlen[k];
    }
    if (pos != len) throw bad;
    // what the encoder can produce at most: an operation per token and line, nine payload bytes per number (a number and
    // what ends it are two raw bytes), a length byte per text byte
    if (H.mraw[0] != 16 * H.ng || H.mraw[1] > 2 * H.raw || H.mraw[2] > 5 * H.raw || H.mraw[3] > 2 * H.raw) throw bad;
}

u64 bfq_names_member_len(const u8 *h_in, u64 len)
{
    const BfqError bad{BFQ_E_ARG, "damaged BFQNAME1 stream"};
    if (len < NM_HDR || !nm_magic(h_in, len)) throw bad;
    u64 total = NM_HDR;
    for (int k = 0; k < 4; k++) {
        const u64 m = nm_get64(h_in + 32 + 8 * k);
        if (m > len - total) throw bad;
        total += m;
    }
    NmHeader H;
    nm_parse(h_in, total, H, false);
    return total;
}

// device bytes a decode of this member takes beside the codec's workspace for its largest inner member (*maxInner)
u64 bfq_names_decode_extra(const u8 *h_in, u64 len, u64 *maxInner)
{
    NmHeader H;
    nm_parse(h_in, len, H, false);
    u64 sum = 0;
    for (int k = 0; k < 4; k++) { sum += H.mraw[k] + 512; if (maxInner && H.mraw[k] > *maxInner) *maxInner = H.mraw[k]; }
    return sum + 32 * (H.ng + 2) + 4096;
}

u64 bfq_names_decompress_device(bfq_ctx *c, const u8 *h_in, const u8 *d_in, u64 len, u8 *d_out, u64 cap)
{
    const BfqError bad{BFQ_E_ARG, "damaged BFQNAME1 stream"};
    NmHeader H;
    nm_parse(h_in, len, H, true);
    if (H.raw > cap) throw BfqError{BFQ_E_ARG, "output buffer too small for the raw stream"};
    const size_t mk = c->mark();
    u8 *d_m[4];
    u64 pos = NM_HDR;
    for (int k = 0; k < 4; k++) {
        d_m[k] = c->alloc<u8>(H.mraw[k] + 16);
        try {
            if (bfq_codec_decompress_device(c, h_in + pos, d_in + pos, H.mlen[k], d_m[k], H.mraw[k]) != H.mraw[k]) throw bad;
        } catch (const BfqError &e) {
            if (e.code != BFQ_E_ARG) throw;
            throw BfqError{BFQ_E_ARG, "damaged BFQNAME1 stream (member " + std::to_string(k) + ": " + e.msg + ")"};
        }
        pos += H.mlen[k];
    }
    // the index on the host: where every group's shares start; the columns must add up to the members and the raw length
    std::vector<u32> idx(4 * H.ng);
    HIP_CHECK(hipMemcpyAsync(idx.data(), d_m[0], 16 * H.ng, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    std::vector<u64> goff(4 * (H.ng + 1));
    u64 acc[4] = {0, 0, 0, 0};
    for (u64 g = 0; g < H.ng; g++)
        for (int k = 0; k < 4; k++) { goff[4 * g + k] = acc[k]; acc[k] += idx[4 * g + k]; }
    for (int k = 0; k < 4; k++) goff[4 * H.ng + k] = acc[k];
    if (acc[0] != H.mraw[1] || acc[1] != H.mraw[2] || acc[2] != H.mraw[3] || acc[3] != H.raw) throw bad;
    u64 *d_goff = c->alloc<u64>(goff.size());
    u32 *d_bad = c->alloc<u32>(1);
    HIP_CHECK(hipMemcpyAsync(d_goff, goff.data(), 8 * goff.size(), hipMemcpyHostToDevice, c->stream));
    HIP_CHECK(hipMemsetAsync(d_bad, 0, 4, c->stream));
    KLAUNCH(c, K_CODEC, 2.0 * (double)H.raw + (double)(acc[0] + acc[1] + acc[2]), k_nm_decode, bfq_grid(H.ng, 256), 256, (const u8 *)d_m[1],
            (const u8 *)d_m[2], (const u8 *)d_m[3], (const u64 *)d_goff, H.ng, H.nl, d_out, d_bad);
    u32 nbad = 0;
    HIP_CHECK(hipMemcpyAsync(&nbad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    c->release(mk);
    if (nbad) throw bad;
    return H.raw;
}

// ---- the encoder: sized first (the arena may have to grow before anything is written), then written and coded
bool bfq_names_size(bfq_ctx *c, const u8 *d_in, u64 n, NamesSized *S)
{
    *S = NamesSized{};
    if (!n) return false;
    u8 last = 0;
    HIP_CHECK(hipMemcpyAsync(&last, d_in + n - 1, 1, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (last != 10) return false;
    u64 nl = 0;
    S->lineEnd = bfq_line_index(c, d_in, n, &nl);
    S->nl = nl;
    u32 *so = c->alloc<u32>(nl), *sn = c->alloc<u32>(nl), *st = c->alloc<u32>(nl), *d_long = c->alloc<u32>(1);
    S->offO = c->alloc<u64>(nl + 1); S->offN = c->alloc<u64>(nl + 1); S->offT = c->alloc<u64>(nl + 1);
    HIP_CHECK(hipMemsetAsync(d_long, 0, 4, c->stream));
    KLAUNCH(c, K_CODEC, 2.0 * (double)n + 20.0 * (double)nl, k_nm_sizes, bfq_grid(nl, 256), 256, d_in, S->lineEnd, nl, so, sn, st, d_long);
    bfq_exscan_u32(c, so, S->offO, nl, S->offO + nl);
    bfq_exscan_u32(c, sn, S->offN, nl, S->offN + nl);
    bfq_exscan_u32(c, st, S->offT, nl, S->offT + nl);
    u32 tooLong = 0;
    HIP_CHECK(hipMemcpyAsync(&tooLong, d_long, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&S->total[0], S->offO + nl, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&S->total[1], S->offN + nl, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_CHECK(hipMemcpyAsync(&S->total[2], S->offT + nl, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    S->eligible = tooLong == 0;
    return S->eligible;
}

// arena bytes bfq_names_sized_bytes() are taken by bfq_names_size(), bfq_names_rest_bytes() by bfq_names_finish()
u64 bfq_names_sized_bytes(u64 n, u64 nl) { return 48 * (nl + 64) + 32 * (n / 4096 + 64) + (1u << 20); }
u64 bfq_names_rest_bytes(u64 n, const NamesSized &S)
{
    if (!S.eligible) return bfq_codec_workspace(n);
    const u64 ng = (S.nl + NM_R - 1) / NM_R;
    u64 streams = 16 * ng + 1024, z = NM_HDR + bfq_codec_bound(16 * ng) + 1024, largest = n > 16 * ng ? n : 16 * ng;
    for (int k = 0; k < 3; k++) { streams += S.total[k] + 272; z += bfq_codec_bound(S.total[k]); if (S.total[k] > largest) largest = S.total[k]; }
    return streams + z + bfq_codec_workspace(largest);
}

u64 bfq_names_finish(bfq_ctx *c, const u8 *d_in, u64 n, const NamesSized &S, u32 flags, u8 *d_out, u64 cap)
{
    const bool always = (flags & 1u) != 0;
    if (!S.eligible) return bfq_codec_compress_device(c, d_in, n, d_out, cap);
    const size_t mk = c->mark();
    const u64 general = always ? 0 : bfq_codec_compress_device(c, d_in, n, d_out, cap);
    const u64 nl = S.nl, ng = (nl + NM_R - 1) / NM_R;
    const u64 mraw[4] = {16 * ng, S.total[0], S.total[1], S.total[2]};
    u8 *d_m[4];
    u64 zcap = NM_HDR + 16;
    for (int k = 0; k < 4; k++) { d_m[k] = c->alloc<u8>(mraw[k] + 16); zcap += bfq_codec_bound(mraw[k]); }
    KLAUNCH(c, K_CODEC, 2.0 * (double)n + 44.0 * (double)nl + (double)(mraw[1] + mraw[2] + mraw[3]), k_nm_write, bfq_grid(nl, 256), 256, d_in, S.lineEnd, nl,
            (const u64 *)S.offO, (const u64 *)S.offN, (const u64 *)S.offT, d_m[1], d_m[2], d_m[3], (u32 *)d_m[0]);
    u8 *d_z = c->alloc<u8>(zcap);
    u8 h[NM_HDR];
    memcpy(h, "BFQNAME1", 8); nm_put64(h + 8, n); nm_put32(h + 16, NM_R); nm_put32(h + 20, 0); nm_put64(h + 24, nl);
    u64 pos = NM_HDR;
    for (int k = 0; k < 4; k++) {
        const u64 got = bfq_codec_compress_device(c, d_m[k], mraw[k], d_z + pos, bfq_codec_bound(mraw[k]));
        nm_put64(h + 32 + 8 * k, got);
        pos += got;
        if (!always && pos >= general) break;                      // already no shorter than the general container
    }
    u64 got = general;
    if (always || pos < general) {
        if (pos > cap) throw BfqError{BFQ_E_ARG, "output buffer too small for the compressed stream"};
        HIP_CHECK(hipMemcpyAsync(d_z, h, NM_HDR, hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipMemcpyAsync(d_out, d_z, pos, hipMemcpyDeviceToDevice, c->stream));
        c->sync();                                                 // h is a stack variable
        got = pos;
    }
    c->release(mk);
    return got;
}
