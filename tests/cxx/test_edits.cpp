// test_edits.cpp -- the host forms of the BFQEDIT1 container (include/bfqzip_hip.h; bfq_edits.h, bfq_edits_host.cpp) as a
// program of its own: encode and decode over the edit counts at which segments begin and end and over gaps of every width,
// a bit-by-bit restatement of the gap layout, every refusal with its first offending edit, and the two text forms on small
// texts.  Buffers are heap blocks of the exact size, so that a sanitizer sees any byte read or written beside them.
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_edits.h"

static int g_fail = 0;
#define CHECK(x) do { if (!(x)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); g_fail++; } } while (0)

static u64 rng_state = 0x9E3779B97F4A7C15ull;
static u64 rnd() { rng_state = bfq_mix64(rng_state); return rng_state; }

struct Heap {                                                     // an exact-size block
    u8 *p; u64 n;
    explicit Heap(u64 n) : p((u8 *)malloc(n ? n : 1)), n(n) {}
    Heap(const Heap &) = delete;
    ~Heap() { free(p); }
};

// E edits with gaps below 2^bits
static void make_edits(u64 E, u32 bits, std::vector<u64> &pos, std::vector<u8> &byte, u64 *T)
{
    pos.clear(); byte.clear();
    u64 g = rnd() % 3;
    for (u64 k = 0; k < E; k++) {
        if (k) g += 1 + (bits ? rnd() >> (64 - bits) : 0);
        pos.push_back(g);
        byte.push_back((u8)(33 + rnd() % 94));
    }
    *T = E ? g + 1 + rnd() % 3 : rnd() % 5;
}

static u64 gap_bitwise(const u8 *words, u64 j, u32 w)
{
    u64 v = 0;
    for (u32 t = 0; t < w; t++) {
        const u64 b = j * w + t;
        u64 word;
        memcpy(&word, words + 8 * (b / 64), 8);
        v |= ((word >> (b % 64)) & 1) << t;
    }
    return v;
}

static void round_trip(u64 E, u32 bits)
{
    std::vector<u64> pos;
    std::vector<u8> byte;
    u64 T;
    make_edits(E, bits, pos, byte, &T);
    const u64 bound = bfq_edits_bound_of(E, T);
    Heap big(bound);
    u64 len = 0;
    CHECK(bfq_edits_encode_host(pos.data(), byte.data(), E, 7, T, 11, 13, big.p, bound, &len) == BFQ_OK);
    CHECK(len <= bound && len >= BFQ_EDIT_HDR);
    Heap z(len);                                                  // exactly the member
    u64 len2 = 0;
    CHECK(bfq_edits_encode_host(pos.data(), byte.data(), E, 7, T, 11, 13, z.p, len, &len2) == BFQ_OK && len2 == len);
    CHECK(!memcmp(z.p, big.p, len));
    if (len) { Heap small(len - 1); CHECK(bfq_edits_encode_host(pos.data(), byte.data(), E, 7, T, 11, 13, small.p, len - 1, &len2) == BFQ_E_ARG && len2 == 0); }
    BfqEditMember M;
    CHECK(bfq_edits_member(z.p, len, &M, nullptr) == nullptr && M.bytes() == len && M.E == E && M.T == T && M.N == 7 && M.shape == 11 && M.targetSum == 13);
    // the layout, bit by bit
    u64 wo = 0;
    for (u64 s = 0; s < M.nseg; s++) {
        const u64 c = bfq_edit_seg_count(E, s);
        const u32 w = z.p[M.offW + s];
        u64 mx = 0;
        for (u64 j = 0; j + 1 < c; j++) {
            const u64 g = pos[s * BFQ_EDIT_SEG + j + 1] - pos[s * BFQ_EDIT_SEG + j] - 1;
            mx = g > mx ? g : mx;
            CHECK(gap_bitwise(z.p + M.offGaps + 8 * wo, j, w) == g);
        }
        u32 wl = 0;
        for (u64 x = mx; x; x >>= 1) wl++;
        CHECK(w == wl);
        CHECK(bfq_edit_ld64(z.p + M.offFirst + 8 * s) == pos[s * BFQ_EDIT_SEG]);
        wo += bfq_edit_seg_words(c, w);
    }
    Heap op(8 * E), ob(E);
    u64 bad = 5;
    const char *why = "x";
    BfqEditMember D;
    CHECK(bfq_edits_decode_host(z.p, len, (u64 *)op.p, ob.p, E, &D, &bad, &why) == BFQ_OK && bad == BFQ_EDIT_NOPOS && why == nullptr);
    CHECK(D.E == E && (!E || (!memcmp(op.p, pos.data(), 8 * E) && !memcmp(ob.p, byte.data(), E))));
    if (E) { Heap sp(8 * (E - 1)), sb(E - 1); CHECK(bfq_edits_decode_host(z.p, len, (u64 *)sp.p, sb.p, E - 1, nullptr, nullptr, nullptr) == BFQ_E_ARG); }
}

// decode must refuse z with first_bad = want and leave its outputs alone
static void refused(const std::vector<u8> &zv, u64 want, const char *what)
{
    Heap z(zv.size());
    if (zv.size()) memcpy(z.p, zv.data(), zv.size());
    const u64 room = 4096;
    Heap op(8 * room), ob(room);
    memset(op.p, 0xA5, 8 * room); memset(ob.p, 0xA5, room);
    u64 bad = 5;
    const int rc = bfq_edits_decode_host(z.p, zv.size(), (u64 *)op.p, ob.p, room, nullptr, &bad, nullptr);
    if (rc != BFQ_E_ARG || bad != want) { printf("FAIL refusal '%s': rc %d first_bad %llu (want %llu)\n", what, rc, bad, want); g_fail++; }
    for (u64 i = 0; i < 8 * room; i++) if (op.p[i] != 0xA5) { CHECK(!"positions written on a refusal"); break; }
    for (u64 i = 0; i < room; i++) if (ob.p[i] != 0xA5) { CHECK(!"bytes written on a refusal"); break; }
}

static std::vector<u8> member_of(const std::vector<u64> &pos, const std::vector<u8> &byte, u64 T)
{
    std::vector<u8> z(bfq_edits_bound_of(pos.size(), T));
    u64 len = 0;
    CHECK(bfq_edits_encode_host(pos.data(), byte.data(), pos.size(), 3, T, 0, 0, z.data(), z.size(), &len) == BFQ_OK);
    z.resize(len);
    return z;
}

static void refusals()
{
    std::vector<u64> pos;
    std::vector<u8> byte;
    u64 T;
    make_edits(2500, 9, pos, byte, &T);
    const std::vector<u8> good = member_of(pos, byte, T);
    BfqEditMember M;
    CHECK(bfq_edits_member(good.data(), good.size(), &M, nullptr) == nullptr);
    std::vector<u8> z;
    z = good; z[0] = 'X'; refused(z, BFQ_EDIT_NOPOS, "magic");
    z = good; z[32] = 0; z[33] = 2; refused(z, BFQ_EDIT_NOPOS, "S");
    z = good; z[36] = 1; refused(z, BFQ_EDIT_NOPOS, "flags");
    z = good; z.push_back(0); refused(z, BFQ_EDIT_NOPOS, "a byte too many");
    z = good; z.pop_back(); refused(z, BFQ_EDIT_NOPOS, "a byte too few");
    z = good; z.resize(40); refused(z, BFQ_EDIT_NOPOS, "cut inside the header");
    z = good; z[M.offW + M.nseg] = 1; refused(z, BFQ_EDIT_NOPOS, "table padding");
    z = good; z[M.offBytes + M.E] = 1; refused(z, BFQ_EDIT_NOPOS, "bytes padding");
    z = good; z[M.offW + 1] = 57; refused(z, 1024, "width above 56");
    z = good; z[M.offBytes + 1500] = 32; refused(z, 1500, "byte 32");
    z = good; z[M.offBytes + 7] = 127; refused(z, 7, "byte 127");
    z = good; z[M.offBytes + 2499] = 10; z[M.offBytes + 30] = 10; refused(z, 30, "two bad bytes: the first");
    { u64 t = pos[2000]; z = good; memcpy(z.data() + 16, &t, 8); refused(z, 2000, "position >= T"); }
    { u64 f = pos[1023]; z = good; memcpy(z.data() + M.offFirst + 8, &f, 8); refused(z, 1024, "first not above the edit before it"); }
    // a width that is not canonical: every gap of segment 0 written one bit wider than needed
    {
        std::vector<u64> p2(pos.begin(), pos.begin() + 100);
        std::vector<u8> b2(byte.begin(), byte.begin() + 100);
        const std::vector<u8> g2 = member_of(p2, b2, T);
        BfqEditMember M2;
        CHECK(bfq_edits_member(g2.data(), g2.size(), &M2, nullptr) == nullptr);
        const u32 w = g2[M2.offW], w2 = w + 1;
        const u64 nw2 = bfq_edit_seg_words(100, w2);
        std::vector<u8> wide(BFQ_EDIT_HDR + 8 + 8 + 8 * nw2 + 104, 0);
        memcpy(wide.data(), g2.data(), BFQ_EDIT_HDR + 8);
        wide[M2.offW] = (u8)w2;
        for (u64 j = 0; j < 99; j++) {
            const u64 g = p2[j + 1] - p2[j] - 1, bit = j * w2;
            for (u32 t = 0; t < w2; t++)
                if (g >> t & 1) wide[M2.offGaps + (bit + t) / 8] |= (u8)(1u << ((bit + t) % 8));
        }
        memcpy(wide.data() + M2.offGaps + 8 * nw2, b2.data(), 100);
        const u64 payload = wide.size() - BFQ_EDIT_HDR;
        memcpy(wide.data() + 56, &payload, 8);
        refused(wide, 0, "a width that is not canonical");
        // padding bits of the segment's last word
        if ((99 * w) & 63) { z = g2; z[M2.offBytes - 1] |= 0x80; refused(z, 0, "gap padding bits"); }
    }
}

static void texts()
{
    // read lengths around the 8-byte word, CRLF, an empty read, no final newline
    std::string a, b;
    std::vector<u64> want;
    u64 g = 0;
    const u32 lens[] = {0, 1, 7, 8, 9, 127, 128, 129, 300};
    for (u32 i = 0; i < 9; i++) {
        std::string s(lens[i], 'A'), t;
        for (u32 j = 0; j < lens[i]; j++) s[j] = "ACGTN"[rnd() % 5];
        t = s;
        for (u32 j = 0; j < lens[i]; j++)
            if (j == 0 || j + 1 == lens[i] || rnd() % 9 == 0) { t[j] = t[j] == 'A' ? 'C' : 'A'; want.push_back(g + j); }
        g += lens[i];
        const std::string q(lens[i], 'I'), eol = i % 2 ? "\r\n" : "\n";
        a += "@r" + eol + s + eol + "+" + eol + q + (i == 8 ? "" : eol);
        b += "@" + eol + t + eol + "+" + eol + q + eol;
    }
    Heap ha(a.size()), hb(b.size());
    memcpy(ha.p, a.data(), a.size()); memcpy(hb.p, b.data(), b.size());
    const u64 cap = bfq_edits_bound_of(want.size(), g);
    Heap z(cap);
    uint64_t zl = 0;
    bfq_edit_stats st;
    CHECK(bfq_fastq_edits_host(ha.p, a.size(), hb.p, b.size(), z.p, cap, &zl, &st) == BFQ_OK);
    CHECK(st.edits == want.size() && st.reads == 9 && st.bases == g && st.bytes == zl && st.reads_touched == 8);
    Heap ze(zl);
    memcpy(ze.p, z.p, zl);
    Heap dp(8 * want.size()), db(want.size());
    CHECK(bfq_edits_decode_host(ze.p, zl, (u64 *)dp.p, db.p, want.size(), nullptr, nullptr, nullptr) == BFQ_OK);
    CHECK(!memcmp(dp.p, want.data(), 8 * want.size()));
    Heap out(b.size());
    uint64_t ol = 0;
    CHECK(bfq_fastq_unedit_host(hb.p, b.size(), ze.p, zl, out.p, b.size(), &ol, &st) == BFQ_OK && ol == b.size());
    // every sequence line is A's, every other byte B's
    {
        std::string o((const char *)out.p, ol);
        size_t ia = 0, io = 0, ib = 0;
        for (u32 i = 0; i < 9; i++) {
            for (int l = 0; l < 4; l++) {
                size_t ea = a.find('\n', ia), eo = o.find('\n', io), eb = b.find('\n', ib);
                if (ea == std::string::npos) ea = a.size();
                std::string la = a.substr(ia, ea - ia), lo = o.substr(io, eo - io), lb = b.substr(ib, eb - ib);
                if (!la.empty() && la.back() == '\r') la.pop_back();
                std::string lo2 = lo;
                if (!lo2.empty() && lo2.back() == '\r') lo2.pop_back();
                if (l == 1) CHECK(lo2 == la); else CHECK(lo == lb);
                ia = ea + 1; io = eo + 1; ib = eb + 1;
            }
        }
    }
    // applied to the INPUT instead of the output: target_sum
    Heap out2(a.size());
    memset(out2.p, 0xEE, a.size());
    CHECK(bfq_fastq_unedit_host(ha.p, a.size(), ze.p, zl, out2.p, a.size(), &ol, &st) == BFQ_E_ARG && ol == 0);
    for (u64 i = 0; i < a.size(); i++) if (out2.p[i] != 0xEE) { CHECK(!"written on a refusal"); break; }
    // two members back to back: the text twice
    {
        std::string bb = b + b;
        Heap hbb(bb.size()), zz(2 * zl), o2(bb.size());
        memcpy(hbb.p, bb.data(), bb.size());
        memcpy(zz.p, ze.p, zl); memcpy(zz.p + zl, ze.p, zl);
        CHECK(bfq_fastq_unedit_host(hbb.p, bb.size(), zz.p, 2 * zl, o2.p, bb.size(), &ol, &st) == BFQ_OK && ol == bb.size() && st.edits == 2 * want.size());
        CHECK(!memcmp(o2.p, out.p, b.size()) && !memcmp(o2.p + b.size(), out.p, b.size()));
        CHECK(bfq_fastq_unedit_host(hbb.p, bb.size(), ze.p, zl, o2.p, bb.size(), &ol, &st) == BFQ_E_ARG);   // one member for two blocks
        // read counts that add up to the text's only mod 2^64: refused before they index anything
        Heap two(2 * BFQ_EDIT_HDR);
        bfq_edits_put_header(two.p, ~0ull, 0, 0, 0, 0, 0);
        bfq_edits_put_header(two.p + BFQ_EDIT_HDR, 19, 0, 0, 0, 0, 0);
        memset(o2.p, 0xEE, bb.size());
        CHECK(bfq_fastq_unedit_host(hbb.p, bb.size(), two.p, 2 * BFQ_EDIT_HDR, o2.p, bb.size(), &ol, &st) == BFQ_E_ARG && ol == 0);
        for (u64 i = 0; i < bb.size(); i++) if (o2.p[i] != 0xEE) { CHECK(!"written on a refusal"); break; }
    }
}

int main()
{
    const u64 counts[] = {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000};
    for (u64 E : counts)
        for (u32 bits : {0u, 1u, 7u, 8u, 13u, 31u, 32u, 33u, 44u, 50u}) {
            u32 eb = 0;
            for (u64 x = E; x; x >>= 1) eb++;
            if (bits + eb <= 55) round_trip(E, bits);           // (the positions stay below 2^56)
        }
    // gaps up to 2^55: w = 56
    {
        std::vector<u64> pos = {5, 5 + (1ull << 55) + 1, 5 + (1ull << 55) + 3};
        std::vector<u8> byte = {'A', 'C', 'G'};
        const std::vector<u8> z = member_of(pos, byte, BFQ_EDIT_TMAX);
        BfqEditMember M;
        CHECK(bfq_edits_member(z.data(), z.size(), &M, nullptr) == nullptr && z[M.offW] == 56);
        u64 p[3]; u8 b[3];
        CHECK(bfq_edits_decode_host(z.data(), z.size(), p, b, 3, nullptr, nullptr, nullptr) == BFQ_OK && p[1] == pos[1] && p[2] == pos[2]);
        CHECK(bfq_edits_bound_of(1, BFQ_EDIT_TMAX + 1) == 0 && bfq_edits_bound_of(3, 2) == 0);
    }
    refusals();
    texts();
    printf(g_fail ? "%d checks FAILED\n" : "all checks passed\n", g_fail);
    return g_fail ? 1 : 0;
}
