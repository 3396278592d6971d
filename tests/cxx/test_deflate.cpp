// test_deflate.cpp -- bfq_deflate.h on the host: the BGZF writer that the kernel runs, over texts the pytest wrote.  Every
// buffer is an exact-size heap block of its own, so that under -fsanitize=address,undefined a byte read or written beside
// them ends the run.
//   test_deflate MANIFEST      one text file per line
//     - the host form at level 1 and 0: within the bound, level 0 exactly len + 31 * members + 28, ends with the EOF member;
//       every member inflates (bfq_bgzf_inflate_payload, lane 0 of 1) to its piece of the text;
//     - every member again into a slot of exactly its piece + 31 bytes (rounded to words) between guard bands.
//   Before the texts: the length limiter on Fibonacci weights, a single used symbol, the bound's arithmetic.
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_deflate.h"

static int g_fail = 0;
#define CHECK(x, ...) do { if (!(x)) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #x); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct Heap {                                     // an exact-size block
    u8 *p; size_t n;
    explicit Heap(size_t n_) : p((u8 *)malloc(n_ ? n_ : 1)), n(n_) {}
    Heap(const Heap &) = delete;
    ~Heap() { free(p); }
};

static std::vector<u8> slurp(const char *path)
{
    std::vector<u8> v;
    FILE *f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); exit(2); }
    u8 buf[65536];
    size_t r;
    while ((r = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + r);
    fclose(f);
    return v;
}

static u32 g_crcTab[256];
static bfq_bgzf_tables g_T;
static bfq_defl_work g_W;

// lengths of `n` weights at `limit`: none above it, Kraft sum 1
static void check_limiter(const u32 *freq, u32 n, u32 limit, const char *what)
{
    u8 lens[320];
    bfq_defl_lengths(freq, n, limit, lens, &g_W);
    u64 kraft = 0;
    u32 longest = 0, used = 0;
    for (u32 i = 0; i < n; i++) {
        CHECK((lens[i] != 0) == (freq[i] != 0), "%s: symbol %u: weight %u, length %u", what, i, freq[i], lens[i]);
        if (!lens[i]) continue;
        used++;
        if (lens[i] > longest) longest = lens[i];
        if (lens[i] <= limit) kraft += 1ull << (limit - lens[i]);
    }
    CHECK(longest <= limit, "%s: a length of %u above the limit %u", what, longest, limit);
    CHECK(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu over %u symbols", what, kraft, 1ull << limit, used);
    // heavier symbols never get longer codes
    for (u32 i = 0; i < n; i++)
        for (u32 j = 0; j < n; j++)
            if (freq[i] && freq[j] && freq[i] > freq[j]) CHECK(lens[i] <= lens[j], "%s: weights %u > %u, lengths %u > %u", what, freq[i], freq[j], lens[i], lens[j]);
}

static void limiter_cases()
{
    u32 fib[320];
    memset(fib, 0, sizeof fib);
    fib[0] = fib[1] = 1;
    for (u32 i = 2; i < 30; i++) fib[i] = fib[i - 1] + fib[i - 2];
    check_limiter(fib, 30, 15, "fibonacci 30 @ 15");
    check_limiter(fib, 12, 7, "fibonacci 12 @ 7");
    check_limiter(fib, 19, 7, "fibonacci 19 @ 7");
    u32 rev[30];
    for (u32 i = 0; i < 30; i++) rev[i] = fib[29 - i];
    check_limiter(rev, 30, 15, "fibonacci 30 reversed @ 15");
    u32 flat[286];
    for (u32 i = 0; i < 286; i++) flat[i] = 7;
    check_limiter(flat, 286, 15, "286 equal weights");
    check_limiter(flat, 2, 15, "two symbols");
    u32 gaps[286];
    for (u32 i = 0; i < 286; i++) gaps[i] = i % 3 == 0 ? 1u + (i * 2654435761u >> 20) : 0;
    check_limiter(gaps, 286, 15, "hashed weights with gaps");
    // a single used symbol: one bit, and a block coded with it decodes
    u32 one[30];
    u8 lens[32];
    memset(one, 0, sizeof one);
    one[5] = 9;
    bfq_defl_lengths(one, 30, 15, lens, &g_W);
    for (u32 i = 0; i < 30; i++) CHECK(lens[i] == (i == 5 ? 1 : 0), "single symbol: length %u at %u", lens[i], i);
    u16 count[16], sym[32], offs[16], fast[256];
    CHECK(bfq_bgzf_build(lens, 30, count, sym, offs, fast, 8) == 1 && count[1] == 1, "the inflater takes the single one-bit code as incomplete");
    memset(one, 0, sizeof one);
    bfq_defl_lengths(one, 30, 15, lens, &g_W);
    for (u32 i = 0; i < 30; i++) CHECK(lens[i] == 0, "no symbol: length %u at %u", lens[i], i);
    // symbols and extra bits against the inflater's tables
    for (u32 len = 3; len <= 258; len++) {
        const u32 s = bfq_defl_lsym(len), i = s - 257, ext = bfq_defl_lext(len);
        const u32 base = s == 285 ? 258 : i < 8 ? 3 + i : 3 + ((4 + (i & 3u)) << ((i >> 2) - 1));
        CHECK(s >= 257 && s <= 285 && ext == (s == 285 || i < 8 ? 0 : (i >> 2) - 1) && len >= base && len - base < (1u << ext), "length %u: symbol %u, %u extra", len, s, ext);
    }
    for (u32 d = 1; d <= 32768; d++) {
        const u32 s = bfq_defl_dsym(d), ext = bfq_defl_dext(d);
        const u32 base = s < 4 ? 1 + s : 1 + ((2 + (s & 1u)) << ((s >> 1) - 1));
        CHECK(s < 30 && ext == (s < 4 ? 0 : (s >> 1) - 1) && d >= base && d - base < (1u << ext), "distance %u: symbol %u, %u extra", d, s, ext);
    }
    CHECK(bfq_defl_bound(0) == 28 && bfq_defl_bound(1) == 60 && bfq_defl_bound(65280) == 65339 && bfq_defl_bound(65281) == 65371, "bound");
    for (u32 i = 0; i < 28; i++) CHECK(bfq_defl_eof_byte(i) == (u8)"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0\x1b\0\x03\0\0\0\0\0\0\0\0\0"[i], "EOF byte %u", i);
}

// the members of gz[0, len) inflated and compared with text; returns the number of members before the EOF member
static u64 check_stream(const u8 *gz, u64 len, const std::vector<u8> &text, const char *name, int level)
{
    u64 n = 0, raw = 0, bad = 0;
    const int r = bfq_bgzf_walk(gz, len, nullptr, 0, &n, &raw, &bad);
    CHECK(r == 0 && raw == text.size(), "%s level %d: walk %d, raw %llu of %zu", name, level, r, raw, text.size());
    if (r) return 0;
    std::vector<bfq_bgzf_member> dir(n);
    bfq_bgzf_walk(gz, len, dir.data(), n, &n, &raw, &bad);
    CHECK(n == bfq_defl_members(text.size()) + 1, "%s level %d: %llu members", name, level, n);
    CHECK(n >= 1 && dir[n - 1].in_len == 28 && dir[n - 1].out_len == 0, "%s level %d: no EOF member at the end", name, level);
    for (u64 i = 0; i < n; i++) {
        bfq_bgzf_hdr h;
        const int hr = bfq_bgzf_member_header(gz + dir[i].in_off, dir[i].in_len, &h);
        CHECK(hr == 0, "%s level %d: header of member %llu", name, level, i);
        if (hr) return 0;
        if (i + 1 < n) CHECK(h.isize == (i + 2 < n ? BFQ_DEFL_PIECE : text.size() - i * BFQ_DEFL_PIECE), "%s level %d: member %llu holds %u bytes", name, level, i, h.isize);
        CHECK(h.total <= h.isize + BFQ_DEFL_OVER || h.isize == 0, "%s level %d: member %llu: %u bytes for %u", name, level, i, h.total, h.isize);
        if (level == 0 && i + 1 < n) CHECK(h.total == h.isize + BFQ_DEFL_OVER, "%s: stored member %llu: %u bytes for %u", name, i, h.total, h.isize);
        Heap pay(h.payLen), out(h.isize);
        if (h.payLen) memcpy(pay.p, gz + dir[i].in_off + h.payOff, h.payLen);
        const int ir = bfq_bgzf_inflate_payload(pay.p, h.payLen, out.p, h.isize, h.crc, &g_T, g_crcTab, 0, 1);
        CHECK(ir == 0, "%s level %d: member %llu is refused: %s", name, level, i, bfq_bgzf_reason(ir));
        if (!ir && h.isize) CHECK(!memcmp(out.p, text.data() + dir[i].out_off, h.isize), "%s level %d: member %llu inflates to another text", name, level, i);
    }
    return n - 1;
}

static void check_text(const char *name)
{
    const std::vector<u8> text = slurp(name);
    Heap in(text.size());
    if (text.size()) memcpy(in.p, text.data(), text.size());
    const u64 bound = bfq_defl_bound(text.size());
    u64 size[2] = {0, 0};
    for (int level = 1; level >= 0; level--) {
        Heap out(bound);
        u64 ol = 0;
        const int r = bfq_defl_host(in.p, in.n, level, out.p, bound, &ol);
        CHECK(r == 0 && ol <= bound && ol >= 28, "%s level %d: %d, %llu bytes of %llu", name, level, r, ol, bound);
        if (r) continue;
        size[level] = ol;
        const u64 m = check_stream(out.p, ol, text, name, level);
        if (level == 0) CHECK(ol == text.size() + 31 * m + 28, "%s: %llu bytes stored", name, ol);
        // the same again: the same bytes
        Heap again(bound);
        u64 ol2 = 0;
        bfq_defl_host(in.p, in.n, level, again.p, bound, &ol2);
        CHECK(ol2 == ol && !memcmp(again.p, out.p, ol), "%s level %d: a second run gives other bytes", name, level);
        u64 ol3 = 7;
        if (bound) CHECK(bfq_defl_host(in.p, in.n, level, again.p, bound - 1, &ol3) == 1 && ol3 == 0, "%s: a capacity below the bound is taken", name);
    }
    CHECK(size[1] <= size[0], "%s: %llu bytes coded, %llu stored", name, size[1], size[0]);
    printf("%s: %zu bytes -> %llu (level 1), %llu (level 0)\n", name, text.size(), size[1], size[0]);
    // member by member into a slot of exactly piece + 31 (in whole words) between guard bands
    std::vector<u32> tok(BFQ_DEFL_PIECE);
    for (u64 off = 0; off < text.size(); off += BFQ_DEFL_PIECE) {
        const u32 n = (u32)(text.size() - off < BFQ_DEFL_PIECE ? text.size() - off : BFQ_DEFL_PIECE);
        const u32 cap = (n + BFQ_DEFL_OVER + 3) & ~3u, band = 64;
        for (int level = 1; level >= 0; level--) {
            Heap piece(n), slot(cap + 2 * band);
            memcpy(piece.p, text.data() + off, n);
            memset(slot.p, 0xA5, slot.n);
            const u32 sz = bfq_defl_member(piece.p, n, level, slot.p + band, cap, tok.data(), &g_W, g_crcTab, 0, 1);
            CHECK(sz <= n + BFQ_DEFL_OVER, "%s: member at %llu: %u bytes for %u", name, off, sz, n);
            bool clean = true;
            for (u32 i = 0; i < band; i++) clean = clean && slot.p[i] == 0xA5 && slot.p[band + cap + i] == 0xA5;
            CHECK(clean, "%s: member at %llu level %d: a guard band is written", name, off, level);
            Heap exact(cap);                                              // ... and with nothing around it but the allocator's red zones
            const u32 sz2 = bfq_defl_member(piece.p, n, level, exact.p, cap, tok.data(), &g_W, g_crcTab, 0, 1);
            CHECK(sz2 == sz && !memcmp(exact.p, slot.p + band, sz), "%s: member at %llu level %d: other bytes in another slot", name, off, level);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_deflate MANIFEST\n"); return 2; }
    for (u32 i = 0; i < 256; i++) g_crcTab[i] = bfq_crc32_entry(i);
    limiter_cases();
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char a[1024];
    int cases = 0;
    while (fscanf(mf, "%1023s", a) == 1) { check_text(a); cases++; }
    fclose(mf);
    printf("%d texts, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
