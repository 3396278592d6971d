// test_bgzf.cpp -- bfq_bgzf.h on the host: the header walk, the inflate and the CRC32 that the kernel runs, over files the
// pytest wrote.  Every buffer is an exact-size heap block of its own (the file, each member's payload, each member's
// output), so that under -fsanitize=address,undefined a byte read or written beside them ends the run.
//   test_bgzf MANIFEST      one case per line:
//     good  FILE.gz EXPECT CRC32HEX       inflates to EXPECT's bytes; CRC32 (zlib's, of the whole text) = serial = parallel form
//     bad   FILE.gz REASON MEMBER OFFSET  refused with that reason at that member, which starts at that byte
//     sweep FILE.gz EXPECT                every byte replaced by 0x00, 0xFF and byte ^ 0x10: the exact text or a refusal
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_bgzf.h"

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

// 0 and the text, or the reason with the member's index and offset
static int inflate_all(const u8 *gz, size_t len, std::vector<u8> &text, u64 *badMember, u64 *badOff)
{
    text.clear();
    u64 n = 0, raw = 0, bad = 0;
    int r = bfq_bgzf_walk(gz, len, nullptr, 0, &n, &raw, &bad);
    std::vector<bfq_bgzf_member> dir(n);
    u64 n2 = 0, raw2 = 0, bad2 = 0;
    const int r2 = bfq_bgzf_walk(gz, len, dir.data(), n, &n2, &raw2, &bad2);
    CHECK(r2 == r && n2 == n && raw2 == raw && bad2 == bad, "the walk is not repeatable");
    for (u64 i = 0; i < n; i++) {
        bfq_bgzf_hdr h;
        const int hr = bfq_bgzf_member_header(gz + dir[i].in_off, dir[i].in_len, &h);
        CHECK(hr == 0 && h.total == dir[i].in_len && h.isize == dir[i].out_len && dir[i].out_off == text.size(), "directory entry %llu", i);
        if (hr) return hr;
        Heap pay(h.payLen), out(h.isize);
        if (h.payLen) memcpy(pay.p, gz + dir[i].in_off + h.payOff, h.payLen);
        const int ir = bfq_bgzf_inflate_payload(pay.p, h.payLen, out.p, h.isize, h.crc, &g_T, g_crcTab, 0, 1);
        if (ir) { *badMember = i; *badOff = dir[i].in_off; return ir; }
        text.insert(text.end(), out.p, out.p + h.isize);
    }
    if (r) { *badMember = n; *badOff = bad; }
    return r;
}

static void check_crc(const std::vector<u8> &text, u32 want)
{
    Heap t(text.size());
    if (text.size()) memcpy(t.p, text.data(), text.size());
    const u32 serial = bfq_crc32_serial(g_crcTab, t.p, text.size());
    CHECK(serial == want, "serial %08x, zlib %08x", serial, want);
    const u32 lanes[] = {1, 2, 7, 64};
    for (u32 nl : lanes) {
        u32 x = 0;
        for (u32 l = 0; l < nl; l++) x ^= bfq_crc32_part(g_crcTab, t.p, (u32)text.size(), l, nl);
        CHECK(x == serial, "%u lanes: %08x, serial %08x (%zu bytes)", nl, x, serial, text.size());
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_bgzf MANIFEST\n"); return 2; }
    for (u32 i = 0; i < 256; i++) g_crcTab[i] = bfq_crc32_entry(i);
    CHECK(g_crcTab[1] == 0x77073096u && g_crcTab[255] == 0x2D02EF8Du, "table");
    CHECK(bfq_crc32_serial(g_crcTab, (const u8 *)"123456789", 9) == 0xCBF43926u, "check value");
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16], a[1024], b[1024];
    unsigned long long x = 0, y = 0;
    int cases = 0;
    while (fscanf(mf, "%15s %1023s %1023s", kind, a, b) == 3) {
        const std::vector<u8> file = slurp(a);
        Heap gz(file.size());
        if (file.size()) memcpy(gz.p, file.data(), file.size());
        std::vector<u8> text;
        u64 bm = 0, bo = 0;
        cases++;
        if (!strcmp(kind, "good")) {
            if (fscanf(mf, "%llx", &x) != 1) return 2;
            const std::vector<u8> want = slurp(b);
            const int r = inflate_all(gz.p, gz.n, text, &bm, &bo);
            CHECK(r == 0, "%s: refused: member %llu at %llu: %s", a, bm, bo, bfq_bgzf_reason(r));
            CHECK(text == want, "%s: the text differs (%zu bytes, %zu expected)", a, text.size(), want.size());
            if (!r) check_crc(text, (u32)x);
        } else if (!strcmp(kind, "bad")) {
            if (fscanf(mf, "%llu %llu", &x, &y) != 2) return 2;
            const int want = atoi(b);
            const int r = inflate_all(gz.p, gz.n, text, &bm, &bo);
            CHECK(r == want && bm == x && bo == y, "%s: got %d (%s) at member %llu byte %llu, expected %d (%s) at member %llu byte %llu", a, r,
                  bfq_bgzf_reason(r), bm, bo, want, bfq_bgzf_reason(want), x, y);
        } else if (!strcmp(kind, "sweep")) {
            const std::vector<u8> want = slurp(b);
            u64 exact = 0, refused = 0;
            for (size_t i = 0; i < gz.n; i++) {
                const u8 keep = gz.p[i];
                const u8 repl[3] = {0x00, 0xFF, (u8)(keep ^ 0x10)};
                for (u8 v : repl) {
                    gz.p[i] = v;
                    const int r = inflate_all(gz.p, gz.n, text, &bm, &bo);
                    if (r) refused++;
                    else { exact++; CHECK(text == want, "%s: byte %zu = %02x: accepted with another text", a, i, v); }
                }
                gz.p[i] = keep;
            }
            printf("sweep %s: %llu exact, %llu refused\n", a, exact, refused);
            CHECK(refused > 0 && exact > 0, "a sweep meets both ends");
        } else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
