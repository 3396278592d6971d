// test_gzip.cpp -- bfq_gzip.h on the host: the member headers, the candidate search, both decoder passes, the windows, the
// resolve and the members' CRC32 that the kernels run (bfq_gzip_host), over files the pytest wrote.  The input and the output
// are exact-size heap blocks of their own, so that under -fsanitize=address,undefined a byte read or written beside them
// ends the run.
//   test_gzip MANIFEST      one case per line:
//     good  FILE.gz EXPECT CHUNKS             inflates to EXPECT's bytes at every chunk of the comma-separated list; the
//                                            measure gives the same length and statistics; a buffer one byte short is refused
//                                            untouched
//     bad   FILE.gz REASON MEMBER OFFSET     refused with that reason at that member, whose header starts at that byte, at
//                                            chunks 512, 4096 and 32768
//     sweep FILE.gz EXPECT                   the file cut at every byte length (chunk 512): a refusal, or the exact text
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_gzip.h"

static int g_fail = 0;
#define CHECK(x, ...) do { if (!(x)) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #x); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct Heap {                                     // an exact-size block
    u8 *p; size_t n;
    explicit Heap(size_t n_) : p((u8 *)malloc(n_ ? n_ : 1)), n(n_) {}
    Heap(const u8 *src, size_t n_) : Heap(n_) { if (n_) memcpy(p, src, n_); }
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

static bool same_stats(const bfq_gzip_stats &a, const bfq_gzip_stats &b)
{
    return a.members == b.members && a.pieces == b.pieces && a.decoders == b.decoders && a.chain == b.chain && a.skipped == b.skipped &&
           a.discarded == b.discarded;
}

static void good(const char *name, const Heap &gz, const std::vector<u8> &want, u64 chunk)
{
    bfq_gzip_stats S{}, S2{};
    bfq_gzip_err E, E2;
    u64 raw = 0, raw2 = 0;
    Heap out(want.size());
    int r = bfq_gzip_host(gz.p, gz.n, chunk, out.p, out.n, false, &raw, &S, &E);
    CHECK(r == 0, "%s chunk %llu: %d: member %llu at %llu: %s", name, chunk, r, E.member, E.off, bfq_gzip_reason(E.reason));
    CHECK(raw == want.size() && (!raw || !memcmp(out.p, want.data(), raw)), "%s chunk %llu: the text differs (%llu bytes, %zu expected)", name, chunk, raw, want.size());
    r = bfq_gzip_host(gz.p, gz.n, chunk, nullptr, 0, true, &raw2, &S2, &E2);
    CHECK(r == 0 && raw2 == raw && same_stats(S, S2), "%s chunk %llu: the measure differs", name, chunk);
    CHECK(S.decoders == S.chain + S.discarded && S.chain >= 1 && S.pieces == bfq_gzip_pieces(gz.n, chunk), "%s chunk %llu: statistics", name, chunk);
    if (want.size()) {
        Heap less(want.size() - 1);
        memset(less.p, 0xA5, less.n);
        r = bfq_gzip_host(gz.p, gz.n, chunk, less.p, less.n, false, &raw2, &S2, &E2);
        bool untouched = true;
        for (size_t i = 0; i < less.n; i++) untouched = untouched && less.p[i] == 0xA5;
        CHECK(r == 2 && raw2 == raw && untouched, "%s chunk %llu: a short buffer: %d", name, chunk, r);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_gzip MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16], a[1024], b[1024], cs[256];
    unsigned long long x = 0, y = 0;
    int cases = 0;
    while (fscanf(mf, "%15s %1023s %1023s", kind, a, b) == 3) {
        const std::vector<u8> file = slurp(a);
        const Heap gz(file.data(), file.size());
        cases++;
        if (!strcmp(kind, "good")) {
            if (fscanf(mf, "%255s", cs) != 1) return 2;
            const std::vector<u8> want = slurp(b);
            for (char *t = strtok(cs, ","); t; t = strtok(nullptr, ",")) good(a, gz, want, strtoull(t, nullptr, 10));
        } else if (!strcmp(kind, "bad")) {
            if (fscanf(mf, "%llu %llu", &x, &y) != 2) return 2;
            const int want = atoi(b);
            const u64 chunks[] = {512, 4096, 32768};
            for (u64 chunk : chunks) {
                bfq_gzip_stats S{};
                bfq_gzip_err E;
                u64 raw = 0;
                Heap out(1u << 20);
                const int r = bfq_gzip_host(gz.p, gz.n, chunk, out.p, out.n, false, &raw, &S, &E);
                CHECK(r == 1 && E.reason == want && E.member == x && E.off == y, "%s chunk %llu: got %d, %d (%s) at member %llu byte %llu, expected %d (%s) at member %llu byte %llu",
                      a, chunk, r, E.reason, bfq_gzip_reason(E.reason), E.member, E.off, want, bfq_gzip_reason(want), x, y);
            }
        } else if (!strcmp(kind, "sweep")) {
            const std::vector<u8> want = slurp(b);
            u64 exact = 0, refused = 0;
            for (size_t n = 0; n <= file.size(); n++) {
                const Heap cut(file.data(), n);
                bfq_gzip_stats S{};
                bfq_gzip_err E;
                u64 raw = 0;
                Heap out(want.size());
                const int r = bfq_gzip_host(cut.p, cut.n, 512, out.p, out.n, false, &raw, &S, &E);
                if (r == 1) refused++;
                else {
                    exact++;
                    CHECK(r == 0 && raw == want.size() && !memcmp(out.p, want.data(), raw), "%s cut at %zu: accepted with another text (%d)", a, n, r);
                }
            }
            printf("sweep %s: %llu exact, %llu refused\n", a, exact, refused);
            CHECK(refused > 0 && exact > 0, "a sweep meets both ends");
        } else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
