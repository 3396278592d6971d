// test_bam.cpp -- bfq_bam.h on the host: the header walk, the record check, the record-start rule, the walkers, the chain,
// the repair and the text of every record that the kernels run (bfq_bam_host), over inflated BAM streams the pytest wrote.
// The input and the outputs are exact-size heap blocks of their own, so that under -fsanitize=address,undefined a byte
// read or written beside them ends the run.
//   test_bam MANIFEST      one case per line:
//     good  FILE SPLIT FQ0 FQ1 FQ2     converts to the three texts at pieces 64, 256, 1024, 4096 and 65536; the measure gives
//                                      the same lengths and statistics; a buffer one byte short is refused untouched
//     bad   FILE MSGFILE               refused with that message at pieces 64, 256 and 65536
//     sweep FILE FQ                    the stream cut at every byte length (piece 64): a refusal, or a prefix of the text
//                                      that ends with a whole record
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_bam.h"

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

static bfq_bam_opts options(u32 piece, u32 split)
{
    bfq_bam_opts in{}, O;
    const char *why = nullptr;
    in.exclude_flags = 0x900; in.mate_suffix = 1; in.default_qual = 1; in.split = split; in.piece = piece;
    if (!bfq_bam_resolve(&in, &O, &why)) { printf("options: %s\n", why); exit(2); }
    return O;
}

static bool same_counts(const bfq_bam_stats &a, const bfq_bam_stats &b, bool pieces)
{
    bool same = a.records == b.records && a.written[0] == b.written[0] && a.written[1] == b.written[1] && a.written[2] == b.written[2] &&
                a.skipped == b.skipped && a.reversed == b.reversed && a.no_qual == b.no_qual && a.clamped_quals == b.clamped_quals && a.n_ref == b.n_ref &&
                a.header_bytes == b.header_bytes;
    if (pieces) same = same && a.pieces == b.pieces && a.walkers == b.walkers && a.dead == b.dead && a.repaired == b.repaired && a.rounds == b.rounds;
    return same;
}

static void good(const char *name, const Heap &in, u32 split, const std::vector<u8> want[3])
{
    const u32 pieces[] = {64, 256, 1024, 4096, 65536};
    bfq_bam_stats first{};
    for (u32 piece : pieces) {
        const bfq_bam_opts O = options(piece, split);
        bfq_bam_stats S{}, S2{};
        bfq_bam_err E, E2;
        u64 ol[3], nr[3], ol2[3], nr2[3];
        Heap o0(want[0].size()), o1(want[1].size()), o2(want[2].size());
        u8 *const out[3] = {o0.p, o1.p, o2.p};
        const u64 cap[3] = {o0.n, o1.n, o2.n};
        int r = bfq_bam_host(in.p, in.n, O, out, cap, false, ol, nr, &S, &E);
        CHECK(r == 0, "%s piece %u: %d: %s", name, piece, r, bfq_bam_message(E).c_str());
        for (int k = 0; k < 3; k++)
            CHECK(ol[k] == want[k].size() && (!ol[k] || !memcmp(out[k], want[k].data(), ol[k])), "%s piece %u: text %d differs (%llu bytes, %zu expected)", name, piece, k,
                  ol[k], want[k].size());
        r = bfq_bam_host(in.p, in.n, O, out, cap, true, ol2, nr2, &S2, &E2);
        CHECK(r == 0 && !memcmp(ol, ol2, sizeof ol) && !memcmp(nr, nr2, sizeof nr) && same_counts(S, S2, true), "%s piece %u: the measure differs", name, piece);
        CHECK(S.rounds == S.repaired + 1 && S.walkers >= 1 && S.walkers <= S.pieces && S.records == S.skipped + S.written[0] + S.written[1] + S.written[2],
              "%s piece %u: statistics", name, piece);
        if (piece == pieces[0]) first = S;
        CHECK(same_counts(first, S, false), "%s piece %u: the counts depend on the piece", name, piece);
        for (int k = 0; k < 3; k++) {
            if (!want[k].size()) continue;
            Heap less(want[k].size() - 1);
            memset(less.p, 0xA5, less.n);
            memset(out[(k + 1) % 3], 0xA5, cap[(k + 1) % 3]);
            u8 *const out2[3] = {k == 0 ? less.p : out[0], k == 1 ? less.p : out[1], k == 2 ? less.p : out[2]};
            const u64 cap2[3] = {k == 0 ? less.n : cap[0], k == 1 ? less.n : cap[1], k == 2 ? less.n : cap[2]};
            r = bfq_bam_host(in.p, in.n, O, out2, cap2, false, ol2, nr2, &S2, &E2);
            bool untouched = true;
            for (size_t i = 0; i < less.n; i++) untouched = untouched && less.p[i] == 0xA5;
            for (size_t i = 0; i < cap[(k + 1) % 3]; i++) untouched = untouched && out[(k + 1) % 3][i] == 0xA5;
            CHECK(r == 2 && !memcmp(ol, ol2, sizeof ol) && untouched, "%s piece %u: a short buffer %d: %d", name, piece, k, r);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_bam MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16], a[1024], b[1024], c[1024], d[1024];
    unsigned split = 0;
    int cases = 0;
    while (fscanf(mf, "%15s %1023s", kind, a) == 2) {
        const std::vector<u8> file = slurp(a);
        const Heap in(file.data(), file.size());
        cases++;
        if (!strcmp(kind, "good")) {
            if (fscanf(mf, "%u %1023s %1023s %1023s", &split, b, c, d) != 4) return 2;
            const std::vector<u8> want[3] = {slurp(b), slurp(c), slurp(d)};
            good(a, in, split, want);
        } else if (!strcmp(kind, "bad")) {
            if (fscanf(mf, "%1023s", b) != 1) return 2;
            const std::vector<u8> msg = slurp(b);
            const std::string want(msg.begin(), msg.end());
            const u32 pieces[] = {64, 256, 65536};
            for (u32 piece : pieces) {
                bfq_bam_stats S{};
                bfq_bam_err E;
                u64 ol[3], nr[3];
                Heap o0(1u << 20);
                u8 *const out[3] = {o0.p, nullptr, nullptr};
                const u64 cap[3] = {o0.n, 0, 0};
                const int r = bfq_bam_host(in.p, in.n, options(piece, 0), out, cap, false, ol, nr, &S, &E);
                CHECK(r == 1 && bfq_bam_message(E) == want, "%s piece %u: got %d \"%s\", expected \"%s\"", a, piece, r, bfq_bam_message(E).c_str(), want.c_str());
            }
        } else if (!strcmp(kind, "sweep")) {
            if (fscanf(mf, "%1023s", b) != 1) return 2;
            const std::vector<u8> want = slurp(b);
            u64 exact = 0, refused = 0;
            for (size_t n = 0; n <= file.size(); n++) {
                const Heap cut(file.data(), n);
                bfq_bam_stats S{};
                bfq_bam_err E;
                u64 ol[3], nr[3];
                Heap o0(want.size());
                u8 *const out[3] = {o0.p, nullptr, nullptr};
                const u64 cap[3] = {o0.n, 0, 0};
                const int r = bfq_bam_host(cut.p, cut.n, options(64, 0), out, cap, false, ol, nr, &S, &E);
                if (r == 1) refused++;
                else {
                    exact++;
                    CHECK(r == 0 && ol[0] <= want.size() && !memcmp(o0.p, want.data(), ol[0]) && (!ol[0] || want[ol[0] - 1] == '\n'),
                          "%s cut at %zu: accepted with another text (%d)", a, n, r);
                }
            }
            printf("sweep %s: %llu exact, %llu refused\n", a, exact, refused);
            CHECK(refused > 0 && exact > 1, "a sweep meets both ends");
        } else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
