// test_repair.cpp -- the repair of bfq_pairs.h on the host: the hash, the hints, the roles and the host form that the kernels'
// text is (bfq_pairs_repair_host), over texts and expected outputs the pytest wrote from its model.  Every text and every
// output is an exact-size heap block of its own, so that under -fsanitize=address,undefined a byte read or written beside
// them ends the run.
//   test_repair MANIFEST         one case per line; OPTS = mate_suffix hash_bits seed reserved0 reserved1; a text "-" is absent
//     repair T0 T1 T2 OPTS WANT0 WANT1 WANT2 PAIRS SINGLES DUPS MIXED MAXRUN   gives the three texts with these statistics; the
//                                                            measuring form gives their lengths; an output one byte short is
//                                                            refused untouched
//     bad    T0 T1 T2 OPTS MSGFILE CODE                      refused with that message and code, nothing written
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_pairs.h"

static int g_fail = 0;
#define CHECK(x, ...) do { if (!(x)) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #x); printf(__VA_ARGS__); printf("\n"); g_fail++; } } while (0)

struct Heap {                                     // an exact-size block
    u8 *p; size_t n;
    explicit Heap(size_t n_) : p((u8 *)malloc(n_ ? n_ : 1)), n(n_) { memset(p, 0xA5, n_ ? n_ : 1); }
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

struct Text {
    Heap *h = nullptr;
    const u8 *p = nullptr;
    u64 n = 0;
    explicit Text(const char *name)
    {
        if (!strcmp(name, "-")) return;
        const std::vector<u8> v = slurp(name);
        h = new Heap(v.data(), v.size());
        p = h->p; n = v.size();
    }
    Text(const Text &) = delete;
    ~Text() { delete h; }
};

static bool all_a5(const Heap &b)
{
    for (size_t i = 0; i < b.n; i++)
        if (b.p[i] != 0xA5) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_repair MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    // the hash: the chunks are zero-padded, the length tells "a" from "a\0"; the sum does not depend on who adds what
    {
        const u8 k[17] = {'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 0, 0, 0, 0, 0, 0, 0, 0, 'x'};
        CHECK(bfq_repair_hash(k, 8, 0) != bfq_repair_hash(k, 9, 0) && bfq_repair_hash(k, 9, 0) != bfq_repair_hash(k, 16, 0), "trailing zero bytes");
        CHECK(bfq_repair_hash(k, 8, 0) != bfq_repair_hash(k, 8, 1), "the seed");
        u64 acc = bfq_repair_chunk(bfq_repair_word(k + 16, 1), 2) + bfq_repair_chunk(bfq_repair_word(k, 8), 0) + bfq_repair_chunk(bfq_repair_word(k + 8, 8), 1);
        CHECK(bfq_repair_finish(acc, 17, 7) == bfq_repair_hash(k, 17, 7), "the sum commutes");
        CHECK(bfq_repair_sort_key(~0ull, 1) == 1 && bfq_repair_sort_key(~0ull, 40) == (1ull << 40) - 1, "the sort key");
    }
    char kind[16], t[3][1024], w[3][1024];
    int cases = 0;
    while (fscanf(mf, "%15s", kind) == 1) {
        const bool bad = !strcmp(kind, "bad");
        if (!bad && strcmp(kind, "repair")) { printf("unknown case kind %s\n", kind); return 2; }
        if (fscanf(mf, "%1023s %1023s %1023s", t[0], t[1], t[2]) != 3) return 2;
        bfq_repair_opts in, O;
        unsigned long long seed = 0;
        unsigned ms = 0, hb = 0, r0 = 0, r1 = 0;
        if (fscanf(mf, "%u %u %llu %u %u", &ms, &hb, &seed, &r0, &r1) != 5) return 2;
        in.mate_suffix = ms; in.hash_bits = hb; in.seed = seed; in.reserved[0] = r0; in.reserved[1] = r1;
        const Text T0(t[0]), T1(t[1]), T2(t[2]);
        const u8 *const tp[3] = {T0.p, T1.p, T2.p};
        const uint64_t tn[3] = {T0.n, T1.n, T2.n};
        bfq_pairs_err X;
        bfq_repair_stats S;
        u64 nr[3];
        const bool resolved = bfq_repair_resolve(&in, &O, &X);
        cases++;
        if (bad) {
            int code = 0;
            if (fscanf(mf, "%1023s %d", w[0], &code) != 2) return 2;
            const std::vector<u8> msg = slurp(w[0]);
            const std::string wantMsg(msg.begin(), msg.end());
            Heap o0(1 << 16), o1(1 << 16), o2(1 << 16);
            u8 *const outs[3] = {o0.p, o1.p, o2.p};
            const uint64_t caps[3] = {o0.n, o1.n, o2.n};
            int r = 2;
            if (resolved) r = bfq_pairs_repair_host(tp, tn, O, outs, caps, false, &S, nr, &X);
            const std::string got = r == 2 ? bfq_pairs_message(X) : std::string("not refused");
            CHECK(r == 2 && got == wantMsg && bfq_pairs_code(X) == code, "%s: got %d \"%s\" (%d), expected \"%s\" (%d)", w[0], r, got.c_str(), bfq_pairs_code(X),
                  wantMsg.c_str(), code);
            CHECK(all_a5(o0) && all_a5(o1) && all_a5(o2), "%s: a refusal wrote", w[0]);
            continue;
        }
        unsigned long long pairs = 0, singles = 0, dups = 0, mixed = 0, maxRun = 0;
        if (fscanf(mf, "%1023s %1023s %1023s %llu %llu %llu %llu %llu", w[0], w[1], w[2], &pairs, &singles, &dups, &mixed, &maxRun) != 8) return 2;
        CHECK(resolved, "%s: options refused", w[1]);
        if (!resolved) continue;
        const std::vector<u8> want[3] = {slurp(w[0]), slurp(w[1]), slurp(w[2])};
        int r = bfq_pairs_repair_host(tp, tn, O, nullptr, nullptr, true, &S, nr, &X);
        CHECK(r == 0 && S.out_len[0] == want[0].size() && S.out_len[1] == want[1].size() && S.out_len[2] == want[2].size(), "%s: measure: %d: %s", w[1], r,
              bfq_pairs_message(X).c_str());
        Heap o0(want[0].size()), o1(want[1].size()), o2(want[2].size());
        u8 *const outs[3] = {o0.p, o1.p, o2.p};
        const uint64_t caps[3] = {o0.n, o1.n, o2.n};
        r = bfq_pairs_repair_host(tp, tn, O, outs, caps, false, &S, nr, &X);
        CHECK(r == 0, "%s: %d: %s", w[1], r, bfq_pairs_message(X).c_str());
        for (int k = 0; k < 3; k++) CHECK(!want[k].size() || !memcmp(outs[k], want[k].data(), want[k].size()), "%s: text %d differs", w[1], k);
        CHECK(S.pairs == pairs && S.singles == singles && S.records == 2 * pairs + singles && nr[0] == singles && nr[1] == pairs && nr[2] == pairs,
              "%s: the counts differ", w[1]);
        CHECK(S.dup_groups == dups && S.mixed_runs == mixed && S.max_run == maxRun, "%s: dup_groups %llu, mixed_runs %llu, max_run %llu", w[1],
              (unsigned long long)S.dup_groups, (unsigned long long)S.mixed_runs, (unsigned long long)S.max_run);
        for (int k = 0; k < 3; k++) {
            if (!want[k].size()) continue;
            Heap l0(want[0].size() - (k == 0)), l1(want[1].size() - (k == 1)), l2(want[2].size() - (k == 2));
            u8 *const lo[3] = {l0.p, l1.p, l2.p};
            const uint64_t lc[3] = {l0.n, l1.n, l2.n};
            r = bfq_pairs_repair_host(tp, tn, O, lo, lc, false, &S, nr, &X);
            CHECK(r == 3 && all_a5(l0) && all_a5(l1) && all_a5(l2) && S.out_len[k] == want[k].size(), "%s: a short buffer %d: %d", w[1], k, r);
        }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail || !cases ? 1 : 0;
}
