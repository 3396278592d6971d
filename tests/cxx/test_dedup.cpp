// test_dedup.cpp -- bfq_dedup.h on the host: the host form that the kernels' text is (bfq_dedup_host), over texts and expected
// outputs the pytest wrote from its model.  Every text and every output is an exact-size heap block of its own, so that under
// -fsanitize=address,undefined a byte read or written beside them ends the run.
//   test_dedup MANIFEST          one case per line; OPTS = keep hash_bits seed reserved0 reserved1; a text "-" is absent
//     dedup T0 T1 OPTS KEPT0 KEPT1 DUP0 DUP1 STATS    gives the four texts; STATS = kept removed dup_groups max_group
//                                                     max_group_first mixed_runs max_run rounds.  The measuring form gives
//                                                     the lengths; without the removed texts the kept ones are the same; an
//                                                     output one byte short is refused untouched
//     bad   T0 T1 OPTS MSGFILE CODE                   refused with that message and code, nothing written
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_dedup.h"

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
static bool same(const Heap &b, const Text &w) { return b.n == w.n && (!w.n || !memcmp(b.p, w.p, w.n)); }

static bfq_dedup_opts opts_of(char **w)
{
    bfq_dedup_opts O;
    O.keep = (uint32_t)strtoul(w[0], nullptr, 10); O.hash_bits = (uint32_t)strtoul(w[1], nullptr, 10); O.seed = strtoull(w[2], nullptr, 10);
    O.reserved[0] = (uint32_t)strtoul(w[3], nullptr, 10); O.reserved[1] = (uint32_t)strtoul(w[4], nullptr, 10);
    return O;
}

// the host entry point's order: the options, then the texts
static int run(const Text &t0, const Text &t1, const bfq_dedup_opts &in, Heap *out[2], Heap *dup[2], bool measure, bfq_dedup_stats *S, bfq_dedup_err *X)
{
    bfq_dedup_opts O;
    *X = bfq_dedup_err{};
    *S = bfq_dedup_stats{};
    if (!bfq_dedup_resolve(&in, &O, X)) return 2;
    const u8 *const text[2] = {t0.p, t1.p};
    const uint64_t len[2] = {t0.n, t1.n};
    u8 *const o[2] = {out ? out[0]->p : nullptr, out ? out[1]->p : nullptr}, *const d[2] = {dup ? dup[0]->p : nullptr, dup ? dup[1]->p : nullptr};
    const uint64_t oc[2] = {out ? out[0]->n : 0, out ? out[1]->n : 0}, dc[2] = {dup ? dup[0]->n : 0, dup ? dup[1]->n : 0};
    return bfq_dedup_host(text, len, O, o, oc, dup ? d : nullptr, dc, measure, S, X);
}

static void case_dedup(char **w)
{
    const Text t0(w[0]), t1(w[1]), k0(w[7]), k1(w[8]), d0(w[9]), d1(w[10]);
    const bfq_dedup_opts O = opts_of(w + 2);
    u64 want[8];
    for (int k = 0; k < 8; k++) want[k] = strtoull(w[11 + k], nullptr, 10);
    bfq_dedup_stats S;
    bfq_dedup_err X;
    CHECK(run(t0, t1, O, nullptr, nullptr, true, &S, &X) == 0, "measure: %s", bfq_dedup_message(X).c_str());
    CHECK(S.out_len[0] == k0.n && S.out_len[1] == k1.n && S.dup_len[0] == d0.n && S.dup_len[1] == d1.n, "the measured lengths");
    {
        Heap a(k0.n), b(k1.n), c(d0.n), d(d1.n), *out[2] = {&a, &b}, *dup[2] = {&c, &d};
        CHECK(run(t0, t1, O, out, dup, false, &S, &X) == 0, "%s", bfq_dedup_message(X).c_str());
        CHECK(same(a, k0) && same(b, k1) && same(c, d0) && same(d, d1), "the four texts");
        const u64 got[8] = {S.kept, S.removed, S.dup_groups, S.max_group, S.max_group_first, S.mixed_runs, S.max_run, S.rounds};
        for (int k = 0; k < 8; k++) CHECK(got[k] == want[k], "statistic %d: %llu, expected %llu", k, got[k], want[k]);
        u64 groups = 0, units = 0;
        for (int l = 0; l < 32; l++) { groups += S.level_groups[l]; units += S.level_units[l]; }
        CHECK(groups == S.kept && units == S.units && S.units == S.kept + S.removed, "the levels add up");
    }
    {
        Heap a(k0.n), b(k1.n), *out[2] = {&a, &b};                   // the removed records counted, not written
        CHECK(run(t0, t1, O, out, nullptr, false, &S, &X) == 0 && same(a, k0) && same(b, k1) && S.dup_len[0] == d0.n, "without the removed texts");
    }
    for (int sh = 0; sh < 4; sh++) {                                 // one output one byte short: refused, nothing written
        const u64 n[4] = {k0.n, k1.n, d0.n, d1.n};
        if (!n[sh]) continue;
        Heap a(n[0] - (sh == 0)), b(n[1] - (sh == 1)), c(n[2] - (sh == 2)), d(n[3] - (sh == 3)), *out[2] = {&a, &b}, *dup[2] = {&c, &d};
        CHECK(run(t0, t1, O, out, dup, false, &S, &X) == 3, "a short output %d", sh);
        CHECK(all_a5(a) && all_a5(b) && all_a5(c) && all_a5(d) && S.out_len[0] == n[0] && S.dup_len[1] == n[3], "a short output %d wrote, or lost the lengths", sh);
    }
}

static void case_bad(char **w)
{
    const Text t0(w[0]), t1(w[1]), msg(w[7]);
    const bfq_dedup_opts O = opts_of(w + 2);
    const int code = atoi(w[8]);
    Heap a(t0.n + 1), b(t1.n + 1), c(t0.n + 1), d(t1.n + 1), *out[2] = {&a, &b}, *dup[2] = {&c, &d};
    bfq_dedup_stats S;
    bfq_dedup_err X;
    CHECK(run(t0, t1, O, out, dup, false, &S, &X) == 2, "not refused");
    const std::string m = bfq_dedup_message(X);
    CHECK(m.size() == msg.n && !memcmp(m.data(), msg.p, msg.n) && bfq_dedup_code(X) == code, "message '%s' code %d", m.c_str(), bfq_dedup_code(X));
    CHECK(all_a5(a) && all_a5(b) && all_a5(c) && all_a5(d), "a refusal wrote");
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: %s MANIFEST\n", argv[0]); return 2; }
    std::vector<u8> man = slurp(argv[1]);
    man.push_back(0);
    int cases = 0;
    for (char *line = strtok((char *)man.data(), "\n"), *next; line; line = next) {
        next = strtok(nullptr, "\n");
        std::vector<char *> w;
        for (char *p = line; *p;) {
            while (*p == ' ') *p++ = 0;
            if (!*p) break;
            w.push_back(p);
            while (*p && *p != ' ') p++;
        }
        if (w.empty()) continue;
        const int before = g_fail;
        if (!strcmp(w[0], "dedup") && w.size() == 20) case_dedup(w.data() + 1);
        else if (!strcmp(w[0], "bad") && w.size() == 10) case_bad(w.data() + 1);
        else { printf("bad manifest line: %s (%zu words)\n", w[0], w.size()); return 2; }
        if (g_fail != before) printf("  ... in case %d (%s %s)\n", cases, w[0], w[1]);
        cases++;
    }
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail ? 1 : 0;
}
