// test_ubam.cpp -- bfq_ubam.h on the host: the sizing pass, the writing pass and the host form that the kernels' text is
// (bfq_ubam_host_form), over FASTQ texts and expected streams the pytest wrote from its model.  Every text and the output are
// exact-size heap blocks of their own, so that under -fsanitize=address,undefined a byte read or written beside them ends
// the run.
//   test_ubam MANIFEST           one case per line; OPTS = mate_suffix paired_check level; a text, HEADER or RG "-" is absent
//     good T0 T1 T2 OPTS HEADER RG WANT NAMED COMMENTS UNKNOWN   gives the stream WANT with these counts; the measuring form
//                                gives its length; an output one byte short is refused untouched
//     bad  T0 T1 T2 OPTS HEADER RG MSGFILE CODE                  refused with that message and code, nothing written
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_ubam.h"

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

struct Texts {
    Heap *h[3] = {nullptr, nullptr, nullptr};
    const u8 *p[3] = {nullptr, nullptr, nullptr};
    u64 n[3] = {0, 0, 0};
    explicit Texts(char name[3][1024])
    {
        for (int k = 0; k < 3; k++) {
            if (!strcmp(name[k], "-")) continue;
            const std::vector<u8> v = slurp(name[k]);
            h[k] = new Heap(v.data(), v.size());
            p[k] = h[k]->p; n[k] = v.size();
        }
    }
    ~Texts() { for (int k = 0; k < 3; k++) delete h[k]; }
};

static bool all_a5(const Heap &b)
{
    for (size_t i = 0; i < b.n; i++)
        if (b.p[i] != 0xA5) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_ubam MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16], t[3][1024], hname[1024], rname[1024], b[1024];
    unsigned w[3];
    int cases = 0;
    while (fscanf(mf, "%15s %1023s %1023s %1023s %u %u %u %1023s %1023s %1023s", kind, t[0], t[1], t[2], &w[0], &w[1], &w[2], hname, rname, b) == 10) {
        const Texts T(t);
        std::vector<u8> header, rg;
        if (strcmp(hname, "-")) header = slurp(hname);
        if (strcmp(rname, "-")) rg = slurp(rname);
        const Heap hdrBlock(header.data(), header.size());
        rg.push_back(0);
        bfq_ubam_opts in{};
        in.mate_suffix = w[0]; in.paired_check = w[1]; in.level = w[2];
        if (strcmp(hname, "-")) { in.header_text = hdrBlock.p; in.header_len = header.size(); }
        if (strcmp(rname, "-")) in.rg_id = (const char *)rg.data();
        bfq_ubam_opts O;
        bfq_ubam_err X;
        bfq_ubam_stats S;
        const bool resolved = bfq_ubam_resolve(&in, &O, &X);
        cases++;
        if (!strcmp(kind, "good")) {
            unsigned long long want_c[3];
            for (int i = 0; i < 3; i++)
                if (fscanf(mf, "%llu", &want_c[i]) != 1) return 2;
            const std::vector<u8> want = slurp(b);
            CHECK(resolved, "%s: options refused", b);
            if (!resolved) continue;
            int r = bfq_ubam_host_form(T.p, T.n, O, nullptr, 0, true, &S, &X);
            CHECK(r == 0 && S.raw_len == want.size() && S.unknown_bases == 0, "%s: measure: %d: %s", b, r, bfq_ubam_message(X).c_str());
            Heap out(want.size());
            memset(out.p, 0xA5, out.n);
            r = bfq_ubam_host_form(T.p, T.n, O, out.p, out.n, false, &S, &X);
            CHECK(r == 0, "%s: %d: %s", b, r, bfq_ubam_message(X).c_str());
            CHECK(!memcmp(out.p, want.data(), want.size()), "%s: the stream differs", b);
            CHECK(S.named == want_c[0] && S.comments_dropped == want_c[1] && S.unknown_bases == want_c[2] && S.raw_len == want.size() &&
                  S.records == S.written[0] + S.written[1] + S.written[2] && S.members == (want.size() + 65279) / 65280 + 1, "%s: the counts differ", b);
            Heap less(want.size() - 1);
            memset(less.p, 0xA5, less.n);
            r = bfq_ubam_host_form(T.p, T.n, O, less.p, less.n, false, &S, &X);
            CHECK(r == 3 && all_a5(less) && S.raw_len == want.size(), "%s: a short buffer: %d", b, r);
        } else if (!strcmp(kind, "bad")) {
            int code = 0;
            if (fscanf(mf, "%d", &code) != 1) return 2;
            const std::vector<u8> msg = slurp(b);
            const std::string wantMsg(msg.begin(), msg.end());
            Heap out(1 << 20);
            memset(out.p, 0xA5, out.n);
            const int r = resolved ? bfq_ubam_host_form(T.p, T.n, O, out.p, out.n, false, &S, &X) : 2;
            const std::string got = r == 2 ? bfq_ubam_message(X) : std::string("not refused");
            CHECK(r == 2 && got == wantMsg && bfq_ubam_code(X) == code, "%s: got %d \"%s\" (%d), expected \"%s\" (%d)", b, r, got.c_str(), bfq_ubam_code(X),
                  wantMsg.c_str(), code);
            CHECK(all_a5(out), "%s: a refusal wrote", b);
        } else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail || !cases ? 1 : 0;
}
