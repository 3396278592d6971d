// test_bam_patch.cpp -- bfq_bam_patch.h on the host: the checking walk, the patching walk and the host form that the kernels'
// text is (bfq_bam_patch_host_form), over inflated BAM streams, FASTQ texts and expected streams the pytest wrote from its
// model.  The stream, every text and the output are exact-size heap blocks of their own, so that under
// -fsanitize=address,undefined a byte read or written beside them ends the run.
//   test_bam_patch MANIFEST      one case per line; OPTS = exclude_flags mate_suffix default_qual split check_names; a text "-"
//                                is absent
//     good STREAM OPTS T0 T1 T2 WANT RC BC QC UB KH KA   patches to WANT with these counts (reads / bases / quals changed, unknown
//                                bases, kept high, kept absent) at pieces 64, 1024 and 65536; the counts do not depend on the
//                                piece; an output one byte short is refused untouched
//     bad  STREAM OPTS T0 T1 T2 MSGFILE                   refused with that message at pieces 64, 256 and 65536, nothing written
// Exit code 0 = all checks passed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../bfqzip_amd/csrc/bfq_bam_patch.h"

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

static bfq_bam_opts options(const unsigned w[5], u32 piece)
{
    bfq_bam_opts in{}, O;
    const char *why = nullptr;
    in.exclude_flags = w[0]; in.mate_suffix = w[1]; in.default_qual = w[2]; in.split = w[3]; in.check_names = w[4]; in.piece = piece;
    if (!bfq_bam_resolve(&in, &O, &why)) { printf("options: %s\n", why); exit(2); }
    return O;
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
    if (argc != 2) { printf("usage: test_bam_patch MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16], a[1024], t[3][1024], b[1024];
    unsigned w[5];
    int cases = 0;
    while (fscanf(mf, "%15s %1023s %u %u %u %u %u %1023s %1023s %1023s %1023s", kind, a, &w[0], &w[1], &w[2], &w[3], &w[4], t[0], t[1], t[2], b) == 11) {
        const std::vector<u8> file = slurp(a);
        const Heap in(file.data(), file.size());
        const Texts T(t);
        cases++;
        if (!strcmp(kind, "good")) {
            unsigned long long want_c[6];
            for (int i = 0; i < 6; i++)
                if (fscanf(mf, "%llu", &want_c[i]) != 1) return 2;
            const std::vector<u8> want = slurp(b);
            const u32 pieces[] = {64, 1024, 65536};
            for (u32 piece : pieces) {
                const bfq_bam_opts O = options(w, piece);
                bfq_bam_patch_stats S;
                bfq_bam_err E;
                bfq_bamp_err X;
                Heap out(in.n);
                memset(out.p, 0xA5, out.n);
                int r = bfq_bam_patch_host_form(in.p, in.n, O, T.p, T.n, out.p, out.n, &S, &E, &X);
                CHECK(r == 0, "%s piece %u: %d: %s / %s", a, piece, r, bfq_bam_message(E).c_str(), bfq_bamp_message(X).c_str());
                CHECK(want.size() == in.n && !memcmp(out.p, want.data(), in.n), "%s piece %u: the stream differs", a, piece);
                CHECK(S.reads_changed == want_c[0] && S.bases_changed == want_c[1] && S.quals_changed == want_c[2] && S.unknown_bases == want_c[3] &&
                      S.kept_high_quals == want_c[4] && S.kept_absent == want_c[5] && S.raw_len == in.n &&
                      S.records == S.skipped + S.patched[0] + S.patched[1] + S.patched[2], "%s piece %u: the counts differ", a, piece);
                if (in.n) {
                    Heap less(in.n - 1);
                    memset(less.p, 0xA5, less.n);
                    r = bfq_bam_patch_host_form(in.p, in.n, O, T.p, T.n, less.p, less.n, &S, &E, &X);
                    CHECK(r == 3 && all_a5(less) && S.raw_len == in.n, "%s piece %u: a short buffer: %d", a, piece, r);
                }
            }
        } else if (!strcmp(kind, "bad")) {
            const std::vector<u8> msg = slurp(b);
            const std::string want(msg.begin(), msg.end());
            const u32 pieces[] = {64, 256, 65536};
            for (u32 piece : pieces) {
                bfq_bam_patch_stats S;
                bfq_bam_err E;
                bfq_bamp_err X;
                Heap out(in.n);
                memset(out.p, 0xA5, out.n);
                const int r = bfq_bam_patch_host_form(in.p, in.n, options(w, piece), T.p, T.n, out.p, out.n, &S, &E, &X);
                const std::string got = r == 1 ? bfq_bam_message(E) : r == 2 ? bfq_bamp_message(X) : std::string("not refused");
                CHECK((r == 1 || r == 2) && got == want, "%s piece %u: got %d \"%s\", expected \"%s\"", a, piece, r, got.c_str(), want.c_str());
                CHECK(all_a5(out), "%s piece %u: a refusal wrote", a, piece);
            }
        } else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail || !cases ? 1 : 0;
}
