// test_bam_tags.cpp -- the aux tags of bfq_bam.h (records to header lines) and bfq_ubam.h (header lines to records) on the
// host: the host forms that the kernels' text is (bfq_bam_host, bfq_ubam_host_form) with a tag selection, over streams,
// texts and expected results the pytest wrote from its model.  Every input and output is an exact-size heap block of its
// own, so that under -fsanitize=address,undefined a byte read or written beside them ends the run.
//   test_bam_tags MANIFEST       one case per line; SEL = '*' or a list (BC,RX); a text or RG "-" is absent
//     in    STREAM SEL STRICT PIECE SPLIT SUFFIX W0 W1 W2 WRITTEN DROPPED BYTES   gives the texts W0..W2 with these tag counts;
//                                the measuring form gives their lengths; an output one byte short is refused untouched
//     inbad STREAM SEL STRICT PIECE MSGFILE                                      refused with that message, nothing written
//     out   T0 T1 T2 SEL PAIRED RG WANT COMMENTS WRITTEN DROPPED BYTES           gives the stream WANT with these counts
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

static bool all_a5(const Heap &b)
{
    for (size_t i = 0; i < b.n; i++)
        if (b.p[i] != 0xA5) return false;
    return true;
}

// SEL into the extension's list
template <class X> static void select(const char *sel, X *x)
{
    x->n_tags = 0;
    if (!strcmp(sel, "*")) return;
    for (const char *p = sel; p[0] && p[1]; p += p[2] ? 3 : 2) { x->tag[x->n_tags][0] = (u8)p[0]; x->tag[x->n_tags][1] = (u8)p[1]; x->n_tags++; }
}

static void way_in(FILE *mf, bool good)
{
    char sname[1024], sel[256], w[3][1024], msgName[1024];
    unsigned strict, piece, split = 0, suffix = 1;
    unsigned long long wc[3] = {0, 0, 0};
    if (fscanf(mf, "%1023s %255s %u %u", sname, sel, &strict, &piece) != 4) exit(2);
    if (good) {
        if (fscanf(mf, "%u %u %1023s %1023s %1023s %llu %llu %llu", &split, &suffix, w[0], w[1], w[2], &wc[0], &wc[1], &wc[2]) != 8) exit(2);
    } else if (fscanf(mf, "%1023s", msgName) != 1) exit(2);
    const std::vector<u8> sv = slurp(sname);
    const Heap stream(sv.data(), sv.size());
    bfq_bam_tag_opts X{};
    bfq_bam_tag_stats TS{};
    const char *why = nullptr;
    bfq_bam_opts O;
    bfq_bam_resolve(nullptr, &X.o, &why);
    X.o.piece = piece; X.o.split = split; X.o.mate_suffix = suffix; X.o.reserved = BFQ_BAM_OPTS_TAGS;
    X.strict = strict;
    select(sel, &X);
    bfq_bam_tagsel G;
    bfq_bam_tag_stats *where = nullptr;
    CHECK(bfq_bam_resolve(&X.o, &O, &why) && bfq_bam_tags_resolve(&X.o, &G, &where, &why) && G.on && where == nullptr, "%s: options refused", sname);
    u64 ol[3], nr[3];
    bfq_bam_stats S;
    bfq_bam_err E;
    u8 *const none[3] = {nullptr, nullptr, nullptr};
    const u64 zero[3] = {0, 0, 0};
    if (good) {
        std::vector<u8> want[3];
        for (int k = 0; k < 3; k++) want[k] = slurp(w[k]);
        int r = bfq_bam_host(stream.p, stream.n, O, none, zero, true, ol, nr, &S, &E, &G, &TS);
        CHECK(r == 0 && ol[0] == want[0].size() && ol[1] == want[1].size() && ol[2] == want[2].size(), "%s: measure: %d", sname, r);
        Heap o0(want[0].size()), o1(want[1].size()), o2(want[2].size());
        memset(o0.p, 0xA5, o0.n); memset(o1.p, 0xA5, o1.n); memset(o2.p, 0xA5, o2.n);
        u8 *const out[3] = {o0.p, o1.p, o2.p};
        const u64 cap[3] = {o0.n, o1.n, o2.n};
        TS = bfq_bam_tag_stats{};
        r = bfq_bam_host(stream.p, stream.n, O, out, cap, false, ol, nr, &S, &E, &G, &TS);
        CHECK(r == 0, "%s: %d: %s", sname, r, bfq_bam_message(E).c_str());
        for (int k = 0; k < 3; k++) CHECK(!want[k].size() || !memcmp(out[k], want[k].data(), want[k].size()), "%s: text %d differs", sname, k);
        CHECK(TS.tags_written == wc[0] && TS.tags_dropped == wc[1] && TS.tag_bytes == wc[2], "%s: the tag counts differ: %llu %llu %llu", sname, TS.tags_written,
              TS.tags_dropped, TS.tag_bytes);
        if (want[0].size()) {
            Heap less(want[0].size() - 1);
            memset(less.p, 0xA5, less.n);
            u8 *const out2[3] = {less.p, o1.p, o2.p};
            const u64 cap2[3] = {less.n, o1.n, o2.n};
            r = bfq_bam_host(stream.p, stream.n, O, out2, cap2, false, ol, nr, &S, &E, &G, &TS);
            CHECK(r == 2 && all_a5(less) && ol[0] == want[0].size(), "%s: a short buffer: %d", sname, r);
        }
        // without the extension: what it gave before (the lengths differ by the tags' bytes)
        u64 pl[3];
        r = bfq_bam_host(stream.p, stream.n, O, none, zero, true, pl, nr, &S, &E);
        CHECK(r == 0 && pl[0] + pl[1] + pl[2] + wc[2] == want[0].size() + want[1].size() + want[2].size(), "%s: the untagged lengths", sname);
    } else {
        const std::vector<u8> msg = slurp(msgName);
        const std::string wantMsg(msg.begin(), msg.end());
        Heap o0(1 << 18), o1(1 << 18), o2(1 << 18);
        memset(o0.p, 0xA5, o0.n); memset(o1.p, 0xA5, o1.n); memset(o2.p, 0xA5, o2.n);
        u8 *const out[3] = {o0.p, o1.p, o2.p};
        const u64 cap[3] = {o0.n, o1.n, o2.n};
        const int r = bfq_bam_host(stream.p, stream.n, O, out, cap, false, ol, nr, &S, &E, &G, &TS);
        const std::string got = r == 1 ? bfq_bam_message(E) : std::string("not refused");
        CHECK(r == 1 && got == wantMsg, "%s: got %d \"%s\", expected \"%s\"", sname, r, got.c_str(), wantMsg.c_str());
        CHECK(all_a5(o0) && all_a5(o1) && all_a5(o2), "%s: a refusal wrote", sname);
        CHECK(bfq_bam_host(stream.p, stream.n, O, none, zero, true, ol, nr, &S, &E) == 0, "%s: refused with tags off", sname);
    }
}

static void way_out(FILE *mf)
{
    char t[3][1024], sel[256], rname[1024], wname[1024];
    unsigned paired;
    unsigned long long wc[4];
    if (fscanf(mf, "%1023s %1023s %1023s %255s %u %1023s %1023s %llu %llu %llu %llu", t[0], t[1], t[2], sel, &paired, rname, wname, &wc[0], &wc[1], &wc[2], &wc[3]) != 11)
        exit(2);
    Heap *h[3] = {nullptr, nullptr, nullptr};
    const u8 *p[3] = {nullptr, nullptr, nullptr};
    u64 n[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {
        if (!strcmp(t[k], "-")) continue;
        const std::vector<u8> v = slurp(t[k]);
        h[k] = new Heap(v.data(), v.size());
        p[k] = h[k]->p; n[k] = v.size();
    }
    std::vector<u8> rg;
    if (strcmp(rname, "-")) rg = slurp(rname);
    rg.push_back(0);
    bfq_ubam_tag_opts X{};
    bfq_ubam_defaults(&X.o);
    X.o.paired_check = paired; X.o.reserved = BFQ_UBAM_OPTS_TAGS;
    if (strcmp(rname, "-")) X.o.rg_id = (const char *)rg.data();
    select(sel, &X);
    bfq_ubam_opts O;
    bfq_ubam_err E;
    bfq_ubam_tagsel G;
    bfq_ubam_tag_stats *where = nullptr, TS{};
    const char *why = nullptr;
    CHECK(bfq_ubam_resolve(&X.o, &O, &E) && bfq_ubam_tags_resolve(&X.o, &G, &where, &why) && G.on, "%s: options refused", wname);
    const std::vector<u8> want = slurp(wname);
    bfq_ubam_stats S;
    int r = bfq_ubam_host_form(p, n, O, nullptr, 0, true, &S, &E, &G, &TS);
    CHECK(r == 0 && S.raw_len == want.size(), "%s: measure: %d: %s", wname, r, bfq_ubam_message(E).c_str());
    Heap out(want.size());
    memset(out.p, 0xA5, out.n);
    TS = bfq_ubam_tag_stats{};
    r = bfq_ubam_host_form(p, n, O, out.p, out.n, false, &S, &E, &G, &TS);
    CHECK(r == 0, "%s: %d: %s", wname, r, bfq_ubam_message(E).c_str());
    CHECK(!memcmp(out.p, want.data(), want.size()), "%s: the stream differs", wname);
    CHECK(S.comments_dropped == wc[0] && TS.tags_written == wc[1] && TS.fields_dropped == wc[2] && TS.tag_bytes == wc[3] && S.raw_len == want.size(),
          "%s: the counts differ: %llu %llu %llu %llu", wname, S.comments_dropped, TS.tags_written, TS.fields_dropped, TS.tag_bytes);
    if (want.size()) {
        Heap less(want.size() - 1);
        memset(less.p, 0xA5, less.n);
        r = bfq_ubam_host_form(p, n, O, less.p, less.n, false, &S, &E, &G, &TS);
        CHECK(r == 3 && all_a5(less), "%s: a short buffer: %d", wname, r);
    }
    for (int k = 0; k < 3; k++) delete h[k];
}

int main(int argc, char **argv)
{
    if (argc != 2) { printf("usage: test_bam_tags MANIFEST\n"); return 2; }
    FILE *mf = fopen(argv[1], "r");
    if (!mf) { printf("cannot open %s\n", argv[1]); return 2; }
    char kind[16];
    int cases = 0;
    while (fscanf(mf, "%15s", kind) == 1) {
        cases++;
        if (!strcmp(kind, "in")) way_in(mf, true);
        else if (!strcmp(kind, "inbad")) way_in(mf, false);
        else if (!strcmp(kind, "out")) way_out(mf);
        else { printf("unknown case kind %s\n", kind); return 2; }
    }
    fclose(mf);
    printf("%d cases, %d failures\n", cases, g_fail);
    return g_fail || !cases ? 1 : 0;
}
