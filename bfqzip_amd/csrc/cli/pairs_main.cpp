// pairs_main.cpp -- interleaved paired FASTQ on the GPU (not a tool of the reference, whose paired runs take two files): one
// file with the mates alternating (bwa mem -p, fastp --interleaved_in, samtools fastq without -1 -2) split into the two files
// of mates, and back (include/bfqzip_hip.h, bfq_fastq_deinterleave_fd / bfq_fastq_interleave_fd; the definition:
// csrc/bfq_pairs.h).  Records move byte for byte.
//     bfq_pairs -s IN.fq -1 A.fq -2 B.fq [-0 S.fq] [-O] [-n] [-k] [-g] [-V]      split
//     bfq_pairs -m -1 A.fq -2 B.fq [-0 S.fq] -o OUT.fq [-n] [-k] [-g] [-V]       merge
//     bfq_pairs -t IN.fq [-O] [-n] [-k] [-g]                                     measure only: records, pairs, singles
//     bfq_pairs -r [-1 A.fq] [-2 B.fq] [-0 MIXED.fq] -A OUT_1.fq -B OUT_2.fq [-S SINGLES.fq] [-k] [-g] [-V]
//                                                                                repair: the mates matched by name, wherever
//                                                                                they stand (bfq_fastq_repair_fd)
//     bfq_pairs -r -t [-1 A.fq] [-2 B.fq] [-0 MIXED.fq] [-k] [-g]                count only; exit 1 when there are singletons
//   -r  -1 and -2 are mate files that may each have lost reads, in any order; -0 is a mixed file whose /1 and /2 say which
//       mate a record is (without them equal names are paired two by two).  Pairs go to -A and -B in the order of their
//       first mates, what finds no mate to -S; singletons without -S are refused before anything is written
//   -O  orphan mode: the records of every run of equal names are paired, what is left over goes to -0 (without -0 the
//       singletons are counted and dropped)
//   -n  the names of the mates are not compared; -k keeps a trailing /1 or /2 in the name that is compared
//   -g  a compressed input is plain gzip (bfq_gzip_inflate_fd); without it a compressed input is BGZF (bfq_bgzf_inflate_fd).
//       An input that begins with 1f 8b is inflated into an unnamed temporary file first ($TMPDIR, /tmp), as bfq_bgzf -d does.
// Exit status 0 on success; 1 with the library's message when the file is not properly paired or damaged, and then the
// output files are left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -s IN.fq -1 A.fq -2 B.fq [-0 S.fq] [-O] [-n] [-k] [-g] [-V]\n"
                    "       %s -m -1 A.fq -2 B.fq [-0 S.fq] -o OUT.fq [-n] [-k] [-g] [-V]\n"
                    "       %s -t IN.fq [-O] [-n] [-k] [-g]\n"
                    "       %s -r [-t] [-1 A.fq] [-2 B.fq] [-0 MIXED.fq] -A OUT_1.fq -B OUT_2.fq [-S SINGLES.fq] [-k] [-g] [-V]\n"
                    "  -s <arg>  interleaved FASTQ to split into -1 and -2\n"
                    "  -m        merge -1 and -2 (and the reads of -0 behind the pairs) into -o\n"
                    "  -t <arg>  measure only: print records, pairs and singles; exit 1 when the file is not properly paired\n"
                    "  -r        repair: match the mates of -1, -2 and -0 by name; pairs to -A and -B, the rest to -S (-t: count only)\n"
                    "  -O        orphan mode: pair the records of every run of equal names, the rest to -0\n"
                    "  -n        do not compare the names of the mates\n"
                    "  -k        keep a trailing /1 or /2 in the names that are compared\n"
                    "  -g        a compressed input is plain gzip (default: BGZF)\n"
                    "  -V        phase timeline on stderr\n", argv0, argv0, argv0, argv0);
    return 1;
}

// -r: the repair.  Returns the exit status.
static int repair_main(int argc, char **argv)
{
    std::string in[3], outName[3];
    bool gzip = false, count = false;
    bfq_repair_opts O;
    bfq_repair_default_opts(&O);
    int opt;
    while ((opt = getopt(argc, argv, "rt0:1:2:A:B:S:kgVh")) != -1) {
        switch (opt) {
        case 'r': break;
        case 't': count = true; break;
        case '0': case '1': case '2': in[opt - '0'] = optarg; break;
        case 'A': outName[1] = optarg; break;
        case 'B': outName[2] = optarg; break;
        case 'S': outName[0] = optarg; break;
        case 'k': O.mate_suffix = 0; break;
        case 'g': gzip = true; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    const bool anyOut = !outName[0].empty() || !outName[1].empty() || !outName[2].empty();
    if (optind != argc || (in[0].empty() && in[1].empty() && in[2].empty())) return usage(argv[0]);
    if (count ? anyOut : (outName[1].empty() || outName[2].empty())) return usage(argv[0]);
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_pairs", &P);
    if (!c) return 1;
    bfq_repair_stats st = {};
    uint64_t outLen[3] = {0, 0, 0}, nReads[3] = {0, 0, 0};
    OutFile out[3];
    auto fail = [&] {                                               // the outputs are left empty
        for (int k = 0; k < 3; k++)
            if (out[k].fd >= 0 && ftruncate(out[k].fd, 0) != 0) perror("bfq_pairs");
        bfq_destroy(c);
        return 1;
    };
    {
        TextFile text[3];
        for (int k = 0; k < 3; k++)
            if (!in[k].empty() && !text[k].open(c, "bfq_pairs", in[k], gzip)) return fail();
        int rc = 0;
        if (count || outName[0].empty()) {                          // the counts first: singletons need a place before anything is written
            void *m[3] = {MAP_FAILED, MAP_FAILED, MAP_FAILED};
            const uint8_t *tp[3] = {nullptr, nullptr, nullptr};
            uint64_t tn[3] = {0, 0, 0};
            static const uint8_t none = 0;
            for (int k = 0; k < 3; k++) {
                if (text[k].fd < 0) continue;
                tp[k] = &none;
                if (!text[k].size) continue;
                m[k] = mmap(nullptr, text[k].size, PROT_READ, MAP_PRIVATE, text[k].fd, 0);
                if (m[k] == MAP_FAILED) { perror("bfq_pairs"); return fail(); }
                tp[k] = (const uint8_t *)m[k]; tn[k] = text[k].size;
            }
            rc = bfq_fastq_repair_measure(c, tp, tn, &O, outLen, nReads, &st);
            for (int k = 0; k < 3; k++)
                if (m[k] != MAP_FAILED) munmap(m[k], text[k].size);
            if (!rc && !count && st.singles) {
                fprintf(stderr, "bfq_pairs: FASTQ repair: %llu singletons and no -S file\n", (unsigned long long)st.singles);
                return fail();
            }
        }
        if (!rc && !count) {
            for (int k = 0; k < 3; k++)
                if (!outName[k].empty() && !out[k].open(outName[k])) { perror("bfq_pairs"); return fail(); }
            const int ifd[3] = {text[0].fd, text[1].fd, text[2].fd}, ofd[3] = {out[0].fd, out[1].fd, out[2].fd};
            rc = bfq_fastq_repair_fd(c, ifd, &O, ofd, outLen, nReads, &st);
        }
        if (rc) {
            fprintf(stderr, "bfq_pairs: %s\n", bfq_last_error(c));
            return fail();
        }
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_pairs");
    bool closed = true;
    for (int k = 0; k < 3; k++) closed = out[k].close() && closed;
    bfq_destroy(c);
    if (!closed) { perror("bfq_pairs"); return 1; }
    bfq_phase_report("bfq_pairs");
    printf("%llu records: %llu pairs, %llu singles (%llu names more than twice)\n", (unsigned long long)st.records, (unsigned long long)st.pairs,
           (unsigned long long)st.singles, (unsigned long long)st.dup_groups);
    return count && st.singles ? 1 : 0;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    for (int k = 1; k < argc; k++)
        if (!strcmp(argv[k], "-r")) return repair_main(argc, argv);
    std::string input, output, mate[3];
    char mode = 0;
    int opt;
    bool gzip = false;
    bfq_pairs_opts O;
    bfq_pairs_default_opts(&O);
    while ((opt = getopt(argc, argv, "s:mt:0:1:2:o:OnkgVh")) != -1) {
        switch (opt) {
        case 's': case 't':
            if (mode) return usage(argv[0]);
            mode = (char)opt; input = optarg; break;
        case 'm':
            if (mode) return usage(argv[0]);
            mode = 'm'; break;
        case '0': case '1': case '2': mate[opt - '0'] = optarg; break;
        case 'o': output = optarg; break;
        case 'O': O.orphans = 1; break;
        case 'n': O.check_names = 0; break;
        case 'k': O.mate_suffix = 0; break;
        case 'g': gzip = true; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    const bool mates = !mate[1].empty() && !mate[2].empty();
    if (!mode || optind != argc) return usage(argv[0]);
    if (mode == 's' && (!mates || !output.empty())) return usage(argv[0]);
    if (mode == 'm' && (!mates || output.empty() || O.orphans)) return usage(argv[0]);
    if (mode == 't' && (!output.empty() || !mate[0].empty() || !mate[1].empty() || !mate[2].empty())) return usage(argv[0]);
    OutFile out[3], merged;
    if (mode == 's')
        for (int k = 0; k < 3; k++)
            if (!mate[k].empty() && !out[k].open(mate[k])) { perror("bfq_pairs"); return 1; }
    if (mode == 'm' && !merged.open(output)) { perror("bfq_pairs"); return 1; }
    auto fail = [&] {                                               // the outputs are left empty
        for (int k = 0; k < 3; k++)
            if (out[k].fd >= 0 && ftruncate(out[k].fd, 0) != 0) perror("bfq_pairs");
        if (merged.fd >= 0 && ftruncate(merged.fd, 0) != 0) perror("bfq_pairs");
        return 1;
    };
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_pairs", &P);
    if (!c) return fail();
    bfq_pairs_stats st = {};
    uint64_t outLen[3] = {0, 0, 0}, nReads[3] = {0, 0, 0}, total = 0;
    int rc = 0;
    {
        TextFile text[3];
        bool ok = true;
        if (mode == 'm') {
            for (int k = 0; k < 3 && ok; k++)
                if (!mate[k].empty()) ok = text[k].open(c, "bfq_pairs", mate[k], gzip);
        } else ok = text[0].open(c, "bfq_pairs", input, gzip);
        if (!ok) { bfq_destroy(c); return fail(); }
        if (mode == 's') {
            const int fds[3] = {out[0].fd, out[1].fd, out[2].fd};
            rc = bfq_fastq_deinterleave_fd(c, text[0].fd, text[0].size, &O, fds, outLen, nReads, &st);
        } else if (mode == 'm') {
            const int fds[3] = {text[0].fd, text[1].fd, text[2].fd};
            rc = bfq_fastq_interleave_fd(c, fds, &O, merged.fd, &total, &st);
        } else {
            void *m = text[0].size ? mmap(nullptr, text[0].size, PROT_READ, MAP_PRIVATE, text[0].fd, 0) : MAP_FAILED;
            if (text[0].size && m == MAP_FAILED) { perror("bfq_pairs"); bfq_destroy(c); return 1; }
            rc = bfq_fastq_deinterleave_measure(c, m != MAP_FAILED ? (const uint8_t *)m : nullptr, m != MAP_FAILED ? text[0].size : 0, &O, outLen, nReads, &st);
            if (m != MAP_FAILED) munmap(m, text[0].size);
        }
    }
    if (rc) {
        fprintf(stderr, "bfq_pairs: %s: %s\n", mode == 'm' ? output.c_str() : input.c_str(), bfq_last_error(c));
        bfq_destroy(c);
        return fail();
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_pairs");
    bool closed = merged.close();
    for (int k = 0; k < 3; k++) closed = out[k].close() && closed;
    bfq_destroy(c);
    if (!closed) { perror("bfq_pairs"); return 1; }
    bfq_phase_report("bfq_pairs");
    if (mode == 'm')
        printf("%llu records: %llu pairs, %llu singles -> %llu bytes\n", (unsigned long long)st.records, (unsigned long long)st.pairs,
               (unsigned long long)st.singles, (unsigned long long)total);
    else
        printf("%llu records: %llu pairs, %llu singles%s\n", (unsigned long long)st.records, (unsigned long long)st.pairs, (unsigned long long)st.singles,
               mode == 's' && st.singles && mate[0].empty() ? " (dropped: no -0)" : "");
    return 0;
}
