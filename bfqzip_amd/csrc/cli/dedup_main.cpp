// dedup_main.cpp -- exact duplicate removal of FASTQ reads and pairs on the GPU (not a tool of the reference): what clumpify
// dedupe, fastuniq, seqkit rmdup -s and fastp --dedup do (include/bfqzip_hip.h, bfq_fastq_dedup_fd; the definition:
// csrc/bfq_dedup.h).  Reads, or pairs, with equal sequences leave one unit behind; records move byte for byte and the kept
// ones stay in input order.
//     bfq_dedup -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-D DUPS.fq [-E DUPS_2.fq]] [-q] [-g] [-r REPORT.json] [-V]
//     bfq_dedup -t -i IN.fq [-j IN_2.fq] [-q] [-g] [-r REPORT.json]              count only, nothing written
//   -j  the second mates: the k-th records of -i and -j are one unit, equal when both sequences are
//   -q  keep the unit with the best qualities of every group (default: the first)
//   -D  -E  the removed records go here, in input order (without them they are counted and dropped)
//   -g  a compressed input is plain gzip (bfq_gzip_inflate_fd); without it a compressed input is BGZF (bfq_bgzf_inflate_fd).
//       An input that begins with 1f 8b is inflated into an unnamed temporary file first ($TMPDIR, /tmp).
//   -r  the statistics as JSON: units, kept, removed, dup_groups, max_group, max_group_first, the duplication levels
// Exit status, as cmp's: 0 when nothing was removed, 1 when duplicates were found, 2 on an error -- then with the library's
// message, and the output files are left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-D DUPS.fq [-E DUPS_2.fq]] [-q] [-g] [-r REPORT.json] [-V]\n"
                    "       %s -t -i IN.fq [-j IN_2.fq] [-q] [-g] [-r REPORT.json]\n"
                    "  -i <arg>  FASTQ: the reads, or the first mates\n"
                    "  -j <arg>  the second mates: record k of -i and of -j are one unit\n"
                    "  -o <arg>  the kept records of -i (-p: of -j)\n"
                    "  -D <arg>  the removed records of -i (-E: of -j)\n"
                    "  -q        keep the best qualities of every group (default: the first unit)\n"
                    "  -t        count only\n"
                    "  -g        a compressed input is plain gzip (default: BGZF)\n"
                    "  -r <arg>  the statistics as JSON\n"
                    "  -V        phase timeline on stderr\n", argv0, argv0);
    return 2;
}

static bool write_report(const std::string &path, const bfq_dedup_stats &st, bool paired, uint32_t keep)
{
    std::string s = "{\"paired\": " + std::to_string(paired ? 1 : 0) + ", \"keep\": " + std::to_string(keep);
    auto put = [&](const char *k, uint64_t v) { s += std::string(", \"") + k + "\": " + std::to_string(v); };
    put("units", st.units); put("kept", st.kept); put("removed", st.removed); put("dup_groups", st.dup_groups); put("max_group", st.max_group);
    put("max_group_first", st.max_group_first); put("mixed_runs", st.mixed_runs); put("max_run", st.max_run); put("rounds", st.rounds);
    auto list = [&](const char *k, const uint64_t *v, int n) {
        s += std::string(", \"") + k + "\": [";
        for (int j = 0; j < n; j++) s += (j ? ", " : "") + std::to_string(v[j]);
        s += "]";
    };
    list("out_len", st.out_len, 2); list("dup_len", st.dup_len, 2); list("level_groups", st.level_groups, 32); list("level_units", st.level_units, 32);
    s += "}\n";
    return write_file(path, s.data(), s.size());
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string in[2], outName[4], report;
    bool gzip = false, count = false;
    bfq_dedup_opts O;
    bfq_dedup_default_opts(&O);
    int opt;
    while ((opt = getopt(argc, argv, "i:j:o:p:D:E:qtgr:Vh")) != -1) {
        switch (opt) {
        case 'i': in[0] = optarg; break;
        case 'j': in[1] = optarg; break;
        case 'o': outName[0] = optarg; break;
        case 'p': outName[1] = optarg; break;
        case 'D': outName[2] = optarg; break;
        case 'E': outName[3] = optarg; break;
        case 'q': O.keep = 1; break;
        case 't': count = true; break;
        case 'g': gzip = true; break;
        case 'r': report = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    const bool paired = !in[1].empty(), anyOut = !outName[0].empty() || !outName[1].empty() || !outName[2].empty() || !outName[3].empty();
    if (optind != argc || in[0].empty()) return usage(argv[0]);
    if (count ? anyOut : (outName[0].empty() || outName[1].empty() == paired || (!outName[3].empty() && (!paired || outName[2].empty())) ||
                          (paired && !outName[2].empty() && outName[3].empty())))
        return usage(argv[0]);
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_dedup", &P);
    if (!c) return 2;
    bfq_dedup_stats st = {};
    uint64_t outLen[2] = {0, 0}, dupLen[2] = {0, 0};
    OutFile out[4];
    auto fail = [&] {                                               // the outputs are left empty
        for (int k = 0; k < 4; k++)
            if (out[k].fd >= 0 && ftruncate(out[k].fd, 0) != 0) perror("bfq_dedup");
        bfq_destroy(c);
        return 2;
    };
    {
        TextFile text[2];
        for (int k = 0; k < 2; k++)
            if (!in[k].empty() && !text[k].open(c, "bfq_dedup", in[k], gzip)) return fail();
        int rc = 0;
        if (count) {
            void *m[2] = {MAP_FAILED, MAP_FAILED};
            const uint8_t *tp[2] = {nullptr, nullptr};
            uint64_t tn[2] = {0, 0};
            static const uint8_t none = 0;
            for (int k = 0; k < 2; k++) {
                if (text[k].fd < 0) continue;
                tp[k] = &none;
                if (!text[k].size) continue;
                m[k] = mmap(nullptr, text[k].size, PROT_READ, MAP_PRIVATE, text[k].fd, 0);
                if (m[k] == MAP_FAILED) { perror("bfq_dedup"); return fail(); }
                tp[k] = (const uint8_t *)m[k]; tn[k] = text[k].size;
            }
            rc = bfq_fastq_dedup_measure(c, tp, tn, &O, outLen, dupLen, &st);
            for (int k = 0; k < 2; k++)
                if (m[k] != MAP_FAILED) munmap(m[k], text[k].size);
        } else {
            for (int k = 0; k < 4; k++)
                if (!outName[k].empty() && !out[k].open(outName[k])) { perror("bfq_dedup"); return fail(); }
            const int ifd[2] = {text[0].fd, text[1].fd}, ofd[2] = {out[0].fd, out[1].fd}, dfd[2] = {out[2].fd, out[3].fd};
            rc = bfq_fastq_dedup_fd(c, ifd, &O, ofd, dfd, outLen, dupLen, &st);
        }
        if (rc) {
            fprintf(stderr, "bfq_dedup: %s\n", bfq_last_error(c));
            return fail();
        }
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_dedup");
    bool closed = true;
    for (int k = 0; k < 4; k++) closed = out[k].close() && closed;
    bfq_destroy(c);
    if (!closed) { perror("bfq_dedup"); return 2; }
    if (!report.empty() && !write_report(report, st, paired, O.keep)) { fprintf(stderr, "bfq_dedup: cannot write %s\n", report.c_str()); return 2; }
    bfq_phase_report("bfq_dedup");
    printf("%llu %s: %llu kept, %llu removed (%llu groups of duplicates, the largest of %llu at record %llu)\n", (unsigned long long)st.units,
           paired ? "pairs" : "reads", (unsigned long long)st.kept, (unsigned long long)st.removed, (unsigned long long)st.dup_groups,
           (unsigned long long)st.max_group, (unsigned long long)st.max_group_first);
    return st.removed ? 1 : 0;
}
