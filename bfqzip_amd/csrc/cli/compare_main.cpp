// compare_main.cpp -- what a run did to the data: a FASTQ file against the FASTQ file that came out, compared on the GPU
// (include/bfqzip_hip.h, bfq_fastq_compare_fd).  The reference leaves the question to a bwa + GATK pipeline downstream.
//     bfq_compare -a A.fq -b B.fq [-P RUN.perm] [-n K] [-o REPORT.json] [-V]
// A is "before", B "after"; -P: B is in the order of a reordered run whose permutation was kept (bfq_reorder -P,
// parallel.py --keep-order), record j of B is compared with record perm[j] of A.  -n K lists the first K differing
// positions.  The report is JSON (the keys of bfqzip_amd.api.CompareReport.as_dict(), "diffs" with -n) on stdout or in -o.
// Exit status as cmp's: 0 the payloads (bases and qualities) are identical, 1 they differ, 2 an error, with the library's message.
#include <unistd.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -a A.fq -b B.fq [-P RUN.perm] [-n K] [-o REPORT.json] [-V]\n"
                    "  -a <arg>  the FASTQ before the run (REQUIRED)\n"
                    "  -b <arg>  the FASTQ after the run (REQUIRED)\n"
                    "  -P <arg>  BFQPERM1 file of the run that gave B its order: record j of B pairs with record perm[j] of A\n"
                    "  -n <arg>  list the first K differing positions (def. 0)\n"
                    "  -o <arg>  write the JSON report there (def. stdout)\n"
                    "  -V        phase timeline on stderr\n"
                    "exit status: 0 bases and qualities identical, 1 they differ, 2 error\n", argv0);
    return 2;
}

static void put_array(std::string &s, const char *key, const uint64_t *v, size_t n)
{
    char b[32];
    s += std::string("\"") + key + "\": [";
    for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, i ? ", %llu" : "%llu", (unsigned long long)v[i]); s += b; }
    s += "]";
}

// the keys and the order of CompareReport.as_dict() (bfqzip_amd/api.py)
static std::string report_json(const bfq_compare_report &R, const bfq_compare_diff *diffs, uint64_t ndiffs, bool withDiffs)
{
    static const char *const scalars[] = {"n_reads", "total_bases", "n_diffs", "reads_changed", "reads_bases_changed", "reads_quals_changed",
                                          "bases_changed", "quals_changed", "quals_raised", "quals_lowered", "qual_abs_sum", "qual_sq_sum",
                                          "qual_abs_max", "first_changed_read", "headers_same", "headers_dropped", "headers_changed"};
    const uint64_t *f = &R.n_reads;                               // the 17 scalar fields stand in this order at the head of the struct
    std::string s = "{";
    char b[96];
    for (size_t i = 0; i < sizeof scalars / sizeof *scalars; i++) {
        if (i == 13 && f[i] == UINT64_MAX) snprintf(b, sizeof b, "\"%s\": null, ", scalars[i]);
        else snprintf(b, sizeof b, "\"%s\": %llu, ", scalars[i], (unsigned long long)f[i]);
        s += b;
    }
    s += R.n_diffs ? "\"identical\": false, " : "\"identical\": true, ";
    s += "\"subst\": [";
    for (int a = 0; a < BFQ_CMP_SYMS; a++) {
        s += a ? ", [" : "[";
        for (int k = 0; k < BFQ_CMP_SYMS; k++) { snprintf(b, sizeof b, k ? ", %llu" : "%llu", (unsigned long long)R.subst[BFQ_CMP_SYMS * a + k]); s += b; }
        s += "]";
    }
    s += "], ";
    put_array(s, "qual_hist_a", R.qual_hist_a, 256); s += ", ";
    put_array(s, "qual_hist_b", R.qual_hist_b, 256); s += ", ";
    put_array(s, "changed_base_qual_hist", R.changed_base_qual_hist, 256); s += ", ";
    size_t np = BFQ_CMP_POS;                                      // the profiles end with the last bin that holds a position
    while (np && !R.pos_len[np - 1]) np--;
    put_array(s, "pos_len", R.pos_len, np); s += ", ";
    put_array(s, "pos_bases", R.pos_bases, np); s += ", ";
    put_array(s, "pos_quals", R.pos_quals, np); s += ", ";
    put_array(s, "pos_abs", R.pos_abs, np);
    if (withDiffs) {
        s += ", \"diffs\": [";
        for (uint64_t i = 0; i < ndiffs; i++) {
            snprintf(b, sizeof b, "%s[%llu, %u, %u, %u, %u, %u]", i ? ", " : "", (unsigned long long)diffs[i].read, diffs[i].pos, diffs[i].base_a,
                     diffs[i].base_b, diffs[i].qual_a, diffs[i].qual_b);
            s += b;
        }
        s += "]";
    }
    s += "}\n";
    return s;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string a, b, perm, out;
    uint64_t K = 0;
    int opt;
    while ((opt = getopt(argc, argv, "a:b:P:n:o:Vh")) != -1) {
        switch (opt) {
        case 'a': a = optarg; break;
        case 'b': b = optarg; break;
        case 'P': perm = optarg; break;
        case 'n': K = strtoull(optarg, nullptr, 10); break;
        case 'o': out = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    if (a.empty() || b.empty()) return usage(argv[0]);
    InFile fa, fb, fp;
    if (!fa.open(a)) { fprintf(stderr, "bfq_compare: cannot read %s\n", a.c_str()); return 2; }
    if (!fb.open(b)) { fprintf(stderr, "bfq_compare: cannot read %s\n", b.c_str()); return 2; }
    if (!perm.empty() && !fp.open(perm)) { fprintf(stderr, "bfq_compare: cannot read %s\n", perm.c_str()); return 2; }
    const uint64_t cap = K < fa.size / 2 ? K : fa.size / 2;       // a text of n bytes has at most n / 2 bases
    std::vector<bfq_compare_diff> diffs(cap);
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_compare", &P);
    if (!c) return 2;
    bfq_compare_report R;
    const int rc = bfq_fastq_compare_fd(c, fa.fd, fa.size, fb.fd, fb.size, perm.empty() ? -1 : fp.fd, fp.size, &R, cap ? diffs.data() : nullptr, cap);
    if (rc) {
        fprintf(stderr, "bfq_compare: %s\n", bfq_last_error(c));
        bfq_destroy(c);
        return 2;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_compare");
    bfq_destroy(c);
    const std::string js = report_json(R, diffs.data(), R.n_diffs < cap ? R.n_diffs : cap, K > 0);
    if (out.empty()) fwrite(js.data(), 1, js.size(), stdout);
    else if (!write_file(out, js.data(), js.size())) { fprintf(stderr, "bfq_compare: cannot write %s\n", out.c_str()); return 2; }
    bfq_phase_report("bfq_compare");
    return R.n_diffs ? 1 : 0;
}
