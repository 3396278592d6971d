// kmers_main.cpp -- which k-mers a run removed, kept and created: the k-mer spectrum of a FASTQ file, or of the file before a
// run against the file that came out, counted on the GPU (include/bfqzip_hip.h, bfq_fastq_kmers_fd).
//     bfq_kmers -a IN.fq [-b OUT.fq] [-k K] [-s SOLID] [-f] [-n LIST] [-o REPORT.json] [-V]
// Nothing is paired: the order of the reads does not matter, no permutation file is needed after a reordered run.  -f counts
// forward k-mers instead of canonical ones.  -n LIST lists the first LIST k-mers that went solid -> absent or absent -> solid,
// as ACGT strings with their two counts.  The report is JSON (the keys of bfqzip_amd.api.KmerReport.as_dict()) on stdout or
// in -o.  Exit status as cmp's: 0 no k-mer's count differs between A and B (always, without -b), 1 some do, 2 an error, with
// the library's message.
#include <unistd.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -a IN.fq [-b OUT.fq] [-k K] [-s SOLID] [-f] [-n LIST] [-o REPORT.json] [-V]\n"
                    "  -a <arg>  the FASTQ before the run, or the only one (REQUIRED)\n"
                    "  -b <arg>  the FASTQ after the run\n"
                    "  -k <arg>  k-mer length, 8..31 (def. 21)\n"
                    "  -s <arg>  a k-mer is solid from this count on, 2..15 (def. 3)\n"
                    "  -f        forward k-mers, not canonical ones\n"
                    "  -n <arg>  list the first LIST k-mers that went solid -> absent or absent -> solid (def. 0)\n"
                    "  -o <arg>  write the JSON report there (def. stdout)\n"
                    "  -V        phase timeline on stderr\n"
                    "exit status: 0 no k-mer's count differs, 1 some do, 2 error\n", argv0);
    return 2;
}

static void put_array(std::string &s, const char *key, const uint64_t *v, size_t n)
{
    char b[32];
    s += std::string("\"") + key + "\": [";
    for (size_t i = 0; i < n; i++) { snprintf(b, sizeof b, i ? ", %llu" : "%llu", (unsigned long long)v[i]); s += b; }
    s += "]";
}

// the keys and the order of KmerReport.as_dict() (bfqzip_amd/api.py)
static std::string report_json(const bfq_kmer_report &R, const bfq_kmer_entry *list, uint64_t nlist)
{
    static const char *const scalars[] = {"k", "solid", "canonical", "n_partitions", "n_reads_a", "n_reads_b", "reads_short_a", "reads_short_b",
                                          "windows_a", "windows_b", "windows_skipped_a", "windows_skipped_b", "distinct_a", "distinct_b",
                                          "distinct_both", "only_a", "only_b", "occ_only_a", "occ_only_b", "distinct_changed", "n_listed"};
    const uint64_t *f = &R.k;                                     // the 21 scalar fields stand in this order at the head of the struct
    std::string s = "{";
    char b[160];
    for (size_t i = 0; i < sizeof scalars / sizeof *scalars; i++) { snprintf(b, sizeof b, "\"%s\": %llu, ", scalars[i], (unsigned long long)f[i]); s += b; }
    put_array(s, "hist_a", R.hist_a, 256); s += ", ";
    put_array(s, "hist_b", R.hist_b, 256); s += ", ";
    put_array(s, "joint", R.joint, 256); s += ", ";
    put_array(s, "trans", R.trans, 9);
    s += ", \"list\": [";
    for (uint64_t i = 0; i < nlist; i++) {
        char km[32];
        for (uint32_t j = 0; j < R.k; j++) km[j] = "ACGT"[(list[i].kmer >> (2 * (R.k - 1 - j))) & 3];
        km[R.k] = 0;
        snprintf(b, sizeof b, "%s[\"%s\", %u, %u]", i ? ", " : "", km, list[i].count_a, list[i].count_b);
        s += b;
    }
    s += "]}\n";
    return s;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string a, b, out;
    bfq_kmer_opts O = {21, 3, 1, 0, 0};
    uint64_t K = 0;
    int opt;
    while ((opt = getopt(argc, argv, "a:b:k:s:fn:o:Vh")) != -1) {
        switch (opt) {
        case 'a': a = optarg; break;
        case 'b': b = optarg; break;
        case 'k': O.k = (uint32_t)strtoul(optarg, nullptr, 10); break;
        case 's': O.solid = (uint32_t)strtoul(optarg, nullptr, 10); break;
        case 'f': O.canonical = 0; break;
        case 'n': K = strtoull(optarg, nullptr, 10); break;
        case 'o': out = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    if (a.empty()) return usage(argv[0]);
    InFile fa, fb;
    if (!fa.open(a)) { fprintf(stderr, "bfq_kmers: cannot read %s\n", a.c_str()); return 2; }
    if (!b.empty() && !fb.open(b)) { fprintf(stderr, "bfq_kmers: cannot read %s\n", b.c_str()); return 2; }
    const uint64_t most = (fa.size + (b.empty() ? 0 : fb.size)) / 2, cap = K < most ? K : most;   // a text of n bytes has at most n / 2 windows
    std::vector<bfq_kmer_entry> list(cap);
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_kmers", &P);
    if (!c) return 2;
    bfq_kmer_report R;
    const int rc = bfq_fastq_kmers_fd(c, fa.fd, fa.size, b.empty() ? -1 : fb.fd, b.empty() ? 0 : fb.size, &O, &R, cap ? list.data() : nullptr, cap);
    if (rc) {
        fprintf(stderr, "bfq_kmers: %s\n", bfq_last_error(c));
        bfq_destroy(c);
        return 2;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_kmers");
    bfq_destroy(c);
    const std::string js = report_json(R, list.data(), R.n_listed < cap ? R.n_listed : cap);
    if (out.empty()) fwrite(js.data(), 1, js.size(), stdout);
    else if (!write_file(out, js.data(), js.size())) { fprintf(stderr, "bfq_kmers: cannot write %s\n", out.c_str()); return 2; }
    bfq_phase_report("bfq_kmers");
    return !b.empty() && R.distinct_changed ? 1 : 0;
}
