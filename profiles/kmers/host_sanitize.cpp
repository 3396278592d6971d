// host_sanitize.cpp -- the host form of the k-mer report under the sanitizers, as a stand-alone program (the library's host
// code is not checked while loaded into python).  Build and run from the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ibfqzip_amd/csrc \
//       profiles/kmers/host_sanitize.cpp bfqzip_amd/csrc/bfq_kmers_host.cpp bfqzip_amd/csrc/bfq_host.cpp -lpthread -o /tmp/kmers_host_san
//   /tmp/kmers_host_san tests/golden
// For each golden pair NAME.fastq / NAME.M2B0.fq and k in {8, 20, 21, 31}, canonical and forward, A against B and A alone,
// with a list of 100 entries behind which a guard must stay intact; then the refusals (k, solid, a cut text).  Prints one line
// per golden and k (the numbers of profiles/kmers/README.md's table); exit 0 when every call did what it should.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/bfqzip_hip.h"

static std::vector<uint8_t> slurp(const std::string &p)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", p.c_str()); exit(2); }
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "tests/golden";
    const char *names[] = {"example", "paired", "synth_fix", "synth_var"};
    const uint32_t ks[] = {8, 20, 21, 31};
    int bad = 0;
    for (const char *name : names) {
        const std::vector<uint8_t> a = slurp(dir + "/" + name + ".fastq"), b = slurp(dir + "/" + name + ".M2B0.fq");
        for (uint32_t k : ks)
            for (uint32_t canonical = 0; canonical < 2; canonical++) {
                bfq_kmer_opts O = {k, 3, canonical, 0, canonical ? 0u : 20000u};
                std::vector<bfq_kmer_entry> list(100 + 1);
                memset(&list[100], 0xA5, sizeof list[100]);
                bfq_kmer_report R, S;
                int rc = bfq_fastq_kmers_host(a.data(), a.size(), b.data(), b.size() - 1, &O, &R, list.data(), 100);   // (B without its final newline)
                if (rc) { fprintf(stderr, "%s k %u: %d %s\n", name, k, rc, bfq_kmers_host_error()); bad++; continue; }
                rc = bfq_fastq_kmers_host(a.data(), a.size(), nullptr, 0, &O, &S, nullptr, 0);
                const uint8_t *g = (const uint8_t *)&list[100];
                for (size_t i = 0; i < sizeof list[100]; i++) bad += g[i] != 0xA5;
                bad += rc != 0 || S.distinct_a != R.distinct_a || S.windows_a != R.windows_a || S.distinct_b != 0;
                if (canonical)
                    printf("%-9s k %2u  windows %llu / %llu  distinct %llu / %llu  only in A %llu  solid lost %llu  only in B %llu  changed %llu\n", name, k,
                           (unsigned long long)R.windows_a, (unsigned long long)R.windows_b, (unsigned long long)R.distinct_a, (unsigned long long)R.distinct_b,
                           (unsigned long long)R.only_a, (unsigned long long)R.trans[6], (unsigned long long)R.only_b, (unsigned long long)R.distinct_changed);
            }
        bfq_kmer_report R;
        bfq_kmer_opts O = {7, 3, 1, 0, 0};
        bad += bfq_fastq_kmers_host(a.data(), a.size(), nullptr, 0, &O, &R, nullptr, 0) != BFQ_E_ARG;
        O = bfq_kmer_opts{21, 16, 1, 0, 0};
        bad += bfq_fastq_kmers_host(a.data(), a.size(), nullptr, 0, &O, &R, nullptr, 0) != BFQ_E_ARG;
        bad += bfq_fastq_kmers_host(a.data(), a.size() / 2, nullptr, 0, nullptr, &R, nullptr, 0) == BFQ_OK && (a.size() / 2) % 7 == 99;   // a cut text: refused or not, no bad access
    }
    printf(bad ? "FAILED: %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
