// edits_main.cpp -- bases back exactly: the base edits of a run as a side file, the BFQEDIT1 container (include/bfqzip_hip.h),
// made and applied on the GPU (bfq_fastq_edits_fd / bfq_fastq_unedit_fd).  Not a tool of the reference, whose only way to
// keep the bases is to switch the method off (-k 10000).
//     bfq_edits -a IN.fq -b OUT.fq -o RUN.edits [-V]       make: the input's byte at every base the run changed
//     bfq_edits -u -E RUN.edits -i OUT.fq -o BACK.fq [-V]  apply: OUT.fq with the input's bases, every other byte as it was
//     bfq_edits -l RUN.edits                               the members of the file, one line each (no GPU)
// IN.fq and OUT.fq are in the same read order; BGZF files are read as their text.  RUN.edits may hold several members, one per
// block of a sharded run (parallel.py --keep-bases).  Exit status of a make as cmp's: 0 the run changed no base, 1 it did,
// 2 an error; of -u and -l: 0, or 2 with the library's message.  On an error the output is left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -a IN.fq -b OUT.fq -o RUN.edits [-V]\n"
                    "       %s -u -E RUN.edits -i OUT.fq -o BACK.fq [-V]\n"
                    "       %s -l RUN.edits\n"
                    "  -a <arg>  the FASTQ that went into the run\n"
                    "  -b <arg>  the FASTQ that came out of it, in the same read order\n"
                    "  -o <arg>  the BFQEDIT1 file to write (make) / the FASTQ with the input's bases (-u)\n"
                    "  -u        apply: needs -E and -i\n"
                    "  -E <arg>  the BFQEDIT1 file of the run (one member, or one per block back to back)\n"
                    "  -i <arg>  the FASTQ the run wrote\n"
                    "  -l <arg>  list the members of a BFQEDIT1 file and exit (no GPU)\n"
                    "  -V        phase timeline on stderr\n"
                    "exit status of a make: 0 no base changed, 1 some did, 2 error\n", argv0, argv0, argv0);
    return 2;
}

static int list_members(const std::string &path)
{
    InFile f;
    if (!f.open(path)) { fprintf(stderr, "bfq_edits: cannot read %s\n", path.c_str()); return 2; }
    void *m = f.size ? mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0) : MAP_FAILED;
    const uint8_t *z = m != MAP_FAILED ? (const uint8_t *)m : nullptr;
    uint64_t N = 0, T = 0, E = 0, M = 0;
    if (bfq_edits_info(z, f.size, &N, &T, &E, &M)) { fprintf(stderr, "bfq_edits: %s\n", bfq_edits_host_error()); return 2; }
    printf("# member  reads  bases  edits  bytes\n");
    uint64_t at = 0;
    for (uint64_t k = 0; k < M; k++) {
        const int64_t len = bfq_edits_member_len(z + at, f.size - at);
        uint64_t n = 0, t = 0, e = 0, one = 0;
        (void)bfq_edits_info(z + at, (uint64_t)len, &n, &t, &e, &one);
        printf("%llu  %llu  %llu  %llu  %lld\n", (unsigned long long)k, (unsigned long long)n, (unsigned long long)t, (unsigned long long)e, (long long)len);
        at += (uint64_t)len;
    }
    printf("%llu members, %llu reads, %llu bases, %llu edits\n", (unsigned long long)M, (unsigned long long)N, (unsigned long long)T, (unsigned long long)E);
    if (m != MAP_FAILED) munmap(m, f.size);
    return 0;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string a, b, out, edits, in, list;
    bool apply = false;
    int opt;
    while ((opt = getopt(argc, argv, "a:b:o:uE:i:l:Vh")) != -1) {
        switch (opt) {
        case 'a': a = optarg; break;
        case 'b': b = optarg; break;
        case 'o': out = optarg; break;
        case 'u': apply = true; break;
        case 'E': edits = optarg; break;
        case 'i': in = optarg; break;
        case 'l': list = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    if (!list.empty()) return list_members(list);
    if (out.empty() || (apply ? edits.empty() || in.empty() || !a.empty() || !b.empty() : a.empty() || b.empty() || !edits.empty() || !in.empty()))
        return usage(argv[0]);
    InFile f1, f2;
    const std::string &p1 = apply ? in : a, &p2 = apply ? edits : b;
    if (!f1.open(p1)) { fprintf(stderr, "bfq_edits: cannot read %s\n", p1.c_str()); return 2; }
    if (!f2.open(p2)) { fprintf(stderr, "bfq_edits: cannot read %s\n", p2.c_str()); return 2; }
    OutFile fo;
    if (!fo.open(out)) { perror("bfq_edits"); return 2; }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_edits", &P);
    if (!c) return 2;
    uint64_t outLen = 0;
    bfq_edit_stats S;
    const int rc = apply ? bfq_fastq_unedit_fd(c, f1.fd, f1.size, f2.fd, f2.size, fo.fd, &outLen, &S)
                         : bfq_fastq_edits_fd(c, f1.fd, f1.size, f2.fd, f2.size, fo.fd, &outLen, &S);
    if (rc) {
        fprintf(stderr, "bfq_edits: %s\n", bfq_last_error(c));
        bfq_destroy(c);
        return 2;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_edits");
    const bool closed = fo.close();
    bfq_destroy(c);
    if (!closed) { perror("bfq_edits"); return 2; }
    bfq_phase_report("bfq_edits");
    if (apply) printf("%llu reads, %llu bases, %llu edits in %llu reads written back, %llu bytes\n", (unsigned long long)S.reads, (unsigned long long)S.bases,
                      (unsigned long long)S.edits, (unsigned long long)S.reads_touched, (unsigned long long)outLen);
    else printf("%llu reads, %llu bases, %llu edits in %llu reads, %llu bytes\n", (unsigned long long)S.reads, (unsigned long long)S.bases,
                (unsigned long long)S.edits, (unsigned long long)S.reads_touched, (unsigned long long)outLen);
    return !apply && S.edits ? 1 : 0;
}
