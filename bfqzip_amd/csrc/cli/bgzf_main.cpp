// bgzf_main.cpp -- bgzip-compressed FASTQ to text and back on the GPU (not a tool of the reference, which takes plain text only):
//     bfq_bgzf -d IN.fq.gz -o OUT.fq [-V]     inflate
//     bfq_bgzf -c IN.fq -o OUT.fq.gz [-0] [-V]  deflate: BGZF members of 65 280 bytes and the EOF member (bfq_bgzf_deflate_fd);
//                                             -0: every member stored.  An input that is already compressed is refused.
//     bfq_bgzf -t IN.fq.gz                    inflate and verify (every member's length and CRC32), writing nothing
//     bfq_bgzf -l IN.fq.gz                    members, raw length, ratio: no GPU is touched
// The input is BGZF (bgzip, htslib, BCL Convert): include/bfqzip_hip.h, bfq_bgzf_inflate_fd.  Plain gzip is refused with a
// message that says to recompress with bgzip.  The tools that take FASTQ (gsufsort, bfq_compare, ...) take a BGZF file as it
// is; this one is for the ones that do not (bfq_reorder, the multi-GPU driver's line index).  Exit status 0 on success; 1 with
// the library's message on a damaged file, and then OUT.fq is left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -d IN.fq.gz -o OUT.fq [-V] | -c IN.fq -o OUT.fq.gz [-0] [-V] | -t IN.fq.gz | -l IN.fq.gz\n"
                    "  -d <arg>  bgzip-compressed (BGZF) input to inflate (with -o)\n"
                    "  -c <arg>  text to compress into BGZF (with -o)\n"
                    "  -0        with -c: every member stored\n"
                    "  -o <arg>  output (text with -d, BGZF with -c)\n"
                    "  -t <arg>  inflate and verify only: no output is written\n"
                    "  -l <arg>  print members, compressed and raw length, ratio, and exit (no GPU)\n"
                    "  -V        phase timeline on stderr\n", argv0);
    return 1;
}

static int list_members(const InFile &f, const std::string &name)
{
    void *m = f.size ? mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0) : MAP_FAILED;
    static const uint8_t none = 0;
    const uint8_t *p = m != MAP_FAILED ? (const uint8_t *)m : &none;
    uint64_t n = 0, raw = 0, bad = 0;
    const int rc = bfq_bgzf_index(p, m != MAP_FAILED ? f.size : 0, nullptr, 0, &n, &raw, &bad);
    if (rc || !f.size) {
        // a gzip member without the extra field is what plain gzip writes; anything else is a damaged or foreign file
        if (n == 0 && f.size >= 4 && p[0] == 0x1F && p[1] == 0x8B && p[2] == 8 && p[3] != 4)
            fprintf(stderr, "bfq_bgzf: %s: gzip input that is not BGZF: recompress it with bgzip\n", name.c_str());
        else
            fprintf(stderr, "bfq_bgzf: %s: not a BGZF file: the header of member %llu at byte %llu is refused\n", name.c_str(),
                    (unsigned long long)n, (unsigned long long)bad);
        return 1;
    }
    printf("%llu members, %llu bytes compressed, %llu bytes raw, ratio %.3f\n", (unsigned long long)n, (unsigned long long)f.size,
           (unsigned long long)raw, f.size ? (double)raw / (double)f.size : 0.0);
    return 0;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string input, output;
    char mode = 0;
    int opt, level = 1;
    while ((opt = getopt(argc, argv, "d:c:t:l:o:0Vh")) != -1) {
        switch (opt) {
        case '0': level = 0; break;
        case 'd': case 'c': case 't': case 'l':
            if (mode) return usage(argv[0]);
            mode = (char)opt; input = optarg; break;
        case 'o': output = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    const bool writes = mode == 'd' || mode == 'c';
    if (!mode || writes != !output.empty() || (level == 0 && mode != 'c')) return usage(argv[0]);
    InFile in;
    if (!in.open(input)) { fprintf(stderr, "bfq_bgzf: cannot read %s\n", input.c_str()); return 1; }
    if (mode == 'l') return list_members(in, input);
    OutFile out;
    if (writes && !out.open(output)) { perror("bfq_bgzf"); return 1; }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_bgzf", &P);
    if (!c) return 1;
    uint64_t outLen = 0;
    const int rc = mode == 'c' ? bfq_bgzf_deflate_fd(c, in.fd, in.size, level, out.fd, &outLen)
                               : bfq_bgzf_inflate_fd(c, in.fd, in.size, mode == 'd' ? out.fd : -1, &outLen);
    if (rc) {
        fprintf(stderr, "bfq_bgzf: %s: %s\n", input.c_str(), bfq_last_error(c));
        bfq_destroy(c);
        if (writes && ftruncate(out.fd, 0) != 0) perror("bfq_bgzf");
        return 1;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_bgzf");
    const bool closed = out.close();
    bfq_destroy(c);
    if (!closed) { perror("bfq_bgzf"); return 1; }
    bfq_phase_report("bfq_bgzf");
    if (mode == 'c') printf("%llu bytes -> %llu bytes\n", (unsigned long long)in.size, (unsigned long long)outLen);
    else printf("%llu bytes%s\n", (unsigned long long)outLen, mode == 't' ? " verified" : "");
    return 0;
}
