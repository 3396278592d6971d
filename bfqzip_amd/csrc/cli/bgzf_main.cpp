// bgzf_main.cpp -- bgzip-compressed FASTQ to text and back on the GPU (not a tool of the reference, which takes plain text only):
//     bfq_bgzf -d IN.fq.gz -o OUT.fq [-V]     inflate
//     bfq_bgzf -c IN.fq -o OUT.fq.gz [-0] [-V]  deflate: BGZF members of 65 280 bytes and the EOF member (bfq_bgzf_deflate_fd);
//                                             -0: every member stored.  An input that is already compressed is refused.
//     bfq_bgzf -t IN.fq.gz                    inflate and verify (every member's length and CRC32), writing nothing
//     bfq_bgzf -l IN.fq.gz                    members, raw length, ratio: no GPU is touched
//     bfq_bgzf -g -d IN.fq.gz -o OUT.fq [-V]  plain gzip (gzip, pigz, bcl2fastq, `cat a.gz b.gz`; BGZF too): the deflate streams
//     bfq_bgzf -g -t IN.fq.gz                 are inflated side by side (bfq_gzip_inflate_fd, csrc/bfq_gzip.h); -t verifies
//     bfq_bgzf -g -l IN.fq.gz                 every member's CRC32 and length; -l prints members, compressed and raw bytes,
//                                             pieces, chain length and skipped candidates (on the GPU: a gzip file has no
//                                             directory to read them from)
// Without -g the input is BGZF (bgzip, htslib, BCL Convert): include/bfqzip_hip.h, bfq_bgzf_inflate_fd, and plain gzip is
// refused with a message that says to recompress with bgzip.  The tools that take FASTQ (gsufsort, bfq_compare, ...) take a BGZF file as it
// is; this one is for the ones that do not (bfq_reorder, the multi-GPU driver's line index).  Exit status 0 on success; 1 with
// the library's message on a damaged file, and then OUT.fq is left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s [-g] -d IN.fq.gz -o OUT.fq [-V] | -c IN.fq -o OUT.fq.gz [-0] [-V] | [-g] -t IN.fq.gz | [-g] -l IN.fq.gz\n"
                    "  -d <arg>  bgzip-compressed (BGZF) input to inflate (with -o)\n"
                    "  -c <arg>  text to compress into BGZF (with -o)\n"
                    "  -0        with -c: every member stored\n"
                    "  -o <arg>  output (text with -d, BGZF with -c)\n"
                    "  -t <arg>  inflate and verify only: no output is written\n"
                    "  -l <arg>  print members, compressed and raw length, ratio, and exit (no GPU)\n"
                    "  -g        with -d, -t, -l: the input is plain gzip (any gzip file), inflated side by side; -l runs on the GPU\n"
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
    bool gzip = false;
    while ((opt = getopt(argc, argv, "d:c:t:l:o:0gVh")) != -1) {
        switch (opt) {
        case '0': level = 0; break;
        case 'g': gzip = true; break;
        case 'd': case 'c': case 't': case 'l':
            if (mode) return usage(argv[0]);
            mode = (char)opt; input = optarg; break;
        case 'o': output = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    const bool writes = mode == 'd' || mode == 'c';
    if (!mode || writes != !output.empty() || (level == 0 && mode != 'c') || (gzip && mode == 'c')) return usage(argv[0]);
    InFile in;
    if (!in.open(input)) { fprintf(stderr, "bfq_bgzf: cannot read %s\n", input.c_str()); return 1; }
    if (mode == 'l' && !gzip) return list_members(in, input);
    OutFile out;
    if (writes && !out.open(output)) { perror("bfq_bgzf"); return 1; }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_bgzf", &P);
    if (!c) return 1;
    uint64_t outLen = 0, members = 0;
    bfq_gzip_stats gs = {};
    int rc;
    if (gzip && mode == 'l') {
        void *m = in.size ? mmap(nullptr, in.size, PROT_READ, MAP_PRIVATE, in.fd, 0) : MAP_FAILED;
        rc = bfq_gzip_measure(c, m != MAP_FAILED ? (const uint8_t *)m : nullptr, m != MAP_FAILED ? in.size : 0, 0, &outLen, &members, &gs);
        if (m != MAP_FAILED) munmap(m, in.size);
    } else if (gzip) rc = bfq_gzip_inflate_fd(c, in.fd, in.size, 0, mode == 'd' ? out.fd : -1, &outLen, &gs);
    else rc = mode == 'c' ? bfq_bgzf_deflate_fd(c, in.fd, in.size, level, out.fd, &outLen)
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
    if (mode == 'l')
        printf("%llu members, %llu bytes compressed, %llu bytes raw, %llu pieces, chain %llu, %llu candidates skipped\n", (unsigned long long)members,
               (unsigned long long)in.size, (unsigned long long)outLen, (unsigned long long)gs.pieces, (unsigned long long)gs.chain,
               (unsigned long long)gs.skipped);
    else if (mode == 'c') printf("%llu bytes -> %llu bytes\n", (unsigned long long)in.size, (unsigned long long)outLen);
    else printf("%llu bytes%s\n", (unsigned long long)outLen, mode == 't' ? " verified" : "");
    return 0;
}
