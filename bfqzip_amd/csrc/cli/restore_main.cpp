// restore_main.cpp -- the way back from the compressed streams to a FASTQ file (not a tool of the reference, which leaves
// this to `7z x` / `bsc d` + `paste`):
//     bfq_restore -d OUT.fq.dna.bsc -q OUT.fq.qs.bsc [-H OUT.h.bsc] [-P PERM] -o OUT.fq [-V]
// The inputs are what `bsc e`, bfq_fastq_job.compress_streams = 1 / 2 / 3 and parallel.py --compress write
// (include/bfqzip_hip.h, bfq_fastq_restore_fd).  -P PERM: the BFQPERM1 file `bfq_reorder -P` / `parallel.py --keep-order`
// wrote for the run: the records come back in the order of the original file (bfq_fastq_restore_ordered_fd).  Exit status 0 on success; 1 with the library's message otherwise, and then
// OUT.fq is left empty.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -d DNA.bsc -q QS.bsc [-H HEADERS.bsc] [-P PERM] -o OUT.fq [-V]\n"
                    "  -d <arg>  container(s) of the DNA stream (OUT.fq.dna; BFQDNAC1 / BFQRANS2 members, or one BFQEBWT1) (REQUIRED)\n"
                    "  -q <arg>  container(s) of the quality stream (OUT.fq.qs) (REQUIRED)\n"
                    "  -H <arg>  container(s) of the header stream (OUT.h); without it every header line is \"@\"\n"
                    "  -P <arg>  BFQPERM1 file of the reordering the collection went through: the text in the order before it\n"
                    "  -o <arg>  output FASTQ (REQUIRED)\n"
                    "  -V        phase timeline on stderr\n", argv0);
    return 1;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string dna, qs, hdr, perm, output;
    int opt;
    while ((opt = getopt(argc, argv, "d:q:H:P:o:Vh")) != -1) {
        switch (opt) {
        case 'd': dna = optarg; break;
        case 'q': qs = optarg; break;
        case 'H': hdr = optarg; break;
        case 'P': perm = optarg; break;
        case 'o': output = optarg; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    if (dna.empty() || qs.empty() || output.empty()) return usage(argv[0]);
    InFile fd, fq, fh, fp;
    if (!fd.open(dna) || !fq.open(qs) || (!hdr.empty() && !fh.open(hdr)) || (!perm.empty() && !fp.open(perm))) { fprintf(stderr, "bfq_restore: cannot read the inputs\n"); return 1; }
    OutFile outText;
    if (!outText.open(output)) { perror("bfq_restore"); return 1; }
    {   // the bound of the text from the container headers: the output's pages are prepared while the GPU starts up
        auto map = [](const InFile &f) { return f.size ? mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0) : MAP_FAILED; };
        void *md = map(fd), *mq = map(fq), *mh = hdr.empty() ? MAP_FAILED : map(fh);
        int64_t bound = -1;
        if (md != MAP_FAILED && mq != MAP_FAILED && (hdr.empty() || mh != MAP_FAILED))
            bound = bfq_fastq_restore_bound((const uint8_t *)md, fd.size, (const uint8_t *)mq, fq.size, hdr.empty() ? nullptr : (const uint8_t *)mh, fh.size);
        if (md != MAP_FAILED) munmap(md, fd.size);
        if (mq != MAP_FAILED) munmap(mq, fq.size);
        if (mh != MAP_FAILED) munmap(mh, fh.size);
        if (bound < 0) { fprintf(stderr, "bfq_restore: the inputs are not containers (BFQDNAC1 / BFQRANS2 / BFQLINE1 / BFQNAME1 / BFQQUAL1 / BFQEBWT1)\n"); outText.close(); return 1; }
        if (bound >= (64 << 20)) (void)bfq_output_prefault(outText.fd, (uint64_t)bound + 4096, (uint64_t)bound / 2);
    }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_restore", &P);
    if (!c) return 1;
    uint64_t outLen = 0, reads = 0;
    const int rc = perm.empty() ? bfq_fastq_restore_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, outText.fd, &outLen, &reads)
                                : bfq_fastq_restore_ordered_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, fp.fd, fp.size,
                                                               outText.fd, &outLen, &reads);
    if (rc) {
        fprintf(stderr, "bfq_restore: %s\n", bfq_last_error(c));
        bfq_destroy(c);
        return 1;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_restore");
    const bool closed = outText.close();
    bfq_destroy(c);
    if (!closed) { perror("bfq_restore"); return 1; }
    bfq_phase_report("bfq_restore");
    printf("%llu reads, %llu bytes\n", (unsigned long long)reads, (unsigned long long)outLen);
    return 0;
}
