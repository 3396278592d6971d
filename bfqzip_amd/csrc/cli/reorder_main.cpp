// reorder_main.cpp -- the reads of a FASTQ file in another order, before a sharded run cuts it into blocks: what
// BFQzip_parallel.py --reorder {1,2} (:59-75,389-437) shells out for (`spring-reorder -i IN -o OUT`, randomFASTQ.py):
//     bfq_reorder -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-r 1|2] [-k K] [-s SEED] [-P PERM] [-V]
//     bfq_reorder -u -P PERM -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-V]
// The order is the library's (include/bfqzip_hip.h, bfq_fastq_reorder_fd): by the smallest hashed k-mer of every read
// (-r 2, the default) or by a seeded hash of its index (-r 1); with -j / -p the mates of a pair move together.
// -P PERM keeps the permutation as a BFQPERM1 file (bfq_fastq_reorder_keep_fd); -u -P PERM undoes it on a text in that order
// (bfq_fastq_unreorder_fd): the records come back in the order of the original file (-r / -k / -s are ignored then).
// Exit status 0 on success; 1 with the library's message otherwise, and then the output files are left empty.
#include <unistd.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-r 1|2] [-k K] [-s SEED] [-P PERM] [-V]\n"
                    "       %s -u -P PERM -i IN.fq [-j IN_2.fq] -o OUT.fq [-p OUT_2.fq] [-V]\n"
                    "  -i <arg>  input FASTQ (REQUIRED)\n"
                    "  -j <arg>  its mates (paired end): record n moves with record n of -i\n"
                    "  -o <arg>  output FASTQ (REQUIRED)\n"
                    "  -p <arg>  output of the mates (REQUIRED with -j)\n"
                    "  -r <arg>  1: seeded random order, 2: by locus (smallest hashed k-mer) (def. 2)\n"
                    "  -k <arg>  k-mer length of -r 2, 8..32 (def. 21)\n"
                    "  -s <arg>  seed of -r 1 (def. 0)\n"
                    "  -P <arg>  the permutation as a BFQPERM1 file: written; read with -u\n"
                    "  -u        undo: IN is in the order of a run with -P, OUT gets the order of the original file (REQUIRES -P)\n"
                    "  -V        phase timeline on stderr\n", argv0, argv0);
    return 1;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string in[2], out[2], perm;
    bool undo = false;
    bfq_reorder_opts O;
    memset(&O, 0, sizeof O);
    O.mode = 2;
    int opt;
    while ((opt = getopt(argc, argv, "i:j:o:p:r:k:s:P:uVh")) != -1) {
        switch (opt) {
        case 'i': in[0] = optarg; break;
        case 'j': in[1] = optarg; break;
        case 'o': out[0] = optarg; break;
        case 'p': out[1] = optarg; break;
        case 'r': O.mode = atoi(optarg); break;
        case 'k': O.k = atoi(optarg); break;
        case 's': O.seed = strtoull(optarg, nullptr, 10); break;
        case 'P': perm = optarg; break;
        case 'u': undo = true; break;
        case 'V': bfq_phase_enable(1); break;
        default: return usage(argv[0]);
        }
    }
    if (in[0].empty() || out[0].empty() || in[1].empty() != out[1].empty() || (undo && perm.empty())) return usage(argv[0]);
    const int np = in[1].empty() ? 1 : 2;
    InFile fi[2], fpin;
    OutFile fo[2], fpout;
    for (int p = 0; p < np; p++)
        if (!fi[p].open(in[p])) { fprintf(stderr, "bfq_reorder: cannot read %s\n", in[p].c_str()); return 1; }
    if (undo && !fpin.open(perm)) { fprintf(stderr, "bfq_reorder: cannot read %s\n", perm.c_str()); return 1; }
    for (int p = 0; p < np; p++)
        if (!fo[p].open(out[p])) { perror("bfq_reorder"); return 1; }
    if (!undo && !perm.empty() && !fpout.open(perm)) { perror("bfq_reorder"); return 1; }
    // the outputs are as long as the inputs: their pages are prepared while the GPU starts up
    for (int p = 0; p < np; p++)
        if (fi[p].size >= (64u << 20)) (void)bfq_output_prefault(fo[p].fd, fi[p].size + 4096, fi[p].size);
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_reorder", &P);
    if (!c) return 1;
    const int ifd[2] = {fi[0].fd, fi[1].fd}, ofd[2] = {fo[0].fd, fo[1].fd};
    const uint64_t ilen[2] = {fi[0].size, fi[1].size};
    uint64_t olen[2] = {0, 0}, reads = 0, plen = 0;
    const int rc = undo             ? bfq_fastq_unreorder_fd(c, ifd, ilen, np, fpin.fd, fpin.size, ofd, olen, &reads)
                   : !perm.empty() ? bfq_fastq_reorder_keep_fd(c, ifd, ilen, np, &O, ofd, fpout.fd, olen, &plen, &reads)
                                   : bfq_fastq_reorder_fd(c, ifd, ilen, np, &O, ofd, olen, &reads);
    if (rc) {
        fprintf(stderr, "bfq_reorder: %s\n", bfq_last_error(c));
        bfq_destroy(c);
        return 1;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_reorder");
    bool closed = true;
    for (int p = 0; p < np; p++) closed = fo[p].close() && closed;
    if (fpout.fd >= 0) closed = fpout.close() && closed;
    bfq_destroy(c);
    if (!closed) { perror("bfq_reorder"); return 1; }
    bfq_phase_report("bfq_reorder");
    printf("%llu reads, %llu bytes\n", (unsigned long long)reads, (unsigned long long)(olen[0] + olen[1]));
    return 0;
}
