// bam_main.cpp -- BAM (unaligned or aligned) to FASTQ text on the GPU (not a tool of the reference, which takes plain text only):
//     bfq_bam -i IN.bam -o OUT.fq [-F MASK] [-n] [-v Q] [-C PIECE] [-a LIST|'*' [-S]] [-V]   every kept record, in file order
//     bfq_bam -i IN.bam -1 OUT_1.fq -2 OUT_2.fq [-0 OTHER.fq] [-c] [...]            READ1 / READ2 / the rest; -c: the pairing check
//     bfq_bam -t IN.bam                                                             convert and verify, writing nothing
//     bfq_bam -i IN.bam -u OUT.bam -o TEXT.fq | -1 T_1.fq -2 T_2.fq [-0 T_0.fq] [-N] [-L 0|1] [...]
//                                                                                   the way back: IN.bam with the reads of the texts in it
//     bfq_bam -w OUT.bam -o IN.fq | -1 IN_1.fq -2 IN_2.fq [-0 IN_0.fq] [-T HEADER.sam] [-R RGID] [-a LIST|'*'] [-c] [-n] [-L 0|1] [-V]
//                                                                                   FASTQ files as an unaligned BAM (no BAM input)
//     bfq_bam -l IN.bam                                                             the header counts and the statistics as JSON
// include/bfqzip_hip.h, bfq_bam_to_fastq_fd: the records' text is this project's definition, modelled on the defaults of
// `samtools fastq` (-F 0x900; /1 and /2 unless -n; absent qualities as -v Q, default 1).  Exit status 0 on success; 1 with
// the library's message on a damaged or unpaired file, and then the outputs are left empty.
// With -u the FASTQ options name the texts to READ (bfq_bam_patch_fd): their sequence and quality lines go back into the SEQ
// and QUAL fields of the records they came from -- -F, -n, -v, -C as on the run that made the texts --, everything else stays
// byte for byte and OUT.bam is compressed on the device.  One line with the statistics; on a refusal OUT.bam is left empty.
// With -w the FASTQ options name the texts to READ too (bfq_fastq_to_bam_fd): their reads become the records of a new unaligned
// BAM -- -o alone: flag 4; -1 -2: flags 77 / 141, interleaved, the reads of -0 behind them --, made and compressed on the device.
// -T: the header's text (as it is; default "@HD VN:1.6 SO:unsorted"), -R: RG:Z:<RGID> on every record, -c: the mates' names
// are compared, -n: "/1" and "/2" stay on the names.  One line with the statistics; on a refusal OUT.bam is left empty.
// -a LIST|'*' carries aux tags through the header lines (modelled on `samtools fastq -T` / `samtools import -T`; -T is the
// header file here): with -i / -t / -l the selected tags of every kept record are written behind its name as \tXX:T:value
// (-S: refuse a selected tag that cannot be carried instead of leaving it out); with -w the fields XX:T:value of the header
// lines become tags of the records; with -u it changes nothing (tags stay byte for byte there).  -V prints the tag counts.
#include <unistd.h>
#include <sys/mman.h>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -i IN.bam -o OUT.fq | -1 OUT_1.fq -2 OUT_2.fq [-0 OTHER.fq] [-c] [-F MASK] [-n] [-v Q] [-C PIECE] [-a LIST|'*' [-S]] [-V] | -t IN.bam | -l IN.bam\n"
                    "       %s -i IN.bam -u OUT.bam -o TEXT.fq | -1 T_1.fq -2 T_2.fq [-0 T_0.fq] [-N] [-L 0|1] [-F MASK] [-n] [-v Q] [-C PIECE] [-V]\n"
                    "       %s -w OUT.bam -o IN.fq | -1 IN_1.fq -2 IN_2.fq [-0 IN_0.fq] [-T HEADER.sam] [-R RGID] [-a LIST|'*'] [-c] [-n] [-L 0|1] [-V]\n"
                    "  -i <arg>  BAM input (BGZF, or the inflated stream itself)\n"
                    "  -o <arg>  one FASTQ output: every kept record in file order\n"
                    "  -1 -2 <arg>  split: READ1-only and READ2-only records; -0 <arg>: the rest (dropped without it)\n"
                    "  -c        with -1 -2: refuse unless the k-th names of both files are equal (collated input)\n"
                    "  -F <arg>  leave out records with any of these flag bits (default 0x900)\n"
                    "  -n        no /1 and /2 behind the names\n"
                    "  -v <arg>  quality given to reads without qualities (default 1)\n"
                    "  -C <arg>  bytes per piece of the stream (default 65536)\n"
                    "  -t <arg>  convert and verify only: no output is written\n"
                    "  -l <arg>  print references, header bytes, records and the statistics as JSON\n"
                    "  -u <arg>  the way back: write IN.bam with the reads of the FASTQ files (-o | -1 -2 [-0], now inputs) in it\n"
                    "  -N        with -u: refuse unless every read's name is its record's\n"
                    "  -L <arg>  with -u: 0 = stored members, 1 = compressed (default 1)\n"
                    "  -w <arg>  no BAM input: write the FASTQ files (-o | -1 -2 [-0], now inputs) as this unaligned BAM\n"
                    "  -T <arg>  with -w: a file whose bytes become the header's text (default: @HD VN:1.6 SO:unsorted)\n"
                    "  -R <arg>  with -w: the read group: RG:Z:<arg> on every record (and @RG ID:<arg> in the default header)\n"
                    "            with -w, -c compares the names of the mates, -n keeps /1 and /2 on the names, -L as with -u\n"
                    "  -a <arg>  aux tags through the header lines: '*' = every tag, or a list (BC,RX; at most 32).  With -i / -t / -l the\n"
                    "            selected tags of a record are written behind its name as <tab>XX:T:value; with -w the fields XX:T:value of\n"
                    "            the header lines become tags (types A, i, Z, H; f and B tags are not carried); with -u nothing changes\n"
                    "  -S        with -a on the way in: refuse a selected tag that cannot be carried instead of leaving it out\n"
                    "  -V        phase timeline on stderr; with -a the tag counts\n", argv0, argv0, argv0);
    return 1;
}

// -u: IN.bam with the reads of the texts in it, to OUT.bam
static int patch(const std::string &input, const std::string text[3], const std::string &outName, const bfq_bam_opts &O, int level)
{
    InFile in, tin[3];
    if (!in.open(input)) { fprintf(stderr, "bfq_bam: cannot read %s\n", input.c_str()); return 1; }
    int fds[3] = {-1, -1, -1};
    for (int k = 0; k < 3; k++)
        if (!text[k].empty()) {
            if (!tin[k].open(text[k])) { fprintf(stderr, "bfq_bam: cannot read %s\n", text[k].c_str()); return 1; }
            fds[k] = tin[k].fd;
        }
    OutFile out;
    if (!out.open(outName)) { perror("bfq_bam"); return 1; }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_bam", &P);
    if (!c) return 1;
    uint64_t outLen = 0;
    bfq_bam_patch_stats S = {};
    if (bfq_bam_patch_fd(c, in.fd, in.size, &O, fds, level, out.fd, &outLen, &S)) {
        fprintf(stderr, "bfq_bam: %s: %s\n", input.c_str(), bfq_last_error(c));
        bfq_destroy(c);
        if (ftruncate(out.fd, 0) != 0) perror("bfq_bam");
        return 1;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_bam");
    const bool closed = out.close();
    bfq_destroy(c);
    if (!closed) { perror("bfq_bam"); return 1; }
    bfq_phase_report("bfq_bam");
    typedef unsigned long long ull;
    printf("%llu records: %llu + %llu + %llu patched, %llu skipped, %llu reads changed (%llu bases, %llu qualities), %llu unknown bases, %llu high qualities and "
           "%llu absent kept; %llu bytes of stream, %llu bytes written\n", (ull)S.records, (ull)S.patched[0], (ull)S.patched[1], (ull)S.patched[2], (ull)S.skipped,
           (ull)S.reads_changed, (ull)S.bases_changed, (ull)S.quals_changed, (ull)S.unknown_bases, (ull)S.kept_high_quals, (ull)S.kept_absent, (ull)S.raw_len, (ull)outLen);
    return 0;
}

// -w: the FASTQ files as an unaligned BAM, to OUT.bam
static int write_ubam(const std::string text[3], const std::string &outName, const std::string &headerName, const std::string &rg, bool pairedCheck, bool mateSuffix,
                      int level, const bfq_bam_tag_opts *tags, bool verbose)
{
    InFile tin[3], hin;
    int fds[3] = {-1, -1, -1};
    for (int k = 0; k < 3; k++)
        if (!text[k].empty()) {
            if (!tin[k].open(text[k])) { fprintf(stderr, "bfq_bam: cannot read %s\n", text[k].c_str()); return 1; }
            fds[k] = tin[k].fd;
        }
    bfq_ubam_tag_opts X = {};
    bfq_ubam_tag_stats TS = {};
    bfq_ubam_opts &O = X.o;
    bfq_ubam_default_opts(&O);
    if (tags) {                                                    // (the list as -a gave it)
        O.reserved = BFQ_UBAM_OPTS_TAGS;
        X.n_tags = tags->n_tags; X.stats = &TS;
        memcpy(X.tag, tags->tag, sizeof X.tag);
    }
    O.paired_check = pairedCheck ? 1 : 0; O.mate_suffix = mateSuffix ? 1 : 0; O.level = (uint32_t)level;
    void *hm = MAP_FAILED;
    static const uint8_t none = 0;
    if (!headerName.empty()) {
        if (!hin.open(headerName)) { fprintf(stderr, "bfq_bam: cannot read %s\n", headerName.c_str()); return 1; }
        hm = hin.size ? mmap(nullptr, hin.size, PROT_READ, MAP_PRIVATE, hin.fd, 0) : MAP_FAILED;
        if (hin.size && hm == MAP_FAILED) { perror("bfq_bam"); return 1; }
        O.header_text = hin.size ? (const uint8_t *)hm : &none; O.header_len = hin.size;
    }
    if (!rg.empty()) O.rg_id = rg.c_str();
    OutFile out;
    if (!out.open(outName)) { perror("bfq_bam"); return 1; }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_bam", &P);
    if (!c) return 1;
    uint64_t outLen = 0;
    bfq_ubam_stats S = {};
    if (bfq_fastq_to_bam_fd(c, fds, &O, out.fd, &outLen, &S)) {
        fprintf(stderr, "bfq_bam: %s: %s\n", outName.c_str(), bfq_last_error(c));
        bfq_destroy(c);
        if (ftruncate(out.fd, 0) != 0) perror("bfq_bam");
        return 1;
    }
    if (hm != MAP_FAILED) munmap(hm, hin.size);
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_bam");
    const bool closed = out.close();
    bfq_destroy(c);
    if (!closed) { perror("bfq_bam"); return 1; }
    bfq_phase_report("bfq_bam");
    typedef unsigned long long ull;
    if (tags && verbose)
        fprintf(stderr, "bfq_bam: tags: %llu written, %llu fields dropped, %llu bytes of stream\n", (ull)TS.tags_written, (ull)TS.fields_dropped, (ull)TS.tag_bytes);
    printf("%llu records: %llu + %llu + %llu written, %llu numbered, %llu comments dropped, %llu unknown bases; %llu bytes of stream in %llu members, "
           "%llu bytes written\n", (ull)S.records, (ull)S.written[0], (ull)S.written[1], (ull)S.written[2], (ull)S.named, (ull)S.comments_dropped,
           (ull)S.unknown_bases, (ull)S.raw_len, (ull)S.members, (ull)outLen);
    return 0;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string input, outName[3], patchName, writeName, headerName, rgId;
    int level = 1;
    char mode = 0;
    bfq_bam_tag_opts X = {};
    bfq_bam_tag_stats TS = {};
    bfq_bam_opts &O = X.o;
    bfq_bam_default_opts(&O);
    bool tags = false, verbose = false;
    int opt;
    bool single = false;                                           // -o was given
    while ((opt = getopt(argc, argv, "i:t:l:o:0:1:2:cF:nv:C:Vhu:NL:w:T:R:a:S")) != -1) {
        switch (opt) {
        case 'i': case 't': case 'l':
            if (mode) return usage(argv[0]);
            mode = (char)opt; input = optarg; break;
        case 'o': case '0':
            if (!outName[0].empty()) return usage(argv[0]);
            outName[0] = optarg; single = opt == 'o'; if (opt == '0') O.split = 1; break;
        case '1': outName[1] = optarg; O.split = 1; break;
        case '2': outName[2] = optarg; O.split = 1; break;
        case 'c': O.paired_check = 1; break;
        case 'F': O.exclude_flags = (uint32_t)strtoul(optarg, nullptr, 0); break;
        case 'n': O.mate_suffix = 0; break;
        case 'v': O.default_qual = (uint32_t)strtoul(optarg, nullptr, 10); break;
        case 'C': O.piece = (uint32_t)strtoul(optarg, nullptr, 10); break;
        case 'V': bfq_phase_enable(1); verbose = true; break;
        case 'a':
            if (!parse_tag_list(optarg, &X.n_tags, X.tag)) { fprintf(stderr, "bfq_bam: -a: '*', or at most 32 two-byte tags separated by commas\n"); return usage(argv[0]); }
            tags = true; break;
        case 'S': X.strict = 1; break;
        case 'u': patchName = optarg; break;
        case 'N': O.check_names = 1; break;
        case 'L': level = atoi(optarg); break;
        case 'w': writeName = optarg; break;
        case 'T': headerName = optarg; break;
        case 'R': rgId = optarg; break;
        default: return usage(argv[0]);
        }
    }
    const bool anyOut = !outName[0].empty() || !outName[1].empty() || !outName[2].empty();
    if (!writeName.empty()) {                                      // -w: no BAM input; -o | -1 -2 [-0] name the texts to read
        if (mode || !patchName.empty() || O.check_names || !anyOut || (single && (!outName[1].empty() || !outName[2].empty())) ||
            outName[1].empty() != outName[2].empty() || (!single && outName[1].empty()) || (O.paired_check && outName[1].empty()))
            return usage(argv[0]);
        if (X.strict) return usage(argv[0]);                        // (the way out drops what is no tag, and never refuses it)
        return write_ubam(outName, writeName, headerName, rgId, O.paired_check != 0, O.mate_suffix != 0, level, tags ? &X : nullptr, verbose);
    }
    if (!headerName.empty() || !rgId.empty() || (X.strict && !tags)) return usage(argv[0]);
    if (tags) { O.reserved = BFQ_BAM_OPTS_TAGS; X.stats = &TS; }
    if (!mode || (mode != 'i' && anyOut) || (mode == 'i' && !anyOut)) return usage(argv[0]);
    if (mode == 'i' && (single ? O.split != 0 : outName[1].empty() || outName[2].empty())) return usage(argv[0]);
    if (O.paired_check && !O.split) return usage(argv[0]);
    if (patchName.empty() ? O.check_names != 0 : mode != 'i' || O.paired_check) return usage(argv[0]);
    if (!patchName.empty()) return patch(input, outName, patchName, O, level);
    InFile in;
    if (!in.open(input)) { fprintf(stderr, "bfq_bam: cannot read %s\n", input.c_str()); return 1; }
    OutFile out[3];
    int fds[3] = {-1, -1, -1};
    for (int o = 0; o < 3; o++)
        if (!outName[o].empty()) {
            if (!out[o].open(outName[o])) { perror("bfq_bam"); return 1; }
            fds[o] = out[o].fd;
        }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_bam", &P);
    if (!c) return 1;
    uint64_t outLen[3] = {0, 0, 0}, nReads[3] = {0, 0, 0};
    bfq_bam_stats S = {};
    int rc;
    if (mode == 'l') {
        void *m = in.size ? mmap(nullptr, in.size, PROT_READ, MAP_PRIVATE, in.fd, 0) : MAP_FAILED;
        rc = bfq_bam_measure(c, m != MAP_FAILED ? (const uint8_t *)m : nullptr, m != MAP_FAILED ? in.size : 0, &O, outLen, nReads, &S);
        if (m != MAP_FAILED) munmap(m, in.size);
    } else rc = bfq_bam_to_fastq_fd(c, in.fd, in.size, &O, fds, outLen, nReads, &S);
    if (rc) {
        fprintf(stderr, "bfq_bam: %s: %s\n", input.c_str(), bfq_last_error(c));
        bfq_destroy(c);
        for (int o = 0; o < 3; o++)
            if (fds[o] >= 0 && ftruncate(fds[o], 0) != 0) perror("bfq_bam");
        return 1;
    }
    bfq_phase("teardown");
    trace_kernel_times(c, "bfq_bam");
    bool closed = true;
    for (int o = 0; o < 3; o++) closed = out[o].close() && closed;
    bfq_destroy(c);
    if (!closed) { perror("bfq_bam"); return 1; }
    bfq_phase_report("bfq_bam");
    typedef unsigned long long ull;
    if (tags && verbose)
        fprintf(stderr, "bfq_bam: tags: %llu written, %llu dropped, %llu bytes of text\n", (ull)TS.tags_written, (ull)TS.tags_dropped, (ull)TS.tag_bytes);
    if (mode == 'l')
        printf("{\"n_ref\": %llu, \"header_bytes\": %llu, \"records\": %llu, \"written\": [%llu, %llu, %llu], \"bytes\": [%llu, %llu, %llu], \"skipped\": %llu, "
               "\"reversed\": %llu, \"no_qual\": %llu, \"clamped_quals\": %llu, \"pieces\": %llu, \"walkers\": %llu, \"dead\": %llu, \"repaired\": %llu, \"rounds\": %llu}\n",
               (ull)S.n_ref, (ull)S.header_bytes, (ull)S.records, (ull)S.written[0], (ull)S.written[1], (ull)S.written[2], (ull)outLen[0], (ull)outLen[1], (ull)outLen[2],
               (ull)S.skipped, (ull)S.reversed, (ull)S.no_qual, (ull)S.clamped_quals, (ull)S.pieces, (ull)S.walkers, (ull)S.dead, (ull)S.repaired, (ull)S.rounds);
    else
        printf("%llu records: %llu + %llu + %llu reads, %llu + %llu + %llu bytes%s\n", (ull)S.records, (ull)nReads[0], (ull)nReads[1], (ull)nReads[2], (ull)outLen[0],
               (ull)outLen[1], (ull)outLen[2], mode == 't' ? " verified" : "");
    return 0;
}
