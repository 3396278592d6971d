// restore_main.cpp -- the way back from the compressed streams to a FASTQ file (not a tool of the reference, which leaves
// this to `7z x` / `bsc d` + `paste`):
//     bfq_restore -d OUT.fq.dna.bsc -q OUT.fq.qs.bsc [-H OUT.h.bsc] [-P PERM | -g | -G FIRST[:COUNT] | -l] [-E RUN.edits] [-z | -b [-a LIST|'*']] -o OUT.fq [-V]
// The inputs are what `bsc e`, bfq_fastq_job.compress_streams = 1 / 2 / 3 and parallel.py --compress write
// (include/bfqzip_hip.h, bfq_fastq_restore_fd).  -P PERM: the BFQPERM1 file `bfq_reorder -P` / `parallel.py --keep-order`
// wrote for the run: the records come back in the order of the original file (bfq_fastq_restore_ordered_fd).
// -g: block by block (bfq_fastq_restore_grouped_fd): the members of the inputs are cut into groups that decode on their own
// -- one per block of a sharded run -- and the device holds one group at a time, so the archive may be larger than the
// device; several BFQEBWT1 members are taken.  -G FIRST[:COUNT]: only those groups.  -l: the plan of the groups, one line
// each, and nothing else: no GPU is touched and no output is created.  -g / -G with -P is a usage error: records in the
// original order draw on all groups at once.  -z: OUT.fq is written as BGZF (.fq.gz: bfq_fastq_restore_bgzf_fd, the text is
// deflated on the device and never crosses to the host), with and without -P; not with -g / -G.  -b: the output is written as an
// unaligned BAM instead (OUT.bam: bfq_fastq_restore_bam_fd, the restored text becomes unpaired records on the device and those
// are deflated there), with and without -P; not with -z, -g / -G; with -a LIST|'*' the fields XX:T:value of the restored header
// lines become aux tags of the records (bfq_ubam_tag_opts, as bfq_bam -w -a).  -E RUN.edits: the BFQEDIT1 file of the run's base
// edits (`bfq_edits`, `parallel.py --keep-bases`): the text comes back with the input's bases (bfq_fastq_restore_edited_fd),
// with and without -P; not with -g / -G / -l (a grouped text goes through `bfq_edits -u`), -z or -b.  Exit status 0 on success; 1 with the library's message
// otherwise, and then OUT.fq is left empty.
#include <unistd.h>
#include <sys/mman.h>
#include <vector>
#include "cli_common.h"

static int usage(const char *argv0)
{
    fprintf(stderr, "usage: %s -d DNA.bsc -q QS.bsc [-H HEADERS.bsc] [-P PERM | -g | -G FIRST[:COUNT] | -l] [-E RUN.edits] [-z | -b [-a LIST|'*']] -o OUT.fq [-V]\n"
                    "  -d <arg>  container(s) of the DNA stream (OUT.fq.dna; BFQDNAC1 / BFQRANS2 members, or one BFQEBWT1) (REQUIRED)\n"
                    "  -q <arg>  container(s) of the quality stream (OUT.fq.qs) (REQUIRED)\n"
                    "  -H <arg>  container(s) of the header stream (OUT.h); without it every header line is \"@\"\n"
                    "  -P <arg>  BFQPERM1 file of the reordering the collection went through: the text in the order before it\n"
                    "  -E <arg>  BFQEDIT1 file of the run's base edits: the text with the input's bases; not with -g / -G / -l, -z, -b\n"
                    "  -g        block by block: one group of members (a block of a sharded run) on the device at a time\n"
                    "  -G <arg>  FIRST[:COUNT]: only these groups of the plan (COUNT omitted: to the end)\n"
                    "  -l        print the plan of the groups and exit (no GPU, no output file; -o not needed)\n"
                    "  -z        write the output as BGZF (OUT.fq.gz), deflated on the GPU; not with -g / -G\n"
                    "  -b        write the output as an unaligned BAM (OUT.bam), records made and deflated on the GPU; not with -z, -g / -G\n"
                    "  -a <arg>  with -b: the fields XX:T:value of the header lines become aux tags: '*' = every field, or a list (BC,RX)\n"
                    "  -o <arg>  output FASTQ (REQUIRED)\n"
                    "  -V        phase timeline on stderr\n", argv0);
    return 1;
}

// -l: index, members of the three inputs, compressed bytes, raw bytes, reads (? where a DNA member states none), text bound
static int list_groups(const InFile &fd, const InFile &fq, const InFile *fh)
{
    auto map = [](const InFile &f) { return f.size ? mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0) : MAP_FAILED; };
    void *md = map(fd), *mq = map(fq), *mh = fh ? map(*fh) : MAP_FAILED;
    const uint8_t *pd = md != MAP_FAILED ? (const uint8_t *)md : nullptr, *pq = mq != MAP_FAILED ? (const uint8_t *)mq : nullptr;
    const uint8_t *ph = mh != MAP_FAILED ? (const uint8_t *)mh : nullptr;
    static const uint8_t none = 0;
    if (!pd) pd = &none;                                                   // (an empty file: the library says so)
    if (!pq) pq = &none;
    if (fh && !ph) ph = &none;
    char why[512];
    int64_t G = bfq_fastq_restore_groups(pd, fd.size, pq, fq.size, ph, fh ? fh->size : 0, nullptr, 0, why, (int)sizeof why);
    std::vector<bfq_restore_group> g((size_t)(G > 0 ? G : 0));
    if (G > 0) G = bfq_fastq_restore_groups(pd, fd.size, pq, fq.size, ph, fh ? fh->size : 0, g.data(), (uint64_t)G, why, (int)sizeof why);
    if (G < 0) { fprintf(stderr, "bfq_restore: %s\n", why); return 1; }
    printf("# group  members(dna qs hdr)  compressed  raw  reads  text_bound\n");
    for (int64_t k = 0; k < G; k++) {
        const bfq_restore_group &r = g[(size_t)k];
        char reads[32];
        if (r.reads == ~0ull) snprintf(reads, sizeof reads, "?");
        else snprintf(reads, sizeof reads, "%llu", (unsigned long long)r.reads);
        printf("%lld  %lld %lld %lld  %llu  %llu  %s  %llu\n", (long long)k, (long long)bfq_stream_members(pd + r.dna_off, r.dna_len),
               (long long)bfq_stream_members(pq + r.qs_off, r.qs_len), (long long)(ph ? bfq_stream_members(ph + r.hdr_off, r.hdr_len) : 0),
               (unsigned long long)(r.dna_len + r.qs_len + r.hdr_len), (unsigned long long)(2 * r.raw_stream + r.raw_hdr), reads,
               (unsigned long long)r.text_bound);
    }
    printf("%lld groups\n", (long long)G);
    return 0;
}

int main(int argc, char **argv)
{
    bfq_phase("start");
    std::string dna, qs, hdr, perm, edits, output;
    bool grouped = false, list = false, bgzf = false, ubam = false, tags = false, verbose = false;
    bfq_ubam_tag_opts X = {};
    bfq_ubam_tag_stats TS = {};
    uint64_t first = 0, count = ~0ull;
    int opt;
    while ((opt = getopt(argc, argv, "d:q:H:P:E:o:gG:lzba:Vh")) != -1) {
        switch (opt) {
        case 'd': dna = optarg; break;
        case 'q': qs = optarg; break;
        case 'H': hdr = optarg; break;
        case 'P': perm = optarg; break;
        case 'E': edits = optarg; break;
        case 'o': output = optarg; break;
        case 'g': grouped = true; break;
        case 'G': {
            char *e = nullptr;
            grouped = true;
            first = strtoull(optarg, &e, 10);
            if (e == optarg || (*e && *e != ':')) return usage(argv[0]);
            if (*e == ':') { const char *q = e + 1; count = strtoull(q, &e, 10); if (e == q || *e) return usage(argv[0]); }
            break;
        }
        case 'l': list = true; break;
        case 'z': bgzf = true; break;
        case 'b': ubam = true; break;
        case 'a':
            if (!parse_tag_list(optarg, &X.n_tags, X.tag)) { fprintf(stderr, "bfq_restore: -a: '*', or at most 32 two-byte tags separated by commas\n"); return usage(argv[0]); }
            tags = true; break;
        case 'V': bfq_phase_enable(1); verbose = true; break;
        default: return usage(argv[0]);
        }
    }
    if (dna.empty() || qs.empty() || (output.empty() && !list)) return usage(argv[0]);
    if ((grouped || list) && !perm.empty()) {
        fprintf(stderr, "bfq_restore: -g / -G / -l do not go with the permutation -P %s: records in the original order draw on all groups at once; "
                        "restore the archive in one piece (without -g)\n", perm.c_str());
        return usage(argv[0]);
    }
    if (!edits.empty() && (grouped || list || bgzf || ubam)) {
        fprintf(stderr, "bfq_restore: -E does not go with -g / -G / -l (the edits count from the first read of the archive: restore in one piece, or "
                        "put the bases back into the grouped text with bfq_edits -u), nor with -z or -b\n");
        return usage(argv[0]);
    }
    if (bgzf && grouped) {
        fprintf(stderr, "bfq_restore: -z does not go with -g / -G: the grouped restore writes plain text; restore the archive in one piece (without -g), "
                        "or compress the text afterwards (bfq_bgzf -c)\n");
        return usage(argv[0]);
    }
    if (ubam && (bgzf || grouped)) {
        fprintf(stderr, "bfq_restore: -b does not go with -z (a BAM file is BGZF already) or with -g / -G (the grouped restore writes plain text)\n");
        return usage(argv[0]);
    }
    if (tags && !ubam) { fprintf(stderr, "bfq_restore: -a needs -b: tags are written into a BAM\n"); return usage(argv[0]); }
    if (tags) { bfq_ubam_default_opts(&X.o); X.o.reserved = BFQ_UBAM_OPTS_TAGS; X.stats = &TS; }
    InFile fd, fq, fh, fp, fe;
    if (!fd.open(dna) || !fq.open(qs) || (!hdr.empty() && !fh.open(hdr)) || (!perm.empty() && !fp.open(perm)) || (!edits.empty() && !fe.open(edits))) { fprintf(stderr, "bfq_restore: cannot read the inputs\n"); return 1; }
    if (list) return list_groups(fd, fq, hdr.empty() ? nullptr : &fh);
    OutFile outText;
    if (!outText.open(output)) { perror("bfq_restore"); return 1; }
    {   // the bound of the text from the container headers: the output's pages are prepared while the GPU starts up
        auto map = [](const InFile &f) { return f.size ? mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0) : MAP_FAILED; };
        void *md = map(fd), *mq = map(fq), *mh = hdr.empty() ? MAP_FAILED : map(fh);
        int64_t bound = -1;
        if (md != MAP_FAILED && mq != MAP_FAILED && (hdr.empty() || mh != MAP_FAILED)) {
            if (!grouped)
                bound = bfq_fastq_restore_bound((const uint8_t *)md, fd.size, (const uint8_t *)mq, fq.size, hdr.empty() ? nullptr : (const uint8_t *)mh, fh.size);
            else {                                                         // the plan's text bounds over the range; what is wrong with it the library says below
                const int64_t G = bfq_fastq_restore_groups((const uint8_t *)md, fd.size, (const uint8_t *)mq, fq.size,
                                                           hdr.empty() ? nullptr : (const uint8_t *)mh, fh.size, nullptr, 0, nullptr, 0);
                std::vector<bfq_restore_group> g((size_t)(G > 0 ? G : 0));
                if (G > 0) (void)bfq_fastq_restore_groups((const uint8_t *)md, fd.size, (const uint8_t *)mq, fq.size,
                                                          hdr.empty() ? nullptr : (const uint8_t *)mh, fh.size, g.data(), (uint64_t)G, nullptr, 0);
                bound = 0;
                for (uint64_t k = first; k < (uint64_t)(G > 0 ? G : 0) && k - first < count; k++) bound += (int64_t)g[(size_t)k].text_bound;
            }
        }
        if (md != MAP_FAILED) munmap(md, fd.size);
        if (mq != MAP_FAILED) munmap(mq, fq.size);
        if (mh != MAP_FAILED) munmap(mh, fh.size);
        if (bound < 0) { fprintf(stderr, "bfq_restore: the inputs are not containers (BFQDNAC1 / BFQRANS2 / BFQLINE1 / BFQNAME1 / BFQQUAL1 / BFQEBWT1)\n"); outText.close(); return 1; }
        if (bound >= (64 << 20) && !bgzf && !ubam) (void)bfq_output_prefault(outText.fd, (uint64_t)bound + 4096, (uint64_t)bound / 2);
    }
    bfq_params P;
    bfq_default_params(&P);
    bfq_ctx *c = create_on_free_gpu("bfq_restore", &P);
    if (!c) return 1;
    uint64_t outLen = 0, reads = 0, rawLen = 0;
    bfq_ubam_stats US = {};
    const int rc = ubam ? bfq_fastq_restore_bam_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, perm.empty() ? -1 : fp.fd, fp.size,
                                                   tags ? &X.o : nullptr, outText.fd, &outLen, &US)
                   : bgzf ? bfq_fastq_restore_bgzf_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, perm.empty() ? -1 : fp.fd, fp.size, 1,
                                                    outText.fd, &outLen, &rawLen, &reads)
                   : !edits.empty() ? bfq_fastq_restore_edited_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, perm.empty() ? -1 : fp.fd,
                                                                  fp.size, fe.fd, fe.size, outText.fd, &outLen, &reads)
                   : grouped ? bfq_fastq_restore_grouped_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, first, count, outText.fd, &outLen, &reads)
                   : perm.empty() ? bfq_fastq_restore_fd(c, fd.fd, fd.size, fq.fd, fq.size, hdr.empty() ? -1 : fh.fd, fh.size, outText.fd, &outLen, &reads)
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
    if (tags && verbose)
        fprintf(stderr, "bfq_restore: tags: %llu written, %llu fields dropped, %llu bytes of stream\n", (unsigned long long)TS.tags_written,
                (unsigned long long)TS.fields_dropped, (unsigned long long)TS.tag_bytes);
    if (ubam) printf("%llu records, %llu bytes of stream -> %llu bytes\n", (unsigned long long)US.records, (unsigned long long)US.raw_len, (unsigned long long)outLen);
    else if (bgzf) printf("%llu reads, %llu bytes -> %llu bytes\n", (unsigned long long)reads, (unsigned long long)rawLen, (unsigned long long)outLen);
    else printf("%llu reads, %llu bytes\n", (unsigned long long)reads, (unsigned long long)outLen);
    return 0;
}
