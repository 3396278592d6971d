"""Block sharding of a FASTQ file across GPUs: the reference's own split / merge rule, on bytes.

BFQzip_parallel.py:288-323 (split_fastq): size_block = num_reads // t, num_blocks = num_reads // size_block;
blocks 0..num_blocks-2 take size_block consecutive reads, the LAST block takes all remaining reads (so
num_blocks may exceed t).  Paired mode (split_fastq_2, :325-360): block k of file 2 (same rule on file 2) is
appended to block k of file 1; after the run the first lines(block k of file 1) output lines go to OUT_1, the
rest to OUT_2 (:153-172).  Every block is a fully independent run of the hot path (`BFQzip.py <block> --rebuild
-0 [--headers]`, :277-285: own eBWT, clusters, inversion); the merge is an ordered concatenation (`cat`, :174-177).

Here: one process per GPU (torch.distributed; backend nccl = RCCL on GPUs, gloo in the CPU tests).  Nothing is
done per read on the host:
  * the input files are memory-mapped; every rank counts the newlines of ITS share of the bytes (host threads
    in libbfqhip.so), the per-chunk counts are all-gathered (a few thousand integers), and block boundaries
    are located by line number inside single 1 MiB chunks;
  * a block = 1 byte range (2 with -p: the mate block appended) handed to Engine.fastq_job, which parses,
    runs the whole path and formats the FASTQ text / the --m2/--m3 streams on the GPU;
  * blocks are dealt round-robin; after every round of `world` blocks the output sizes (6 integers per block)
    are all-gathered and each rank writes its block's bytes at their final offsets (pwrite) -- there is no
    data-path collective and no gather of payload bytes.
"""
import os
import sys
import numpy as np

CHUNK = 1 << 20


def split_blocks(num_reads, t):
    """[(first_read, end_read)] per block, exactly as split_fastq() cuts them (t == 0: one block, :302-303)."""
    if num_reads <= 0:
        return []
    t = int(t)
    size_block = num_reads if t <= 0 else num_reads // t
    if size_block == 0:                       # more threads than reads: the reference divides by zero; one block
        return [(0, num_reads)]
    num_blocks = num_reads // size_block
    out = []
    for b in range(num_blocks):
        s = b * size_block
        e = num_reads if b == num_blocks - 1 else s + size_block
        out.append((s, e))
    return out


def blocks_of_rank(num_blocks, rank, world):
    return list(range(rank, num_blocks, world))


class Comm:
    """The few integers the ranks exchange; single process when torch.distributed is not initialised."""

    def __init__(self, dist=None, device=None):
        self.dist, self.device = dist, device
        self.rank = dist.get_rank() if dist is not None else 0
        self.world = dist.get_world_size() if dist is not None else 1

    def all_gather_i64(self, vec):
        """vec: int64 array of the same length on every rank -> array [world, len]."""
        vec = np.ascontiguousarray(vec, np.int64)
        if self.dist is None or self.world == 1:
            return vec[None, :].copy()
        import torch
        dev = self.device if self.device is not None else torch.device("cpu")
        mine = torch.from_numpy(vec).to(dev)
        got = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(got, mine)
        return np.stack([g.cpu().numpy() for g in got])

    def barrier(self):
        if self.dist is not None and self.world > 1:
            self.dist.barrier()

    def _direct(self, t):
        return self.dist is not None and self.dist.get_backend() == "nccl" and t.is_cuda

    def broadcast_(self, t, src):
        """In-place broadcast of a tensor (RCCL on GPU tensors; through the host under gloo)."""
        if self.dist is None or self.world == 1 or t.numel() == 0:
            return
        if self._direct(t) or not t.is_cuda:
            self.dist.broadcast(t, src)
        else:
            h = t.cpu()
            self.dist.broadcast(h, src)
            t.copy_(h)

    def all_reduce_sum_(self, t):
        if self.dist is None or self.world == 1 or t.numel() == 0:
            return
        if self._direct(t) or not t.is_cuda:
            self.dist.all_reduce(t)
        else:
            h = t.cpu()
            self.dist.all_reduce(h)
            t.copy_(h)


def pwrite_all(fd, data, offset, host=None):
    """`data` into the open file at `offset`: through the library's threaded writer (bfq_file_put: fallocate + shared
    mapping, several threads -- a 9.5 GB output takes a Python os.pwrite 1.6 s) when the engine's host helpers offer it,
    else os.pwrite until everything is written (one call moves at most 0x7ffff000 bytes on Linux)."""
    put = getattr(host, "file_put", None) if host is not None else None
    if put is not None and len(data) >= (1 << 20):
        put(fd, data, offset)
        return
    mv = memoryview(data).cast("B")
    done = 0
    while done < len(mv):
        done += os.pwrite(fd, mv[done:done + (1 << 30)], offset + done)


def map_file(path):
    """Read-only uint8 view of a file (nothing is read until touched)."""
    if os.path.getsize(path) == 0:
        return np.zeros(0, np.uint8)
    return np.memmap(path, dtype=np.uint8, mode="r")


class TextIndex:
    """Line index of a memory-mapped text, built by all ranks together: rank r counts the newlines of the r-th
    share of the chunks; cum[i] = newlines before chunk i."""

    def __init__(self, buf, comm, count_fn, nth_fn, chunk=CHUNK):
        self.buf, self.chunk, self.nth_fn = buf, chunk, nth_fn
        n = len(buf)
        nch = (n + chunk - 1) // chunk
        per = (nch + comm.world - 1) // comm.world if nch else 0
        lo, hi = min(nch, comm.rank * per), min(nch, (comm.rank + 1) * per)
        mine = np.zeros(per, np.int64)
        if hi > lo:
            mine[:hi - lo] = count_fn(buf[lo * chunk:min(n, hi * chunk)], chunk).astype(np.int64)
        allc = comm.all_gather_i64(mine).reshape(-1)[:nch] if per else np.zeros(0, np.int64)
        self.cum = np.zeros(nch + 1, np.int64)
        np.cumsum(allc, out=self.cum[1:])
        self.num_lines = int(self.cum[-1]) + (1 if n and buf[n - 1] != 10 else 0)

    def line_start(self, k):
        """Byte offset at which line k (0-based) starts; k == num_lines -> end of the text."""
        n = len(self.buf)
        if k <= 0:
            return 0
        if k >= self.num_lines:
            return n
        j = k - 1                                                   # the newline that ends line k-1
        ci = int(np.searchsorted(self.cum, j, side="right")) - 1
        b = ci * self.chunk
        off = self.nth_fn(self.buf[b:min(n, b + self.chunk)], j - int(self.cum[ci]))
        if off < 0:
            raise RuntimeError("line index inconsistent with the text (file changed while mapped?)")
        return b + off + 1


def byte_blocks(index, t):
    """[(byte0, byte1, n_reads)] per block of split_fastq(); num_reads = num_lines // 4 (:298)."""
    if index.num_lines % 4:
        raise ValueError("FASTQ: number of lines is not a multiple of 4")
    out = []
    for s, e in split_blocks(index.num_lines // 4, t):
        out.append((index.line_start(4 * s), index.line_start(4 * e), e - s))
    return out


def output_names(inputs, out, paired):
    """Merged FASTQ names as BFQzip_parallel.py:142-153 builds them (+ the stream names of BFQzip.py:192-251)."""
    root1, ext1 = os.path.splitext(inputs[0])
    if not out:
        fq = [root1 + ".cat" + ext1]
        base = [root1 + ".cat"]
        if paired:
            root2, ext2 = os.path.splitext(inputs[1])
            fq.append(root2 + ".cat" + ext2); base.append(root2 + ".cat")
    elif paired:
        fq = [out + "_1" + ext1, out + "_2" + ext1]
        base = [out + "_1", out + "_2"]
    else:
        fq = [out + ext1]
        base = [out]
    return [{"fastq": f, "dna": f + ".dna", "qs": f + ".qs", "hdr": b + ".h"} for f, b in zip(fq, base)]


def inflated_name(path, out):
    """Where a bgzip-compressed input is inflated to: beside the outputs (the directory of -o, else the input's), the name
    without its .gz / .bgz and with .inflated in front of the extension (in.fastq.gz -> in.inflated.fastq)."""
    base = os.path.basename(path)
    for z in (".gz", ".bgz", ".bgzf"):
        if base.endswith(z):
            base = base[:-len(z)]
            break
    root, ext = os.path.splitext(base)
    return os.path.join(os.path.dirname(out) if out else os.path.dirname(path), root + ".inflated" + ext)


def inflate_inputs(eng, comm, inputs, out="", log=None, gunzip=False):
    """A bgzip-compressed (BGZF) input is inflated on the GPU to a plain file beside the outputs before the line index is
    built (eng.bgzf_inflate_files), by rank 0, and the run goes on with that file: returns (the new input list, the files
    written).  The blocks are cut by line number, which a compressed file does not give: one extra trip of the text through
    the file system.  gunzip (--gunzip): an input that is gzip but not BGZF goes through eng.gzip_inflate_files, its deflate
    streams inflated side by side; without it such a file keeps the library's refusal."""
    new, tmp = [], []
    for p in inputs:
        with open(p, "rb") as f:
            head = f.read(2)
        if head[:2] != b"\x1f\x8b":
            new.append(p)
            continue
        q = inflated_name(p, out)
        if gunzip:
            from . import api
            with open(p, "rb") as f:
                gunzip_this = not api.bgzf_probe(f.read(1 << 17))   # (a whole first member: at most 64 KiB)
        if comm.rank == 0 and gunzip and gunzip_this:
            n, st = eng.gzip_inflate_files(p, q)                    # (a damaged file: the library's message)
            if log:
                log(f"gunzip: {st}")
        elif comm.rank == 0:
            n = eng.bgzf_inflate_files(p, q)                        # (plain gzip, a damaged file: the library's message)
            if log:
                log(f"inflate: {p} -> {q}, {n} bytes")
        new.append(q)
        tmp.append(q)
    if tmp:
        comm.barrier()
    return new, tmp


def bam_names(path, out, split):
    """Where --bam converts a BAM input to: beside the outputs (the directory of -o, else the input's), <name>.fastq, or
    <name>_1.fastq and <name>_2.fastq for the one file of a paired run."""
    root = os.path.splitext(os.path.basename(path))[0]
    d = os.path.dirname(out) if out else os.path.dirname(path)
    return [os.path.join(d, root + tag + ".fastq") for tag in (("_1", "_2") if split else ("",))]


def convert_bam_inputs(eng, comm, inputs, out="", paired=False, log=None, tags=None):
    """--bam: an input for which api.bam_probe holds is converted to FASTQ text on the GPU (eng.bam_to_fastq_files) by rank 0
    before the line index is built, as inflate_inputs does for .gz, and the run goes on with that file: returns (the new
    input list, the files written).  With -p and a single BAM input the file is split by its READ1 / READ2 flags, with the
    pairing check (records that are neither are left out), and the run goes on as a two-file paired run.  tags (--bam-tags):
    the aux tags written behind the names (api.bam_opts)."""
    from . import api
    new, tmp = [], []
    for p in inputs:
        with open(p, "rb") as f:
            is_bam = api.bam_probe(f.read(1 << 17))                 # (a whole first member: at most 64 KiB)
        if not is_bam:
            new.append(p)
            continue
        split = paired and len(inputs) == 1
        q = bam_names(p, out, split)
        if comm.rank == 0:                                          # (a damaged or unpaired file: the library's message)
            n, reads, st = eng.bam_to_fastq_files(p, (None, q[0], q[1]) if split else (q[0], None, None), split=int(split), paired_check=int(split),
                                                      **(dict(tags=tags) if tags else {}))
            if log:
                log(f"bam: {p} -> {q}, {reads} reads, {st}" + (f", {st.tags}" if tags else ""))
        new += q
        tmp += q
    if tmp:
        comm.barrier()
    return new, tmp


def split_interleaved_input(eng, comm, inputs, out="", log=None):
    """--interleaved: the one input -- a FASTQ file with the mates alternating -- is split on the GPU into <name>_1.fastq and
    <name>_2.fastq beside the outputs (bam_names, as the one paired BAM of --bam -p) by rank 0, in strict mode with the name
    check (eng.fastq_deinterleave_files), and the run goes on as a two-file paired run: returns (the new input list, the
    files written, None) -- or, for a file that is not properly paired, (the old list, the files written, the library's
    message) on every rank, before any block runs."""
    from . import api
    q = bam_names(inputs[0], out, True)
    why = None
    if comm.rank == 0:
        try:
            n, reads, st = eng.fastq_deinterleave_files(inputs[0], (None, q[0], q[1]), check_names=1, orphans=0)
            if log:
                log(f"interleaved: {inputs[0]} -> {q}, {reads[1]} pairs, {st}")
        except api.BfqError as e:
            why = str(e)
    if comm.all_gather_i64([1 if why else 0])[0, 0]:
        return list(inputs), q, why or "the interleaved input was refused on rank 0"
    comm.barrier()
    return q, q, None


def repair_inputs(eng, comm, inputs, out="", log=None):
    """--repair: the mates of the inputs -- two mate files that may each have lost reads, in any order, or one mixed file --
    are matched by name on the GPU of rank 0 (eng.fastq_repair_files) into <name>_1.fastq and <name>_2.fastq beside the
    outputs (bam_names), what finds no mate into <name>_singles.fastq, which the run does not touch; the run goes on as a
    two-file paired run: returns (the new input list, the two files written, None) -- or, for a refusal, (the old list,
    the files written, the library's message) on every rank, before any block runs."""
    from . import api
    q = bam_names(inputs[0], out, True)
    singles = q[0][:-len("_1.fastq")] + "_singles.fastq"
    why = None
    if comm.rank == 0:
        try:
            texts = (None, inputs[0], inputs[1]) if len(inputs) == 2 else (inputs[0], None, None)
            n, reads, st = eng.fastq_repair_files(texts, (singles, q[0], q[1]))
            if log:
                log(f"repair: {' '.join(inputs)} -> {q}, {reads[1]} pairs; {reads[0]} singletons -> {singles}, {st}")
        except api.BfqError as e:
            why = str(e)
            if os.path.exists(singles):
                os.remove(singles)
    if comm.all_gather_i64([1 if why else 0])[0, 0]:
        return list(inputs), q, why or "the inputs were refused on rank 0"
    comm.barrier()
    return q, q, None


def dedup_names(inputs, out, paired):
    """Where --dedup writes: beside the outputs (bam_names), (<name>.dedup.fastq, <name>.dups.fastq), or with -p
    (<name>.dedup_1.fastq, <name>.dedup_2.fastq, <name>.dups_1.fastq, <name>.dups_2.fastq): (the kept files, the removed ones)"""
    base = bam_names(inputs[0], out, False)[0][:-len(".fastq")]
    tags = ("_1", "_2") if paired else ("",)
    return [base + ".dedup" + t + ".fastq" for t in tags], [base + ".dups" + t + ".fastq" for t in tags]


def dedup_inputs(eng, comm, inputs, out="", paired=False, best=False, log=None):
    """--dedup: exact duplicates -- reads, or with -p pairs, with equal sequences -- are removed on the GPU of rank 0
    (eng.fastq_dedup_files) before the run: the kept records go into the files of dedup_names() and the run goes on with them,
    the removed ones into <name>.dups[_1|_2].fastq, which the run does not touch.  best: the unit with the best qualities of
    every group is kept, else the first.  Returns (the new input list, the kept files, None) -- or, for a refusal, (the old
    list, the kept files, the library's message) on every rank, before any block runs."""
    from . import api
    kept, dups = dedup_names(inputs, out, paired)
    why = None
    if comm.rank == 0:
        try:
            ol, dl, st = eng.fastq_dedup_files(inputs, kept, dups, keep=1 if best else 0)
            if log:
                log(f"dedup: {' '.join(inputs)} -> {kept}: {st.units} {'pairs' if paired else 'reads'}, {st.kept} kept, {st.removed} removed -> {dups} "
                    f"({st.dup_groups} groups of duplicates, the largest of {st.max_group} at record {st.max_group_first})")
        except api.BfqError as e:
            why = str(e)
            for q in dups:
                if os.path.exists(q):
                    os.remove(q)
    if comm.all_gather_i64([1 if why else 0])[0, 0]:
        return list(inputs), kept, why or "the inputs were refused on rank 0"
    comm.barrier()
    return kept, kept, None


def merge_interleaved_output(eng, comm, outputs, path, check_names, log=None):
    """--interleaved-out: after the run rank 0 merges the two merged output texts into one file with the mates alternating
    (eng.fastq_interleave_files), the names compared when the run kept them.  Returns None, or the library's message on every
    rank."""
    from . import api
    comm.barrier()
    why = None
    if comm.rank == 0:
        try:
            n, st = eng.fastq_interleave_files((None, outputs[0], outputs[1]), path, check_names=int(check_names))
            if log:
                log(f"interleaved-out: {' '.join(outputs)} -> {path}, {n} bytes, {st}")
        except api.BfqError as e:
            why = str(e)
    if comm.all_gather_i64([1 if why else 0])[0, 0]:
        return why or "the merge was refused on rank 0"
    return None


def reordered_names(inputs, mode):
    """Where --reorder puts its intermediate files: <root>.reordered<ext> (mode 2, BFQzip_parallel.py:398) or
    <root>.random<ext> (mode 1, :421) beside every input."""
    tag = ".reordered" if mode == 2 else ".random"
    return [root + tag + ext for root, ext in (os.path.splitext(p) for p in inputs)]


def reorder_inputs(eng, comm, inputs, mode, k=21, seed=0, paired=False, log=None, perm_path=None):
    """--reorder {1,2} of BFQzip_parallel.py (:59-75): the reads of the input(s) are written in another order (mode 2: by
    locus, mode 1: seeded random; eng.fastq_reorder_files -- mates move together) by rank 0, and the run goes on with those
    files: returns the new input list (the reference replaces args.input and re-derives the output names from it, :403-404,
    :432-435).  mode 0: the inputs as they are.  perm_path (--keep-order): rank 0 also writes the permutation there, as a
    BFQPERM1 file (restore_order() and `bfq_restore -P` undo it)."""
    if not mode:
        return list(inputs)
    if mode not in (1, 2):
        raise ValueError("--reorder: 0 (no reorder), 1 (random) or 2 (locus)")
    src = list(inputs[:2 if paired else 1])
    dst = reordered_names(src, mode)
    if comm.rank == 0:
        keep = dict(perm_path=perm_path) if perm_path else {}
        sizes, n = eng.fastq_reorder_files(src, dst, mode=mode, k=k, seed=seed, **keep)
        if log:
            log(f"reorder {mode}: {n} reads, {sum(sizes)} bytes -> {' '.join(dst)}" + (f", permutation -> {perm_path}" if perm_path else ""))
    comm.barrier()
    return dst + list(inputs[len(src):])


def restore_order(eng, comm, outputs, perm_path, log=None):
    """--keep-order after the run: rank 0 replaces the merged FASTQ output (or the two mates' outputs, in one call) by its
    un-reordered form (eng.fastq_unreorder_files with the permutation reorder_inputs kept), through temporary files in the
    same directories and os.replace, after the barrier that ends the writes."""
    import tempfile
    comm.barrier()
    if comm.rank == 0:
        tmps = []
        try:
            for o in outputs:
                fd, t = tempfile.mkstemp(prefix=os.path.basename(o) + ".", suffix=".tmp", dir=os.path.dirname(o) or ".")
                os.close(fd)
                tmps.append(t)
            sizes, n = eng.fastq_unreorder_files(list(outputs), tmps, perm_path)
            for t, o in zip(tmps, outputs):
                os.replace(t, o)
            tmps = []
            if log:
                log(f"keep-order: {n} reads, {sum(sizes)} bytes back in input order -> {' '.join(outputs)}")
        finally:
            for t in tmps:
                if os.path.exists(t):
                    os.remove(t)
    comm.barrier()


def write_reports(eng, comm, before, outputs, log=None):
    """--report after the run: rank 0 compares every merged FASTQ output with the input it came from, in the same order
    (eng.fastq_compare_files), and writes `<output fastq>.report.json` (the keys of CompareReport.as_dict()), one per mate,
    after the barrier that ends the writes.  Returns the report names."""
    import json
    comm.barrier()
    paths = [o + ".report.json" for o in outputs]
    if comm.rank == 0:
        for src, o, p in zip(before, outputs, paths):
            rep = eng.fastq_compare_files(src, o)
            with open(p, "w") as f:
                json.dump(rep.as_dict(), f)
                f.write("\n")
            if log:
                log(f"report: {o} against {src}: {rep.n_diffs} differing positions in {rep.reads_changed} of {rep.n_reads} reads -> {p}")
    comm.barrier()
    return paths


def write_kmer_reports(eng, comm, before, outputs, k, log=None):
    """--report-kmers K after the run: rank 0 counts the k-mers of every merged FASTQ output against the input it came from
    (eng.fastq_kmers_files: nothing is paired, so any order of the reads will do and no permutation file is read) and writes
    `<output fastq>.kmers.json` (the keys of KmerReport.as_dict()), one per mate, beside what --report writes.  Returns the
    report names."""
    import json
    comm.barrier()
    paths = [o + ".kmers.json" for o in outputs]
    if comm.rank == 0:
        for src, o, p in zip(before, outputs, paths):
            rep = eng.fastq_kmers_files(src, o, k=k)
            with open(p, "w") as f:
                json.dump(rep.as_dict(), f)
                f.write("\n")
            if log:
                log(f"k-mers: {o} against {src}: k {k}: {rep.only_a} of {rep.distinct_a} distinct k-mers removed, {rep.only_b} created, "
                    f"{rep.solid_lost} solid ones lost -> {p}")
    comm.barrier()
    return paths


KINDS = ("fastq", "dna", "qs", "hdr")


def _pinned_outputs(kinds, cap):
    """Page-locked output buffers of `cap` bytes for the wanted kinds (direct DMA instead of the staging pipeline)."""
    from . import api
    pins = {k: api.PinnedBuffer(cap) for k in kinds}
    return pins, {k: p.array for k, p in pins.items()}


def run_files(eng, comm, inputs, t, names, paired=False, headers=False, want_fastq=True, want_streams=False,
              want_hdr=False, out_bufs=None, log=None, compress=False, pinned=False, name_codec=False, qual_codec=False, edits_path=None):
    """The whole multi-GPU job.  eng: Engine-like (fastq_job, text_line_counts/text_nth_newline via `eng.host`).
    Returns per-rank totals {"blocks", "reads", "bases", "stats"} (stats summed over this rank's blocks).
    compress: step 5 too (BFQzip.py:253-275) -- every block's share of every output goes through the stream codec
    (eng.stream_compress) and the files `<name>.bsc` hold one BFQRANS2 container per block, in block order
    (`bsc d` / stream_decompress read them back as one stream).  name_codec: the header shares go through
    eng.names_compress instead (the tokenised BFQNAME1 container where it is shorter; restore takes either), qual_codec:
    the quality shares through eng.quals_compress (BFQQUAL1 where it is shorter).  edits_path (--keep-bases; one input
    file): every block's job also makes the BFQEDIT1 member of its base edits (fastq_job(edits=True)) and the file holds
    the members in block order, like every other output."""
    host = eng.host
    bufs = [map_file(p) for p in inputs]
    idx = [TextIndex(b, comm, host.text_line_counts, host.text_nth_newline) for b in bufs]
    blocks = [byte_blocks(i, t) for i in idx]
    nblocks = len(blocks[0])                                         # the blocks of file 1 drive the run (:97-119)
    kinds = [k for k, w in zip(KINDS, (want_fastq, want_streams, want_streams, want_hdr)) if w]
    nout = 2 if paired else 1
    if compress:
        names = [{k: v + ".bsc" for k, v in nm.items()} for nm in names]
    if comm.rank == 0:                                               # create / truncate the outputs once
        for o in range(nout):
            for k in kinds:
                open(names[o][k], "wb").close()
    comm.barrier()
    if edits_path and comm.rank == 0:
        open(edits_path, "wb").close()
        comm.barrier()
    elif edits_path:
        comm.barrier()
    fds = {(o, k): os.open(names[o][k], os.O_RDWR) for o in range(nout) for k in kinds}       # (read too: the writer maps the file)
    fd_edits = os.open(edits_path, os.O_RDWR) if edits_path else -1
    cursor = np.zeros((nout, 5), np.int64)                           # next free byte of every output file (column 4: the edits)
    tot = {"blocks": 0, "reads": 0, "bases": 0, "stats": {}}
    out_bufs = out_bufs if out_bufs is not None else {}
    pins = None
    if pinned and not out_bufs and nblocks:
        # sized from the line index: the largest block's bytes (+ its mate's) bound every one of its outputs
        big = max((blocks[0][k][1] - blocks[0][k][0]) + ((blocks[1][k][1] - blocks[1][k][0]) if paired and k < len(blocks[1]) else 0)
                  for k in range(nblocks))
        pins, out_bufs = _pinned_outputs(kinds, big + 5 * 2 + 64)
    rounds = (nblocks + comm.world - 1) // comm.world
    for rd in range(rounds):
        k = rd * comm.world + comm.rank
        sizes = np.zeros((2, 5), np.int64)
        res = None
        if k < nblocks:
            b0, b1, _ = blocks[0][k]
            parts = [bufs[0][b0:b1]]
            if paired and k < len(blocks[1]):
                c0, c1, _ = blocks[1][k]
                parts.append(bufs[1][c0:c1])
            res = eng.fastq_job(parts, keep_headers=headers, fastq=want_fastq, streams=want_streams, hdr=want_hdr,
                                out=out_bufs, **(dict(edits=True) if edits_path else {}))
            if edits_path:
                sizes[0, 4] = len(res.edits)
            cut = {"fastq": res.part_fastq_off, "dna": res.part_stream_off, "qs": res.part_stream_off,
                   "hdr": res.part_hdr_off}
            raw = {"fastq": res.fastq, "dna": res.dna, "qs": res.qs, "hdr": res.hdr}
            blobs = {}
            for o in range(nout):
                for ki, kind in enumerate(KINDS):
                    if kind in kinds:
                        lo = cut[kind][o] if o < len(parts) else cut[kind][-1]
                        hi = cut[kind][o + 1] if o < len(parts) else cut[kind][-1]
                        sizes[o, ki] = hi - lo
                        if compress:                                 # this mate's share of the block as one container
                            code = (eng.names_compress if (name_codec and kind == "hdr") else
                                    eng.quals_compress if (qual_codec and kind == "qs") else eng.stream_compress)
                            blobs[(o, kind)] = code(raw[kind][lo:hi])
                            sizes[o, ki] = len(blobs[(o, kind)])
            tot["blocks"] += 1; tot["reads"] += res.n_reads; tot["bases"] += res.total_bases
            for key, v in res.stats.items():
                if key.startswith("n_"):
                    continue
                tot["stats"][key] = tot["stats"].get(key, 0) + v
            if log:
                log(f"block {k + 1}/{nblocks}: {res.n_reads} reads, {res.total_bases} bases")
        allsz = comm.all_gather_i64(sizes.reshape(-1)).reshape(comm.world, 2, 5)
        before = allsz[:comm.rank].sum(axis=0)                       # blocks of this round that come first
        if res is not None:
            data = {"fastq": res.fastq, "dna": res.dna, "qs": res.qs, "hdr": res.hdr}
            for o in range(nout):
                for ki, kind in enumerate(KINDS):
                    if kind in kinds and sizes[o, ki]:
                        lo = cut[kind][o]
                        piece = blobs[(o, kind)] if compress else data[kind][lo:lo + int(sizes[o, ki])]
                        pwrite_all(fds[(o, kind)], piece, int(cursor[o, ki] + before[o, ki]), host)
            if edits_path:
                pwrite_all(fd_edits, res.edits, int(cursor[0, 4] + before[0, 4]), host)
        cursor += allsz.sum(axis=0)[:nout]
    for fd in fds.values():
        os.close(fd)
    if fd_edits >= 0:
        os.close(fd_edits)
    if pins:
        for pb in pins.values():
            pb.free()
    comm.barrier()
    return tot


def restore_files(eng, comm, dna_path, qs_path, hdr_path, out_path, log=None, edits_path=None):
    """The way back of run_files(.., compress=True) on as many GPUs as it was written with: the three .bsc files are mapped,
    every rank computes the group plan from the container headers (eng.host.restore_groups: one group per block), group k
    goes to rank k mod world (eng.fastq_restore(.., groups=(k, 1))), after every round the text lengths are all-gathered
    (one integer per rank) and every rank writes its text at its final offset.  No payload collective, nothing per read on
    the host.  hdr_path may be None ("@" lines).  The two mates of a paired run are two invocations.  Returns this rank's
    totals {"groups", "reads", "bytes"} with "bytes_all" = the length of the whole text.  edits_path (--keep-bases): the
    BFQEDIT1 file the run wrote, one member per block = per group: the text of group k gets the input's bases back from
    member k (eng.fastq_unedit) before it is written."""
    from . import api
    host = eng.host
    dna, qs = map_file(dna_path), map_file(qs_path)
    hdr = map_file(hdr_path) if hdr_path is not None else None
    plan = host.restore_groups(dna, qs, hdr)
    members = api.edits_members(map_file(edits_path)) if edits_path is not None else None
    if members is not None and len(members) != len(plan):
        raise ValueError(f"{edits_path}: {len(members)} members for an archive of {len(plan)} blocks")
    if comm.rank == 0:
        open(out_path, "wb").close()
    comm.barrier()
    fd = os.open(out_path, os.O_RDWR)
    tot = {"groups": 0, "reads": 0, "bytes": 0}
    cursor = 0
    try:
        rounds = (len(plan) + comm.world - 1) // comm.world
        for rd in range(rounds):
            k = rd * comm.world + comm.rank
            text, n = None, 0
            if k < len(plan):
                text, n = eng.fastq_restore(dna, qs, hdr, groups=(k, 1))
                if members is not None:
                    text, _ = eng.fastq_unedit(text, members[k])
                tot["groups"] += 1; tot["reads"] += n; tot["bytes"] += len(text)
                if log:
                    log(f"group {k + 1}/{len(plan)}: {n} reads, {len(text)} bytes")
            allsz = comm.all_gather_i64(np.array([len(text) if text is not None else 0], np.int64)).reshape(-1)
            if text is not None and len(text):
                pwrite_all(fd, text, cursor + int(allsz[:comm.rank].sum()), host)
            cursor += int(allsz.sum())
    finally:
        os.close(fd)
    comm.barrier()
    tot["bytes_all"] = cursor
    return tot


def deal_piles(counts, world):
    """The two-symbol piles (first 1..5, second 1..5; a second symbol 0 = suffixes of one base: never in a cluster) dealt to
    the ranks, largest first to the least loaded rank: [[(s, s2), ...] per rank] -- the same list on every rank."""
    piles = sorted(((int(counts[s][s2]), s, s2) for s in range(1, 6) for s2 in range(1, 6) if counts[s][s2]), reverse=True)
    load = [0] * world
    mine = [[] for _ in range(world)]
    for cnt, s, s2 in piles:
        r = min(range(world), key=lambda k: (load[k], k))
        load[r] += cnt
        mine[r].append((s, s2))
    return mine


def run_global(eng, comm, inputs, names, headers=False, want_fastq=True, want_streams=False, want_hdr=False, log=None, out_bufs=None,
               pinned=False):
    """ONE collection over all ranks with the result of the unsharded run (k_global.hip): every rank parses its share of the
    file(s), the terminated text is exchanged, the two-symbol piles of the global eBWT are dealt to the ranks, the edits are
    combined with one all-reduce, and every rank writes its own reads.  Two input files (paired end) form ONE collection --
    all reads of file 1, then all reads of file 2, as `BFQzip_parallel.py -p -t 0` appends them -- and give two outputs."""
    import time
    import torch
    dev = torch.device(eng.tensor_device)
    host = eng.host
    tm = {}
    t_last = [time.perf_counter()]

    def lap(name):
        if dev.type == "cuda":
            torch.cuda.synchronize()
        now = time.perf_counter(); tm[name] = round(tm.get(name, 0.0) + now - t_last[0], 4); t_last[0] = now

    def tsync():
        """The engine runs on its own non-blocking stream (bfq_api.hip: hipStreamNonBlocking) and returns synchronised; what
        torch has queued on ITS stream (clones, copies, collectives) must be complete before the engine reads or overwrites
        those tensors -- stated here explicitly instead of resting on the timing helper."""
        if dev.type == "cuda":
            torch.cuda.current_stream().synchronize()
    nf = len(inputs)
    W, r = comm.world, comm.rank
    bufs = [map_file(p) for p in inputs]
    parts, tlen = [], 0
    for buf in bufs:                                                 # my share of every file: reads R r / W .. R (r + 1) / W
        idx = TextIndex(buf, comm, host.text_line_counts, host.text_nth_newline)
        if idx.num_lines % 4:
            raise ValueError("FASTQ: number of lines is not a multiple of 4")
        R = idx.num_lines // 4
        b0, b1 = idx.line_start(4 * (R * r // W)), idx.line_start(4 * (R * (r + 1) // W))
        parts.append(buf[b0:b1]); tlen += b1 - b0
    lap("index")
    Np, Tp = eng.glob_begin(parts)                                    # reads / bases of each of my parts
    lap("upload+parse")
    sz = comm.all_gather_i64(np.array([Np[f] + Tp[f] for f in range(nf)], np.int64))       # rows [rank][file]
    # global text = file 0's parts in rank order, then file 1's: base[f][k] = first row of rank k's part of file f
    flat = np.concatenate([[0], np.cumsum(sz.T.reshape(-1))]).astype(np.int64)
    base = flat[:-1].reshape(nf, W)
    n = int(flat[-1])
    # 64 bytes of padding: the pile kernels read the text 16 bytes at a time (k_piles.hip)
    t8 = torch.empty(n + 64, dtype=torch.uint8, device=dev); q8 = torch.empty_like(t8)
    t8[n:] = 0; q8[n:] = 0
    myrows = [int(sz[r][f]) for f in range(nf)]
    if sum(myrows):
        lt = torch.empty(sum(myrows), dtype=torch.uint8, device=dev); lq = torch.empty_like(lt)
        eng.glob_local_text(lt, lq)                                   # my parts back to back
        o = 0
        for f in range(nf):
            t8[int(base[f][r]):int(base[f][r]) + myrows[f]] = lt[o:o + myrows[f]]
            q8[int(base[f][r]):int(base[f][r]) + myrows[f]] = lq[o:o + myrows[f]]
            o += myrows[f]
        del lt, lq
    for f in range(nf):                                               # every rank ends up with the whole text
        for src in range(W):
            lo, hi = int(base[f][src]), int(base[f][src]) + int(sz[src][f])
            comm.broadcast_(t8[lo:hi], src)
            comm.broadcast_(q8[lo:hi], src)
    lap("text exchange")
    tot = {"blocks": 1, "reads": sum(Np), "bases": sum(Tp), "stats": {}, "seconds": tm}
    # The stream files' sizes are known from here on (one byte per row): they are created now, and this rank's byte range of
    # each is mapped and populated by a helper thread while the piles are sorted -- the streams then leave the GPU straight
    # into the files' pages, with nothing to write afterwards (one input file; with two the shares of both go through a buffer).
    kinds = [k for k, w in zip(KINDS, (want_fastq, want_streams, want_streams, want_hdr)) if w]
    if comm.rank == 0:
        for f in range(nf):
            for k in kinds:
                open(names[f][k], "wb").close()
    comm.barrier()
    direct, direct_thread = {}, None
    FileRange = getattr(host, "FileRange", None)
    if want_streams and nf == 1 and FileRange is not None and not out_bufs and not pinned and sum(myrows) >= (1 << 20):
        import threading
        off0 = int(sz[:r, 0].sum())

        def _map_streams():
            for kind in ("dna", "qs"):
                fd = os.open(names[0][kind], os.O_RDWR)
                fr = FileRange(fd, off0, myrows[0])
                os.close(fd)
                if fr.array is not None:
                    direct[kind] = fr
        direct_thread = threading.Thread(target=_map_streams)
        direct_thread.start()
    sym = torch.empty_like(t8); qual = torch.empty_like(t8)
    if n:
        tsync()
        counts = eng.glob_pile_counts(t8, n)
        mine = deal_piles(counts, W)[r]
        eng.glob_init_out(t8, q8, n, sym, qual)
        if W > 1:
            osym, oqual = sym.clone(), qual.clone()
            tsync()                                                  # the clones are read before the piles edit sym / qual
        for s, s2 in mine:
            st = eng.glob_run_pile(t8, q8, n, s, s2, sym, qual)
            for key, v in st.items():
                if not key.startswith("n_"):
                    tot["stats"][key] = tot["stats"].get(key, 0) + v
            if log:
                log(f"pile {'#ACGNT'[s]}{'#ACGNT'[s2]}: {st['n_rows']} rows, {st['num_clust']} clusters")
        del t8, q8
        lap("piles")
        segs = [(int(base[f][r]), int(base[f][r]) + myrows[f]) for f in range(nf)]
        if W > 1:
            sym ^= osym; qual ^= oqual                               # what this rank's piles changed (zero elsewhere)
            comm.all_reduce_sum_(sym); comm.all_reduce_sum_(qual)
            dna = torch.cat([osym[a:b] ^ sym[a:b] for a, b in segs]); qs = torch.cat([oqual[a:b] ^ qual[a:b] for a, b in segs])
            del osym, oqual
        elif nf == 1:                                                # one rank, one file: the edited streams are the result as they are
            dna, qs = sym[segs[0][0]:segs[0][1]], qual[segs[0][0]:segs[0][1]]
        else:
            dna = torch.cat([sym[a:b] for a, b in segs]); qs = torch.cat([qual[a:b] for a, b in segs])
        del sym, qual
        lap("delta all-reduce")
    else:
        dna = torch.empty(0, dtype=torch.uint8, device=dev); qs = dna.clone()
    tsync()
    pins = None
    if direct_thread is not None:
        direct_thread.join()
        if len(direct) == 2:
            out_bufs = {k: fr.array for k, fr in direct.items()}
        else:
            for fr in direct.values():
                fr.close()
            direct = {}
    if pinned and not out_bufs:
        pins, out_bufs = _pinned_outputs([k for k, w in zip(KINDS, (want_fastq, want_streams, want_streams, want_hdr)) if w], int(tlen) + 64)
    res = eng.glob_finish(dna, qs, keep_headers=headers, fastq=want_fastq, streams=want_streams, hdr=want_hdr, text_len=int(tlen), nparts=nf,
                          **({"out": out_bufs} if out_bufs else {}))
    # outputs at their final offsets: output f = the shares of part f of all ranks, in rank order
    data = {"fastq": res.fastq, "dna": res.dna, "qs": res.qs, "hdr": res.hdr}
    cut = {"fastq": res.part_fastq_off, "dna": res.part_stream_off, "qs": res.part_stream_off, "hdr": res.part_hdr_off}
    sizes = np.zeros((nf, 4), np.int64)
    for f in range(nf):
        for ki, kind in enumerate(KINDS):
            if kind in kinds:
                sizes[f, ki] = cut[kind][f + 1] - cut[kind][f]
    allsz = comm.all_gather_i64(sizes.reshape(-1)).reshape(W, nf, 4)
    before = allsz[:comm.rank].sum(axis=0)
    for f in range(nf):
        for ki, kind in enumerate(KINDS):
            if kind in kinds:
                if kind in direct:                                   # already in the file's pages
                    assert int(before[f, ki]) == direct[kind].offset and int(sizes[f, ki]) == direct[kind].nbytes
                    continue
                fd = os.open(names[f][kind], os.O_RDWR)
                if sizes[f, ki]:
                    pwrite_all(fd, data[kind][cut[kind][f]:cut[kind][f + 1]], int(before[f, ki]), host)
                os.close(fd)
    if pins or direct:
        del res, data
        out_bufs = None
    if pins:
        for pb in pins.values():
            pb.free()
    for fr in direct.values():
        fr.close()
    comm.barrier()
    lap("format+write")
    keys = sorted(tot["stats"]) if tot["stats"] else ["num_clust", "num_clust_discarded", "num_clust_amb_discarded", "num_clust_mod",
                                                     "num_clust_alleq", "bases_inside", "qs_smoothed", "modified"]
    allst = comm.all_gather_i64(np.array([tot["stats"].get(k, 0) for k in keys], np.int64))
    tot["stats_all_ranks"] = {k: int(v) for k, v in zip(keys, allst.sum(axis=0))}
    return tot


def main(argv=None):
    """`python -m torch.distributed.run --nproc-per-node G -m bfqzip_amd.parallel in.fastq [in2.fastq -p] -o OUT -t n [-H]`

    The multi-GPU counterpart of `BFQzip_parallel.py in.fastq [in2.fastq -p] -o OUT -t n -0` (same flags, same
    block split, same output names: OUT<ext> or OUT_1<ext> / OUT_2<ext>), one block per GPU at a time.  --m2 / --m3
    additionally write the streams BFQzip.py cuts with sed (<fastq>.dna, <fastq>.qs; --m3: OUT.h and header lines
    kept).  Without torchrun it runs all blocks on GPU 0.
    `... -m bfqzip_amd.parallel --restore DNA.bsc QS.bsc [HDR.bsc] -o OUT.fq` is the way back of a --compress run
    (restore_files)."""
    import argparse
    import torch
    from . import api
    ap = argparse.ArgumentParser(prog="bfqzip_amd.parallel")
    ap.add_argument("input", nargs="+")
    ap.add_argument("-o", "--out", default="")
    ap.add_argument("-T", "--mcl", default="", help="minimum context length (bfq_int -k)")
    ap.add_argument("-Q", "--rv", default="", help="constant replacement value (bfq_int -v)")
    ap.add_argument("-H", "--headers", action="store_true", help="store original headers")
    ap.add_argument("-0", "--m0", action="store_true", help="do not compress (the default here; see --compress)")
    ap.add_argument("--compress", action="store_true",
                    help="step 5 on the GPU: every output goes through the stream codec, files get the suffix .bsc (one container per block)")
    ap.add_argument("--names", action="store_true",
                    help="with --compress: read names (OUT.h) as tokens, the BFQNAME1 container where it is shorter than the general one")
    ap.add_argument("--quals", action="store_true",
                    help="with --compress: quality lines coded by their place in the read, the BFQQUAL1 container where it is shorter than the general one")
    ap.add_argument("-p", "--paired", action="store_true")
    ap.add_argument("-t", "--threads", type=int, default=0, help="number of blocks")
    ap.add_argument("-c", "--check", action="store_true", help="accepted: records are always checked on the GPU")
    ap.add_argument("-v", type=int, default=0)
    ap.add_argument("--m2", action="store_true", help="also write <fastq>.dna and <fastq>.qs (BFQzip.py:231-249)")
    ap.add_argument("--m3", action="store_true", help="--m2 plus OUT.h, headers kept (BFQzip.py:60-64,192-201)")
    ap.add_argument("--streams-only", action="store_true", help="with --m2/--m3: do not write the merged FASTQ text")
    ap.add_argument("--pinned", action="store_true", help="page-locked output buffers (direct DMA)")
    ap.add_argument("--global", dest="glob", action="store_true",
                    help="ONE eBWT over the whole input, its piles dealt to the GPUs: the result of the unsharded run (-t is ignored)")
    ap.add_argument("--reorder", type=int, default=0, choices=(0, 1, 2),
                    help="reorder the reads before the input is cut into blocks (0: no reorder, 1: random, 2: by locus): "
                         "writes <input>.random<ext> / <input>.reordered<ext> and runs on those")
    ap.add_argument("--keep-order", action="store_true",
                    help="with --reorder 1|2: keep the permutation as <first reordered intermediate>.perm and give the merged "
                         "FASTQ text back in input order (streams and --compress containers stay in run order: bfq_restore -P)")
    ap.add_argument("--keep-bases", action="store_true",
                    help="bases back exactly: every block's job also keeps the input's byte at every base the run changed; the "
                         "BFQEDIT1 members go to OUT.edits in block order (one input file; not with --global).  With --restore: "
                         "OUT.edits is read and the text comes back with the input's bases")
    ap.add_argument("--edits", default="", metavar="PATH", help="with --keep-bases: the BFQEDIT1 file, instead of <output>.edits")
    ap.add_argument("--reorder-k", type=int, default=21, help="k-mer length of --reorder 2 (8..32)")
    ap.add_argument("--seed", type=int, default=0, help="seed of --reorder 1")
    ap.add_argument("--report", action="store_true",
                    help="after the run, compare every merged FASTQ output with the input in the same order on the GPU and write "
                         "<output fastq>.report.json (needs the uncompressed merged FASTQ text: not with --streams-only or --compress)")
    ap.add_argument("--report-kmers", type=int, default=0, metavar="K",
                    help="after the run, count the K-mers (8..31) of every merged FASTQ output against the input on the GPU and write "
                         "<output fastq>.kmers.json: which k-mers the run removed, kept and created (any read order; same limits as --report)")
    ap.add_argument("--restore", action="store_true",
                    help="the way back: the inputs are DNA.bsc QS.bsc [HDR.bsc] of a --compress run, -o OUT.fq the FASTQ file to write; "
                         "group k of the archive (one per block) is restored by rank k mod world")
    ap.add_argument("--keep-inflated", action="store_true",
                    help="a bgzip-compressed input is inflated to <name>.inflated<ext> beside the outputs first: keep that file")
    ap.add_argument("--gunzip", action="store_true",
                    help="a .gz input that is gzip but not BGZF (gzip, pigz, bcl2fastq) is inflated on the GPU too, its deflate streams "
                         "side by side; without this such a file is refused")
    ap.add_argument("--bam", action="store_true",
                    help="a BAM input (unaligned or aligned) is converted to <name>.fastq beside the outputs on the GPU first "
                         "(--keep-inflated keeps it); with -p one BAM file is split into <name>_1.fastq / <name>_2.fastq with the pairing check")
    ap.add_argument("--bam-out", default="", metavar="PATH",
                    help="with --bam, one BAM input and a merged FASTQ output: after the run the output text(s) are written back into "
                         "the SEQ and QUAL fields of the input's records on the GPU and the result goes to PATH (with -p the two texts "
                         "meet the READ1 / READ2 records; with -H the names are compared); an index of the input does not fit PATH")
    ap.add_argument("--ubam-out", default="", metavar="PATH",
                    help="with a merged FASTQ output: after the run the output text becomes an unaligned BAM on the GPU of rank 0 "
                         "and goes to PATH (with -p both merged texts become one paired uBAM, the names compared with -H); "
                         "not with --bam-out, --restore, --streams-only or --compress")
    ap.add_argument("--bam-tags", default="", metavar="LIST",
                    help="aux tags through the FASTQ header lines: '*' = every tag, or a list (BC,RX).  With --bam the selected tags of "
                         "a record are written behind its name as <tab>XX:T:value; with --ubam-out the fields XX:T:value of the header "
                         "lines become tags of the records; needs kept headers (-H or --m3); --bam-out keeps the input's tags as they are")
    ap.add_argument("--interleaved", action="store_true",
                    help="the one input is a FASTQ file with the mates alternating (bwa mem -p, fastp --interleaved_in): it is split on the "
                         "GPU into <name>_1.fastq / <name>_2.fastq beside the outputs first, with the name check (--keep-inflated keeps "
                         "them), and the run goes on as -p on those; a file that is not properly paired ends the run")
    ap.add_argument("--interleaved-out", default="", metavar="PATH",
                    help="with -p and a merged FASTQ output: after the run the two output texts are merged on the GPU of rank 0 into one "
                         "file with the mates alternating at PATH (the names compared with -H or --m3); not with --restore, "
                         "--streams-only or --compress")
    ap.add_argument("--repair", action="store_true",
                    help="the mates are matched by name on the GPU first, wherever they stand: with -p the two inputs are mate files that "
                         "may each have lost reads; one input is a mixed file (/1 and /2 say which mate a record is).  The run goes on as "
                         "-p on <name>_1.fastq / <name>_2.fastq beside the outputs (--keep-inflated keeps them); what finds no mate goes to "
                         "<name>_singles.fastq, which the run does not touch; more than 1024 records of one name end the run")
    ap.add_argument("--dedup", action="store_true",
                    help="exact duplicates are removed on the GPU first: reads -- with -p pairs -- with equal sequences leave their first unit "
                         "behind.  Behind the inflation and --repair, in front of --reorder; the run goes on with <name>.dedup.fastq (-p: "
                         "<name>.dedup_1.fastq / <name>.dedup_2.fastq) beside the outputs (--keep-inflated keeps them); the removed records "
                         "go to <name>.dups[_1|_2].fastq, which the run does not touch")
    ap.add_argument("--dedup-best", action="store_true", help="--dedup, keeping the unit with the best qualities of every group of duplicates")
    ap.add_argument("--M", type=int, default=2); ap.add_argument("--B", type=int, default=0)
    a = ap.parse_args(argv)
    a.dedup = a.dedup or a.dedup_best
    if a.dedup and (a.restore or a.bam_out):
        print("=== ERROR ===\n--dedup removes records in front of a run: not with --restore or --bam-out", file=sys.stderr)
        return 1
    if a.dedup and not (a.bam or a.interleaved or a.repair) and len(a.input) != (2 if a.paired else 1):
        print("=== ERROR ===\n--dedup takes one input file, or two mate files with -p", file=sys.stderr)
        return 1
    if a.repair:
        why = None
        if a.restore or a.interleaved or a.bam:
            why = "--repair reads FASTQ text in front of a run: not with --restore, --interleaved or --bam"
        elif len(a.input) != (2 if a.paired else 1):
            why = "--repair takes two mate files with -p, or one mixed file"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    if a.interleaved:
        why = None
        if len(a.input) != 1 or a.restore:
            why = "--interleaved takes exactly one input, a FASTQ file with the mates alternating"
        elif a.bam:
            why = "--interleaved reads FASTQ text: one paired BAM input goes through --bam -p"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
        a.paired = True
    if a.interleaved_out:
        why = None
        if not a.paired:
            why = "--interleaved-out merges the two outputs of a paired run: it needs -p (or --interleaved)"
        elif a.restore:
            why = "--interleaved-out follows a run: not with --restore"
        elif ((a.m2 or a.m3) and a.streams_only) or (a.compress and not a.m0):
            why = "--interleaved-out merges the merged FASTQ texts: not with --streams-only or --compress"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    if a.bam_tags:
        why = None
        try:
            api._tag_list(a.bam_tags, "--bam-tags")
        except ValueError as e:
            why = str(e)
        if not why and not (a.headers or a.m3):
            why = "--bam-tags needs kept headers (-H or --m3): a run without them writes \"@\" alone and the tags would be lost"
        elif not why and not (a.bam or a.ubam_out):
            why = "--bam-tags applies to a --bam input and to --ubam-out: one of them"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    if a.ubam_out:
        why = None
        if a.bam_out:
            why = "--ubam-out makes new records, --bam-out patches those of the input: one of them"
        elif a.restore:
            why = "--ubam-out follows a run: not with --restore (bfq_restore -b writes a uBAM from the containers)"
        elif ((a.m2 or a.m3) and a.streams_only) or (a.compress and not a.m0):
            why = "--ubam-out converts the merged FASTQ text: not with --streams-only or --compress"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    if a.bam_out:
        why = None
        if not a.bam or len(a.input) != 1 or a.restore:
            why = "--bam-out needs --bam and exactly one BAM input"
        elif ((a.m2 or a.m3) and a.streams_only) or (a.compress and not a.m0):
            why = "--bam-out patches the merged FASTQ text: not with --streams-only or --compress"
        elif a.reorder and not a.keep_order:
            why = "--bam-out needs the reads in file order: --reorder only with --keep-order"
        if not why:
            try:
                with open(a.input[0], "rb") as f:
                    if not api.bam_probe(f.read(1 << 17)):               # (a whole first member: at most 64 KiB)
                        why = "--bam-out: the input is no BAM file"
            except OSError as e:
                why = f"--bam-out: {e}"
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    if a.keep_bases:
        why = None
        if a.glob:
            why = ("--keep-bases does not go with --global: the edits of a collection are made where one job holds its bases before and "
                   "after the run, and the global mode spreads them over the ranks; run the blocks without --global, or make the file "
                   "afterwards with bfq_edits -a IN.fq -b OUT.fq")
        elif not a.restore and (a.paired or len(a.input) != 1):
            why = "--keep-bases takes one input file: the member of a block covers both mates, the outputs of a paired run are cut by mate"
        elif not a.restore and a.keep_order and a.reorder and not ((a.m2 or a.m3) and a.streams_only) and not (a.compress and not a.m0):
            why = ("--keep-bases with --keep-order: the edits are in run order, the merged FASTQ text goes back to input order; use "
                   "--compress (bfq_restore -P PERM -E OUT.edits undoes both) or --streams-only")
        if why:
            print("=== ERROR ===\n" + why, file=sys.stderr)
            return 1
    elif a.edits:
        print("=== ERROR ===\n--edits names the file of --keep-bases", file=sys.stderr)
        return 1
    if a.restore and (len(a.input) not in (2, 3) or not a.out):
        print("=== ERROR ===\n--restore DNA.bsc QS.bsc [HDR.bsc] -o OUT.fq", file=sys.stderr)
        return 1
    if a.repair:
        a.paired = True
    if a.paired and len(a.input) != 2 and not ((a.bam or a.interleaved or a.repair) and len(a.input) == 1):
        print("=== ERROR ===\npaired end mode", file=sys.stderr)
        return 1
    if a.m3:
        a.headers = True
    if a.report_kmers and (not 8 <= a.report_kmers <= 31 or a.restore or ((a.m2 or a.m3) and a.streams_only) or (a.compress and not a.m0 and not a.glob)):
        print("=== ERROR ===\n--report-kmers K: K is 8..31, and it reads the merged FASTQ text: not with --restore, --streams-only or --compress", file=sys.stderr)
        return 1
    if a.report and (a.restore or ((a.m2 or a.m3) and a.streams_only) or (a.compress and not a.m0 and not a.glob)):
        print("=== ERROR ===\n--report compares the merged FASTQ text: not with --restore, --streams-only or --compress", file=sys.stderr)
        return 1
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
    if torch.cuda.device_count():
        torch.cuda.set_device(local)                                 # tensors of the global mode and RCCL use the engine's GPU
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("BFQ_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local) if (dist and dist.get_backend() == "nccl") else None
    comm = Comm(dist, dev)
    par = dict(m=5, M=a.M, B=a.B)                                    # -m 5: what BFQzip.py passes (BFQzip.py:215)
    if a.mcl:
        par["k"] = int(a.mcl)
    if a.rv:
        par["v"] = ord(a.rv)
    eng = api.Engine(local, **par)
    log = (lambda m: print(f"[rank {comm.rank}] {m}", flush=True)) if a.v else None
    if a.restore:
        tot = restore_files(eng, comm, a.input[0], a.input[1], a.input[2] if len(a.input) == 3 else None, a.out, log=log,
                            edits_path=(a.edits or os.path.splitext(a.out)[0] + ".edits") if a.keep_bases else None)
        if a.v:
            print(f"[rank {comm.rank}] {tot}", flush=True)
        eng.close()
        if dist:
            dist.destroy_process_group()
        return 0
    converted, bam_src = [], a.input[0]
    if a.bam:
        a.input, converted = convert_bam_inputs(eng, comm, a.input, a.out, paired=a.paired, log=log, tags=a.bam_tags or None)
        if a.paired and len(a.input) != 2:
            print("=== ERROR ===\npaired end mode", file=sys.stderr)
            return 1
    a.input, inflated = inflate_inputs(eng, comm, a.input, a.out, log=log, gunzip=a.gunzip)
    inflated = converted + inflated
    if a.interleaved:
        a.input, mates, why = split_interleaved_input(eng, comm, a.input, a.out, log=log)
        inflated += mates
        if why:                                                      # (not properly paired: the library's message; every rank leaves with it)
            if comm.rank == 0:
                print(f"=== ERROR ===\n--interleaved: {why}", file=sys.stderr)
                for q in inflated:
                    if os.path.exists(q) and not a.keep_inflated:
                        os.remove(q)
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    if a.repair:
        a.input, mates, why = repair_inputs(eng, comm, a.input, a.out, log=log)
        inflated += mates
        if why:                                                      # (the library's message; every rank leaves with it)
            if comm.rank == 0:
                print(f"=== ERROR ===\n--repair: {why}", file=sys.stderr)
                for q in inflated:
                    if os.path.exists(q) and not a.keep_inflated:
                        os.remove(q)
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    if a.dedup:
        a.input, kept, why = dedup_inputs(eng, comm, a.input, a.out, paired=a.paired, best=a.dedup_best, log=log)
        inflated += kept
        if why:                                                      # (the library's message; every rank leaves with it)
            if comm.rank == 0:
                print(f"=== ERROR ===\n--dedup: {why}", file=sys.stderr)
                for q in inflated:
                    if os.path.exists(q) and not a.keep_inflated:
                        os.remove(q)
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    perm_path = reordered_names(a.input[:1], a.reorder)[0] + ".perm" if (a.keep_order and a.reorder) else None
    keep = dict(perm_path=perm_path) if perm_path else {}
    original = list(a.input)
    a.input = reorder_inputs(eng, comm, a.input, a.reorder, k=a.reorder_k, seed=a.seed, paired=a.paired, log=log, **keep)
    names = output_names(a.input, a.out, a.paired)                   # after the replacement, as define_basename() in the reference
    streams = a.m2 or a.m3
    if a.glob:
        tot = run_global(eng, comm, a.input[:2 if a.paired else 1], names, headers=a.headers, want_fastq=not (streams and a.streams_only),
                         want_streams=streams, want_hdr=a.m3, log=log, pinned=a.pinned)
    else:
        tot = run_files(eng, comm, a.input, a.threads, names, paired=a.paired, headers=a.headers,
                        want_fastq=not (streams and a.streams_only), want_streams=streams, want_hdr=a.m3, log=log,
                        compress=a.compress and not a.m0, pinned=a.pinned, name_codec=a.names, qual_codec=a.quals,
                        edits_path=(a.edits or os.path.splitext(names[0]["hdr"])[0] + ".edits") if a.keep_bases else None)
    if perm_path:
        want_fastq = not (streams and a.streams_only)
        compress = a.compress and not a.m0 and not a.glob
        if want_fastq and not compress:
            restore_order(eng, comm, [n["fastq"] for n in names], perm_path, log=log)
        if log and comm.rank == 0 and (streams or compress):
            log(f"keep-order: the {'containers' if compress else 'raw streams'} stay in run order; pass {perm_path} to bfq_restore -P")
    if a.report:                                                     # against what is in the outputs' order: the originals unless the run reordered for good
        write_reports(eng, comm, original if (perm_path or not a.reorder) else a.input, [n["fastq"] for n in names], log=log)
    if a.report_kmers:                                               # (the original input always: the order does not matter)
        write_kmer_reports(eng, comm, original, [n["fastq"] for n in names], a.report_kmers, log=log)
    if a.bam_out:
        comm.barrier()
        failed = None
        if comm.rank == 0:
            fq = [n["fastq"] for n in names]
            try:
                n, st = eng.bam_patch_files(bam_src, (None, fq[0], fq[1]) if a.paired else (fq[0],), a.bam_out, split=int(a.paired), check_names=int(a.headers))
                if log:
                    log(f"bam-out: {bam_src} + {' '.join(fq)} -> {a.bam_out}, {n} bytes, {st}")
            except api.BfqError as e:                                # (a refusal: the library's message; every rank leaves with it)
                failed = e
                print(f"=== ERROR ===\n--bam-out: {e}", file=sys.stderr)
        if comm.all_gather_i64([1 if failed else 0])[0, 0]:
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    if a.ubam_out:
        comm.barrier()
        failed = None
        if comm.rank == 0:
            fq = [n["fastq"] for n in names]
            try:
                n, st = eng.fastq_to_bam_files((None, fq[0], fq[1]) if a.paired else (fq[0],), a.ubam_out, paired_check=int(a.paired and a.headers),
                                                   **(dict(tags=a.bam_tags) if a.bam_tags else {}))
                if log:
                    log(f"ubam-out: {' '.join(fq)} -> {a.ubam_out}, {n} bytes, {st}" + (f", {st.tags}" if a.bam_tags else ""))
            except api.BfqError as e:                                # (a refusal: the library's message; every rank leaves with it)
                failed = e
                print(f"=== ERROR ===\n--ubam-out: {e}", file=sys.stderr)
        if comm.all_gather_i64([1 if failed else 0])[0, 0]:
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    if a.interleaved_out:                                            # (after the order is restored: the outputs are what the user keeps)
        why = merge_interleaved_output(eng, comm, [n["fastq"] for n in names], a.interleaved_out, a.headers, log=log)
        if why:
            if comm.rank == 0:
                print(f"=== ERROR ===\n--interleaved-out: {why}", file=sys.stderr)
            eng.close()
            if dist:
                dist.destroy_process_group()
            return 1
    if inflated and not a.keep_inflated:
        comm.barrier()
        if comm.rank == 0:
            for q in inflated:
                os.remove(q)
    if a.v:
        print(f"[rank {comm.rank}] {tot}", flush=True)
    eng.close()
    if dist:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
