"""Host-side mirror of the reference's interface for the hot path.

The reference exposes this path only as executables driven by BFQzip.py /
BFQzip_ext.py (gsufsort|eGap -> bfq_int|bfq_ext).  `Engine` offers the same
operations as functions over numpy arrays, all executed by libbfqhip.so on the
GPU (no CPU fallback):

    build_ebwt(...)     ~ gsufsort <fq> --bwt --qs -o OUT        (BFQzip.py:184)
                        ~ eGap <fq> --qs --lcp --lbytes 1 -o OUT  (BFQzip_ext.py:177)
    smooth_invert(...)  ~ bfq_int -e OUT.bwt -q OUT.bwt.qs -o OUT.fq -m 5 ...   (BFQzip.py:215-222)
                        ~ bfq_ext ... -a OUT.1.lcp                (BFQzip_ext.py:208-214)
    run_reads(...)      = both, fused, nothing written in between

Parameter names and defaults are those of bfq_int's getopt flags
(bfq_int.cpp:883-935) plus the compile-time knobs M and B.
"""
import ctypes as C
import numpy as np
from . import _lib


class BfqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbfqhip error {code}: {msg}")
        self.code = code


def make_params(k=16, m=2, v=ord(">"), f=40, t=20, s=ord("#"), M=2, B=0, ext=0, piles=0, ws_cap_mib=0):
    p = _lib.Params()
    p.K, p.m, p.v, p.f, p.t, p.term, p.M, p.B, p.ext, p.piles, p.ws_cap_mib = k, m, v, f, t, s, M, B, ext, piles, ws_cap_mib
    return p


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _u8(text):
    """bytes / bytearray / ndarray / memmap slice -> contiguous uint8 ndarray (no copy when possible)."""
    if isinstance(text, np.ndarray):
        return text if (text.dtype == np.uint8 and text.flags.c_contiguous) else np.ascontiguousarray(text, np.uint8)
    return np.frombuffer(text, np.uint8)


class PinnedBuffer:
    """Page-locked host memory (bfq_host_alloc) as a uint8 numpy array: transferred by direct DMA."""

    def __init__(self, nbytes):
        self.L = _lib.lib()
        self.nbytes = int(nbytes)
        self.ptr = self.L.bfq_host_alloc(max(self.nbytes, 1))
        if not self.ptr:
            raise MemoryError(f"bfq_host_alloc({nbytes})")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr))[:self.nbytes]

    def free(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.L.bfq_host_free(self.ptr)
            self.ptr = None

    __del__ = free


class JobResult:
    """Outputs of Engine.fastq_job: arrays trimmed to their lengths + where every input part's share starts."""
    __slots__ = ("fastq", "dna", "qs", "hdr", "edits", "n_reads", "total_bases", "part_reads", "part_fastq_off",
                 "part_stream_off", "part_hdr_off", "stats")


def text_line_counts(buf, chunk=1 << 20, threads=0):
    """Number of newlines in every `chunk` bytes of a text (host threads, no GPU): uint64 array."""
    a = _u8(buf)
    nch = (len(a) + chunk - 1) // chunk
    counts = np.zeros(max(nch, 1), np.uint64)
    rc = _lib.lib().bfq_text_count_lines(_ptr(a) if len(a) else None, len(a), chunk, _ptr(counts), threads)
    if rc:
        raise BfqError(rc, "bfq_text_count_lines")
    return counts[:nch]


def text_nth_newline(buf, k):
    a = _u8(buf)
    return int(_lib.lib().bfq_text_nth_newline(_ptr(a) if len(a) else None, len(a), k))


def file_put(fd, data, offset, threads=0):
    """The bytes of `data` (uint8 array / bytes) into the open file `fd` at `offset` (bfq_file_put: several threads, no GPU)."""
    a = _u8(data)
    if len(a):
        rc = _lib.lib().bfq_file_put(fd, offset, _ptr(a), len(a), threads)
        if rc:
            raise BfqError(rc, "bfq_file_put")


class FileRange:
    """The byte range [offset, offset + nbytes) of an open file as a uint8 array whose pages are the file's (bfq_file_map:
    allocated, mapped and populated by a few threads): an output buffer that needs no writing afterwards.  .array is None
    when the file cannot be mapped.  close() unmaps."""

    def __init__(self, fd, offset, nbytes, threads=0):
        self.L = _lib.lib()
        self.offset, self.nbytes = int(offset), int(nbytes)
        self.ptr = self.L.bfq_file_map(fd, self.offset, self.nbytes, threads) if self.nbytes else None
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr)) if self.ptr else None

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self.L.bfq_file_unmap(self.ptr, self.offset, self.nbytes)
            self.ptr = None

    __del__ = close


ALL_GROUPS = (1 << 64) - 1
NO_READ = (1 << 64) - 1

DIFF_DTYPE = np.dtype([("read", "<u8"), ("pos", "<u4"), ("base_a", "u1"), ("base_b", "u1"), ("qual_a", "u1"), ("qual_b", "u1")])


class CompareReport:
    """What Engine.fastq_compare found (bfq_compare_report): the scalar fields as ints (first_changed_read: NO_READ when
    nothing differs), subst as a 6 x 6 uint64 array ([class of A's base][class of B's], classes A C G N T other), the
    histograms and position profiles as uint64 arrays, .diffs the listed positions as a structured array (DIFF_DTYPE, in
    (read, pos) order), .identical = no base and no quality differs."""

    def __init__(self, raw, diffs):
        for k in _lib.COMPARE_SCALARS:
            setattr(self, k, int(getattr(raw, k)))
        for k, n in _lib.COMPARE_ARRAYS:
            setattr(self, k, np.array(getattr(raw, k), np.uint64))
        self.subst = self.subst.reshape(_lib.CMP_SYMS, _lib.CMP_SYMS)
        self.diffs = diffs

    @property
    def identical(self):
        return self.n_diffs == 0

    def as_dict(self):
        """Plain ints and lists (JSON): the scalars (first_changed_read None when nothing differs), identical, subst as six
        rows, the histograms, and the position profiles cut after the last bin that holds a position."""
        d = {k: getattr(self, k) for k in _lib.COMPARE_SCALARS}
        if d["first_changed_read"] == NO_READ:
            d["first_changed_read"] = None
        d["identical"] = self.identical
        d["subst"] = [[int(v) for v in row] for row in self.subst]
        for k in ("qual_hist_a", "qual_hist_b", "changed_base_qual_hist"):
            d[k] = [int(v) for v in getattr(self, k)]
        nz = np.flatnonzero(self.pos_len)
        n = int(nz[-1]) + 1 if len(nz) else 0
        for k in ("pos_len", "pos_bases", "pos_quals", "pos_abs"):
            d[k] = [int(v) for v in getattr(self, k)[:n]]
        return d


KMER_DTYPE = np.dtype([("kmer", "<u8"), ("count_a", "<u4"), ("count_b", "<u4")])


class KmerReport:
    """What Engine.fastq_kmers found (bfq_kmer_report): the scalar fields as ints, hist_a / hist_b (256 bins), joint (16 x 16,
    [min(cA, 15)][min(cB, 15)]) and trans (3 x 3, [class in A][class in B], classes absent / weak / solid) as uint64 arrays,
    .listed the listed k-mers as a structured array (KMER_DTYPE, ascending), .solid_lost = trans[2][0], .unchanged = no k-mer's
    count differs."""

    def __init__(self, raw, listed):
        for k in _lib.KMER_SCALARS:
            setattr(self, k, int(getattr(raw, k)))
        for k, n in _lib.KMER_ARRAYS:
            setattr(self, k, np.array(getattr(raw, k), np.uint64))
        self.joint = self.joint.reshape(16, 16)
        self.trans = self.trans.reshape(3, 3)
        self.listed = listed

    @property
    def solid_lost(self):
        return int(self.trans[2, 0])

    @property
    def unchanged(self):
        return self.distinct_changed == 0

    def kmer_strings(self):
        """The listed k-mers as ACGT strings."""
        return ["".join("ACGT"[(int(v) >> (2 * (self.k - 1 - i))) & 3] for i in range(self.k)) for v in self.listed["kmer"]]

    def as_dict(self):
        """Plain ints and lists (JSON): every field of the report, and the list as [k-mer string, count_a, count_b]."""
        d = {k: getattr(self, k) for k in _lib.KMER_SCALARS}
        for k, _ in _lib.KMER_ARRAYS:
            d[k] = [int(v) for v in getattr(self, k).reshape(-1)]
        d["list"] = [[s, int(e["count_a"]), int(e["count_b"])] for s, e in zip(self.kmer_strings(), self.listed)]
        return d


def _kmer_call(call, k, solid, canonical, max_list, list_out, part_records):
    O = _lib.KmerOpts(k=k, solid=solid, canonical=1 if canonical else 0, reserved=0, part_records=int(part_records))
    buf = list_out if list_out is not None else np.zeros(max(int(max_list), 1), KMER_DTYPE)
    assert buf.dtype == KMER_DTYPE and len(buf) >= max_list
    raw = _lib.KmerReport()
    call(C.byref(O), C.byref(raw), _ptr(buf) if max_list else None, int(max_list))
    return KmerReport(raw, buf[:min(int(raw.n_listed), int(max_list))])


def fastq_kmers_host(a, b=None, k=21, solid=3, canonical=True, max_list=0, list_out=None, part_records=0):
    """bfq_fastq_kmers_host: the k-mer report of plain text a (against b) on one thread of the host, no GPU: a KmerReport.
    It states the algorithm; nothing falls back to it."""
    L = _lib.lib()
    a = _u8(a)
    b = _u8(b) if b is not None else None
    pad = np.zeros(1, np.uint8)

    def call(po, pr, pl, cap):
        rc = L.bfq_fastq_kmers_host(_ptr(a if len(a) else pad), len(a), _ptr(b if len(b) else pad) if b is not None else None,
                                    len(b) if b is not None else 0, po, pr, pl, cap)
        if rc:
            raise BfqError(rc, L.bfq_kmers_host_error().decode())
    return _kmer_call(call, k, solid, canonical, max_list, list_out, part_records)


def restore_groups(dna, qs, hdr=None):
    """The group plan of an archive (bfq_fastq_restore_groups: container headers only, no GPU): a list of dicts, one per
    group that decodes on its own -- a block of a sharded run -- with the keys of bfq_restore_group (dna_off, dna_len, qs_off,
    qs_len, hdr_off, hdr_len, raw_stream, raw_hdr, reads (None where a DNA member states none), text_bound) plus the member
    counts members = (dna, qs, hdr).  Inputs that do not group raise BfqError with the library's reason."""
    L = _lib.lib()
    dna, qs = _u8(dna), _u8(qs)
    hdr = _u8(hdr) if hdr is not None else None
    pad = np.zeros(1, np.uint8)                                      # (an empty input: a pointer the library can name as such)
    pd, pq, ph = (_ptr(a if len(a) else pad) if a is not None else None for a in (dna, qs, hdr))
    args = (pd, len(dna), pq, len(qs), ph, len(hdr) if hdr is not None else 0)
    why = C.create_string_buffer(512)
    G = int(L.bfq_fastq_restore_groups(*args, None, 0, why, len(why)))
    arr = (_lib.RestoreGroup * max(G, 1))()
    if G > 0:
        G = int(L.bfq_fastq_restore_groups(*args, arr, G, why, len(why)))
    if G < 0:
        raise BfqError(G, why.value.decode())
    out = []
    for k in range(G):
        g = {name: int(getattr(arr[k], name)) for name, _ in _lib.RestoreGroup._fields_}
        if g["reads"] == ALL_GROUPS:
            g["reads"] = None
        cnt = lambda a, off, n: int(L.bfq_stream_members(C.c_void_p(a.ctypes.data + off), n)) if a is not None and n else 0
        g["members"] = (cnt(dna, g["dna_off"], g["dna_len"]), cnt(qs, g["qs_off"], g["qs_len"]), cnt(hdr, g["hdr_off"], g["hdr_len"]))
        out.append(g)
    return out


class BgzfIndexError(BfqError):
    """bgzf_index met a member header it refuses: `members` well-formed members stand before it, it starts at byte `bad_off`."""

    def __init__(self, code, members, bad_off):
        super().__init__(code, f"not a BGZF member: member {members} at byte {bad_off}")
        self.members, self.bad_off = members, bad_off


def bgzf_probe(blob):
    """True when the bytes begin with a well-formed BGZF member header (a FASTQ text never does)."""
    blob = _u8(blob)
    return bool(len(blob)) and bool(_lib.lib().bfq_bgzf_probe(_ptr(blob), len(blob)))


def bgzf_index(blob):
    """The directory of a BGZF file: ([(in_off, out_off, in_len, out_len) per member], raw length); BgzfIndexError when a
    member header is refused."""
    blob = _u8(blob)
    L = _lib.lib()
    n, raw, bad = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = L.bfq_bgzf_index(_ptr(blob), len(blob), None, 0, C.byref(n), C.byref(raw), C.byref(bad))
    if rc != 0:
        raise BgzfIndexError(rc, int(n.value), int(bad.value))
    m = (_lib.BgzfMember * max(int(n.value), 1))()
    L.bfq_bgzf_index(_ptr(blob), len(blob), m, int(n.value), C.byref(n), C.byref(raw), C.byref(bad))
    return [(int(e.in_off), int(e.out_off), int(e.in_len), int(e.out_len)) for e in m[:int(n.value)]], int(raw.value)


def bgzf_deflate_bound(n):
    """bfq_bgzf_deflate_bound: the bytes the BGZF form of a text of n bytes takes at most (n + 31 per member of 65 280 + 28)."""
    return int(_lib.lib().bfq_bgzf_deflate_bound(int(n)))


def bgzf_deflate_model(text, level=1):
    """The BGZF form of a text by the host form of the writer (bfq_bgzf_deflate_host: one thread, no GPU) as a uint8 array:
    the statement of the format -- Engine.bgzf_deflate gives the same bytes.  level 0: every member stored."""
    text = _u8(text)
    L = _lib.lib()
    out = np.empty(bgzf_deflate_bound(len(text)), np.uint8)
    ol = C.c_uint64(0)
    rc = L.bfq_bgzf_deflate_host(_ptr(text) if len(text) else None, len(text), int(level), _ptr(out), len(out), C.byref(ol))
    if rc != 0:
        raise BfqError(rc, "bgzf_deflate_model: level other than 0 / 1, or an input that is already compressed (1f 8b)")
    return out[:int(ol.value)]


def gzip_probe(blob):
    """True when the bytes begin with a well-formed gzip member header (bfq_gzip_probe): plain gzip or BGZF."""
    blob = _u8(blob)
    return bool(len(blob)) and bool(_lib.lib().bfq_gzip_probe(_ptr(blob), len(blob)))


def _gzip_raise(rc, msg, needed):
    e = BfqError(rc, msg)
    e.needed = int(needed)                                         # the raw length, when the buffer was too small for it; else 0
    raise e


def gzip_inflate_host(blob, chunk=0, out=None):
    """(text, stats) of a gzip file by the host form of the side-by-side inflate (bfq_gzip_inflate_host: the steps of
    csrc/bfq_gzip.h by one thread, no GPU): the statement of the algorithm -- Engine.gzip_inflate gives the same bytes and the
    same stats.  `out`: a uint8 array to fill; one that is too small raises BfqError with .needed = the raw length and is
    left untouched.  A damaged file raises BfqError ("damaged gzip input: member <i> at byte <off>: <reason>")."""
    blob = _u8(blob)
    L = _lib.lib()
    st, ol = _lib.GzipStats(), C.c_uint64(0)
    if out is None:
        rc = L.bfq_gzip_inflate_host(_ptr(blob) if len(blob) else None, len(blob), int(chunk), None, 0, C.byref(ol), C.byref(st))
        if rc == 0:
            return np.empty(0, np.uint8), st
        if not ol.value:
            _gzip_raise(rc, L.bfq_gzip_host_error().decode(), 0)
        out = np.empty(int(ol.value), np.uint8)
    rc = L.bfq_gzip_inflate_host(_ptr(blob) if len(blob) else None, len(blob), int(chunk), _ptr(out), len(out), C.byref(ol), C.byref(st))
    if rc != 0:
        _gzip_raise(rc, L.bfq_gzip_host_error().decode(), ol.value)
    return out[:int(ol.value)], st


def _tag_list(tags, what):
    """the keys of a tag selection: "*" -> [] (every tag), "BC,RX" / b"BC,RX" / a sequence of keys -> [b"BC", b"RX"]"""
    if isinstance(tags, (str, bytes)):
        tags = [] if tags in ("*", b"*") else tags.split("," if isinstance(tags, str) else b",")
    keys = [t.encode() if isinstance(t, str) else bytes(t) for t in tags]
    if len(keys) > 32 or any(len(k) != 2 for k in keys):
        raise ValueError("%s: tags: '*', or at most 32 two-byte tags" % what)
    return keys


def _tag_ext(x, keys, stats):
    x.n_tags = len(keys)
    for j, k in enumerate(keys):
        x.tag[j][0], x.tag[j][1] = k[0], k[1]
    x.stats = C.pointer(stats)
    x.tag_stats = stats                                            # (kept alive with the options; the call fills it)
    return x


def bam_opts(exclude_flags=0x900, mate_suffix=1, default_qual=1, split=0, paired_check=0, piece=0, check_names=0, tags=None, strict_tags=0):
    """bfq_bam_opts (include/bfqzip_hip.h); the defaults are bfq_bam_default_opts'.  check_names: bam_patch* only.
    tags: None, or "*" (every aux tag) or "BC,RX" (those) into the header lines as \\tXX:T:value -- then a bfq_bam_tag_opts
    comes back, whose .tag_stats (a BamTagStats: tags_written, tags_dropped, tag_bytes) the call fills; the entry points hand
    it on as stats.tags.  strict_tags: refuse a selected tag that cannot be carried instead of leaving it out."""
    if tags is not None:
        x = _tag_ext(_lib.BamTagOpts(), _tag_list(tags, "bam_opts"), _lib.BamTagStats())
        x.o = bam_opts(exclude_flags, mate_suffix, default_qual, split, paired_check, piece, check_names)
        x.o.reserved, x.strict = _lib.BAM_OPTS_TAGS, int(strict_tags)
        return x
    o = _lib.BamOpts()
    o.check_names = int(check_names)
    o.exclude_flags, o.mate_suffix, o.default_qual, o.split, o.paired_check, o.piece = (int(exclude_flags), int(mate_suffix), int(default_qual), int(split),
                                                                                      int(paired_check), int(piece))
    return o


def bam_probe(blob):
    """True for a BAM file (bfq_bam_probe): the inflated stream itself ("BAM\\1"), or BGZF whose first member inflates to one."""
    blob = _u8(blob)
    return bool(len(blob)) and bool(_lib.lib().bfq_bam_probe(_ptr(blob), len(blob)))


def _bam_raise(rc, msg, needed):
    e = BfqError(rc, msg)
    e.needed = [int(v) for v in needed]                            # the three lengths, when a buffer was too small; else zeros
    raise e


def _bam_outs(outs):
    ptrs = (C.c_void_p * 3)(*[o.ctypes.data if len(o) else None for o in outs])
    caps = (C.c_uint64 * 3)(*[len(o) for o in outs])
    return ptrs, caps


def bam_to_fastq_host(raw, outs=None, **opts):
    """(texts[3], stats) of the INFLATED stream of a BAM file by the host form of the conversion (bfq_bam_to_fastq_host: the
    steps of csrc/bfq_bam.h by one thread, no GPU): the statement of the algorithm -- Engine.bam_to_fastq gives the same bytes
    and the same stats.  opts: bam_opts().  `outs`: three uint8 arrays to fill; one that is too small raises BfqError with
    .needed = the three lengths and all are left untouched.  Refusals raise BfqError ("damaged BAM input: ...")."""
    raw = _u8(raw)
    L = _lib.lib()
    O, st = bam_opts(**opts), _lib.BamStats()
    st.tags = getattr(O, "tag_stats", None)                         # the tag counts beside the stats (None without tags=): so at every call below
    ol, nr = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    src = _ptr(raw) if len(raw) else None
    if outs is None:
        rc = L.bfq_bam_to_fastq_host(src, len(raw), C.byref(O), None, None, ol, nr, C.byref(st))
        if rc != 0:
            _bam_raise(rc, L.bfq_bam_host_error().decode(), ol)
        outs = [np.empty(int(v), np.uint8) for v in ol]
    ptrs, caps = _bam_outs(outs)
    rc = L.bfq_bam_to_fastq_host(src, len(raw), C.byref(O), ptrs, caps, ol, nr, C.byref(st))
    if rc != 0:
        _bam_raise(rc, L.bfq_bam_host_error().decode(), ol)
    return [o[:int(n)] for o, n in zip(outs, ol)], st


def _bam_patch_raise(rc, msg, needed):
    e = BfqError(rc, msg)
    e.needed = int(needed)                                         # the capacity needed, when the buffer was too small; else 0
    raise e


_EMPTY_TEXT = np.zeros(1, np.uint8)                                # where an empty text (present, unlike None) points


def _bam_texts(texts):
    """the three texts of a bam_patch call (None: absent; fewer than three: the rest absent) as pointer and length arrays"""
    texts = [None if t is None else _u8(t) for t in list(texts) + [None] * (3 - len(texts))]
    if len(texts) != 3:
        raise ValueError("bam_patch: at most three texts")
    ptrs = (C.c_void_p * 3)(*[None if t is None else (t if len(t) else _EMPTY_TEXT).ctypes.data for t in texts])
    lens = (C.c_uint64 * 3)(*[0 if t is None else len(t) for t in texts])
    return texts, ptrs, lens


def bam_patch_host(stream, texts, out=None, **opts):
    """(the patched stream, stats) of the INFLATED stream of a BAM file with the reads of up to three FASTQ texts written
    back into it, by the host form (bfq_bam_patch_host: the steps of csrc/bfq_bam_patch.h by one thread, no GPU): the
    statement of the algorithm -- Engine.bam_patch_device gives the same bytes and the same stats.  texts[k] (None: absent)
    meets output k of bam_to_fastq with the same opts (bam_opts(); check_names=1 compares the names too).  `out`: a uint8 array
    of at least len(stream) to fill.  Refusals raise BfqError ("BAM patch: ...", "FASTQ: ...", "damaged BAM input: ...") and
    write nothing."""
    stream = _u8(stream)
    L = _lib.lib()
    keep, ptrs, lens = _bam_texts(texts)
    if out is None:
        out = np.empty(len(stream), np.uint8)
    O, st = bam_opts(**opts), _lib.BamPatchStats()
    rc = L.bfq_bam_patch_host(_ptr(stream) if len(stream) else None, len(stream), C.byref(O), ptrs, lens, _ptr(out) if len(out) else None, len(out), C.byref(st))
    if rc != 0:
        _bam_patch_raise(rc, L.bfq_bam_host_error().decode(), st.raw_len)
    return out[:len(stream)], st


def ubam_opts(mate_suffix=1, paired_check=0, level=1, header_text=None, rg_id=None, tags=None):
    """(bfq_ubam_opts, what it points to) (include/bfqzip_hip.h); the defaults are bfq_ubam_default_opts'.  header_text: bytes
    written as the BAM header's text (None: the default header); rg_id: bytes or str, RG:Z:<rg_id> on every record.
    tags: None, or "*" (every field XX:T:value of the header lines) or "BC,RX" (those) as aux tags of the records -- then a
    bfq_ubam_tag_opts comes back, whose .tag_stats (a UbamTagStats: tags_written, fields_dropped, tag_bytes) the call fills;
    the entry points hand it on as stats.tags."""
    if tags is not None:
        x = _tag_ext(_lib.UbamTagOpts(), _tag_list(tags, "ubam_opts"), _lib.UbamTagStats())
        o, keep = ubam_opts(mate_suffix, paired_check, level, header_text, rg_id)
        x.o = o
        x.o.reserved = _lib.UBAM_OPTS_TAGS
        x.held_rg = o                                              # (rg_id's bytes live with the plain options)
        return x, keep
    o = _lib.UbamOpts()
    o.mate_suffix, o.paired_check, o.level, o.reserved = int(mate_suffix), int(paired_check), int(level), 0
    keep = []
    if header_text is not None:
        h = np.frombuffer(bytes(header_text) + b"\0", np.uint8)
        keep.append(h)
        o.header_text, o.header_len = h.ctypes.data, len(h) - 1
    if rg_id is not None:
        o.rg_id = rg_id.encode() if isinstance(rg_id, str) else bytes(rg_id)
    return o, keep


def _ubam_raise(rc, msg, needed):
    e = BfqError(rc, msg)
    e.needed = int(needed)                                         # the capacity needed, when the buffer was too small; else 0
    raise e


def fastq_to_bam_host(texts, out=None, **opts):
    """(the INFLATED stream of an unaligned BAM, stats) made of up to three FASTQ texts by the host form
    (bfq_fastq_to_bam_host: the steps of csrc/bfq_ubam.h by one thread, no GPU): the statement of the algorithm --
    Engine.fastq_to_bam_device gives the same bytes and the same stats.  texts[0]: unpaired reads (flag 4); texts[1] and
    texts[2]: the mates of a paired run (flags 77 and 141, interleaved in front of the reads of texts[0]); None: absent.
    opts: ubam_opts().  `out`: a uint8 array to fill; one that is too small raises BfqError with .needed = the length,
    nothing written.  Refusals raise BfqError ("FASTQ to BAM: ...", "FASTQ: ...")."""
    L = _lib.lib()
    keep, ptrs, lens = _bam_texts(texts)
    O, held = ubam_opts(**opts)
    st, rl = _lib.UbamStats(), C.c_uint64(0)
    st.tags = getattr(O, "tag_stats", None)
    if out is None:
        rc = L.bfq_fastq_to_bam_host(ptrs, lens, C.byref(O), None, 0, C.byref(rl), C.byref(st))
        if rc != 0 and not rl.value:
            _ubam_raise(rc, L.bfq_ubam_host_error().decode(), 0)
        out = np.empty(int(rl.value), np.uint8)
    rc = L.bfq_fastq_to_bam_host(ptrs, lens, C.byref(O), _ptr(out) if len(out) else None, len(out), C.byref(rl), C.byref(st))
    if rc != 0:
        _ubam_raise(rc, L.bfq_ubam_host_error().decode(), rl.value)
    return out[:int(rl.value)], st


def pairs_opts(check_names=1, mate_suffix=1, orphans=0, reserved=0):
    """bfq_pairs_opts (include/bfqzip_hip.h); the defaults are bfq_pairs_default_opts'.  check_names: the keys of the two mates
    of every pair are compared; mate_suffix: a trailing /1 or /2 is no part of the key; orphans: the split pairs the records
    of every run of equal keys and sends what is left over to output 0; reserved must be 0."""
    o = _lib.PairsOpts()
    o.check_names, o.mate_suffix, o.orphans, o.reserved = int(check_names), int(mate_suffix), int(orphans), int(reserved)
    return o


def _pairs_raise(rc, msg, needed):
    e = BfqError(rc, msg)
    e.needed = [int(v) for v in needed] if hasattr(needed, "__len__") else int(needed)   # the lengths needed, when a buffer was too small; else 0
    raise e


def fastq_deinterleave_host(text, outs=None, **opts):
    """(texts[3], stats) of an interleaved FASTQ text split by the host form (bfq_fastq_deinterleave_host: the steps of
    csrc/bfq_pairs.h by one thread, no GPU): the statement of the algorithm -- Engine.fastq_deinterleave gives the same bytes,
    stats and messages.  texts[1] / texts[2]: the mates; texts[0]: the singletons of orphans=1.  opts: pairs_opts().  `outs`:
    three uint8 arrays to fill; one that is too small raises BfqError with .needed = the three lengths, nothing written.
    stats.n_reads: the reads per output."""
    text = _u8(text)
    L = _lib.lib()
    O, st = pairs_opts(**opts), _lib.PairsStats()
    ol, nr = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    src = _ptr(text) if len(text) else None
    if outs is None:
        rc = L.bfq_fastq_deinterleave_host(src, len(text), C.byref(O), None, None, ol, nr, C.byref(st))
        if rc != 0:
            _pairs_raise(rc, L.bfq_pairs_host_error().decode(), ol)
        outs = [np.empty(int(v), np.uint8) for v in ol]
    ptrs, caps = _bam_outs(outs)
    rc = L.bfq_fastq_deinterleave_host(src, len(text), C.byref(O), ptrs, caps, ol, nr, C.byref(st))
    if rc != 0:
        _pairs_raise(rc, L.bfq_pairs_host_error().decode(), ol)
    st.n_reads = [int(v) for v in nr]
    return [o[:int(n)] for o, n in zip(outs, ol)], st


def fastq_interleave_host(texts, out=None, **opts):
    """(the interleaved text, stats) of the mates texts[1] and texts[2] (and the reads of an optional texts[0] behind the
    pairs; None: absent) by the host form (bfq_fastq_interleave_host, no GPU): Engine.fastq_interleave gives the same bytes,
    stats and messages.  opts: pairs_opts().  `out`: a uint8 array to fill; one that is too small raises BfqError with
    .needed = the length, nothing written."""
    L = _lib.lib()
    keep, ptrs, lens = _bam_texts(texts)
    O, st, ol = pairs_opts(**opts), _lib.PairsStats(), C.c_uint64(0)
    if out is None:
        rc = L.bfq_fastq_interleave_host(ptrs, lens, C.byref(O), None, 0, C.byref(ol), C.byref(st))
        if rc != 0:
            _pairs_raise(rc, L.bfq_pairs_host_error().decode(), 0)
        out = np.empty(int(ol.value), np.uint8)
    rc = L.bfq_fastq_interleave_host(ptrs, lens, C.byref(O), _ptr(out) if len(out) else None, len(out), C.byref(ol), C.byref(st))
    if rc != 0:
        _pairs_raise(rc, L.bfq_pairs_host_error().decode(), ol.value)
    return out[:int(ol.value)], st


def repair_opts(mate_suffix=1, hash_bits=40, seed=0, reserved=(0, 0)):
    """bfq_repair_opts (include/bfqzip_hip.h); the defaults are bfq_repair_default_opts'.  mate_suffix: a trailing /1 or /2 is no
    part of the key (and, in text 0, says which mate a record is); hash_bits (1..40): the bits of the name hash the records
    are sorted by -- small values are a test knob, the outputs do not depend on it, nor on seed; reserved must be 0."""
    o = _lib.RepairOpts()
    o.mate_suffix, o.hash_bits, o.seed = int(mate_suffix), int(hash_bits), int(seed)
    o.reserved[0], o.reserved[1] = (int(reserved), 0) if not hasattr(reserved, "__len__") else (int(reserved[0]), int(reserved[1]))
    return o


def fastq_repair_host(texts, outs=None, **opts):
    """(texts[3], stats) of the texts (texts[1] and texts[2]: mate files; texts[0]: a mixed file; None: absent) with the mates
    matched by name by the host form (bfq_fastq_repair_host: the steps of csrc/bfq_pairs.h by one thread, no GPU): the
    statement of the algorithm -- Engine.fastq_repair gives the same bytes, stats and messages.  Result texts[1] / texts[2]:
    the mates, pair k at place k of both; texts[0]: the singletons.  opts: repair_opts().  `outs`: three uint8 arrays to fill;
    one that is too small raises BfqError with .needed = the three lengths, nothing written.  stats.n_reads: the reads per
    output."""
    L = _lib.lib()
    keep, ptrs, lens = _bam_texts(texts)
    O, st = repair_opts(**opts), _lib.RepairStats()
    ol, nr = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    if outs is None:
        rc = L.bfq_fastq_repair_host(ptrs, lens, C.byref(O), None, None, ol, nr, C.byref(st))
        if rc != 0:
            _pairs_raise(rc, L.bfq_pairs_host_error().decode(), ol)
        outs = [np.empty(int(v), np.uint8) for v in ol]
    optrs, caps = _bam_outs(outs)
    rc = L.bfq_fastq_repair_host(ptrs, lens, C.byref(O), optrs, caps, ol, nr, C.byref(st))
    if rc != 0:
        _pairs_raise(rc, L.bfq_pairs_host_error().decode(), ol)
    st.n_reads = [int(v) for v in nr]
    return [o[:int(n)] for o, n in zip(outs, ol)], st


def dedup_opts(keep=0, hash_bits=40, seed=0, reserved=(0, 0)):
    """bfq_dedup_opts (include/bfqzip_hip.h); the defaults are bfq_dedup_default_opts'.  keep: 0 keeps the first unit of every
    group of equal sequences, 1 the one with the best qualities (ties: the first); hash_bits (1..40): the bits of the sequence
    hash the units are sorted by -- small values are a test knob, the outputs do not depend on it, nor on seed; reserved must
    be 0."""
    o = _lib.DedupOpts()
    o.keep, o.hash_bits, o.seed = int(keep), int(hash_bits), int(seed)
    o.reserved[0], o.reserved[1] = (int(reserved), 0) if not hasattr(reserved, "__len__") else (int(reserved[0]), int(reserved[1]))
    return o


def _dedup_texts(texts):
    """the one or two texts of a dedup call (None: absent) as pointer and length arrays"""
    texts = [None if t is None else _u8(t) for t in list(texts) + [None] * (2 - len(texts))]
    if len(texts) != 2:
        raise ValueError("dedup: at most two texts")
    ptrs = (C.c_void_p * 2)(*[None if t is None else (t if len(t) else _EMPTY_TEXT).ctypes.data for t in texts])
    lens = (C.c_uint64 * 2)(*[0 if t is None else len(t) for t in texts])
    return texts, ptrs, lens


def _dedup_bufs(bufs):
    return (C.c_void_p * 2)(*[b.ctypes.data if len(b) else None for b in bufs]), (C.c_uint64 * 2)(*[len(b) for b in bufs])


def _dedup_call(fn, err, texts, outs, dups, opts):
    """the memory forms' shared body: fn(ptrs, lens, opts, outs, caps, dups, caps, out_len, dup_len, stats) -> rc; err(): the
    message.  dups: False (not written), True (sized by the call) or two uint8 arrays."""
    keep, ptrs, lens = _dedup_texts(texts)
    O, st, ol, dl = dedup_opts(**opts), _lib.DedupStats(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    optrs, ocaps = _dedup_bufs(outs)
    dptrs, dcaps = _dedup_bufs(dups) if dups is not False else (None, None)
    rc = fn(ptrs, lens, C.byref(O), optrs, ocaps, dptrs, dcaps, ol, dl, C.byref(st))
    if rc != 0:
        _pairs_raise(rc, err(), list(ol) + list(dl))
    return [o[:int(n)] for o, n in zip(outs, ol)], None if dups is False else [d[:int(n)] for d, n in zip(dups, dl)], st


def fastq_dedup_host(texts, outs=None, dups=False, **opts):
    """(kept[2], removed[2] or None, stats) of the FASTQ texts (texts[0]: the reads or the first mates; texts[1]: the second
    mates, None: single-end) with exact duplicates removed by the host form (bfq_fastq_dedup_host: the steps of
    csrc/bfq_dedup.h by one thread, no GPU): the statement of the algorithm -- Engine.fastq_dedup gives the same bytes, stats
    and messages.  opts: dedup_opts().  `outs`: two uint8 arrays to fill; `dups`: False (the removed records are counted and
    not written), True, or two uint8 arrays; a buffer that is too small raises BfqError with .needed = the four lengths,
    nothing written."""
    L = _lib.lib()
    err = lambda: L.bfq_dedup_host_error().decode()
    if outs is None or dups is True:
        keep, ptrs, lens = _dedup_texts(texts)
        O, st, ol, dl = dedup_opts(**opts), _lib.DedupStats(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        rc = L.bfq_fastq_dedup_host(ptrs, lens, C.byref(O), None, None, None, None, ol, dl, C.byref(st))
        if rc != 0:
            _pairs_raise(rc, err(), list(ol) + list(dl))
        outs = [np.empty(int(v), np.uint8) for v in ol] if outs is None else outs
        dups = [np.empty(int(v), np.uint8) for v in dl] if dups is True else dups
    return _dedup_call(L.bfq_fastq_dedup_host, err, texts, outs, dups, opts)


def text_len(a):
    """The length a FASTQ source has as text: its own, or the raw length of a BGZF source (what output buffers are sized from)."""
    a = _u8(a)
    if len(a) >= 2 and a[0] == 0x1F and a[1] == 0x8B:
        raw = C.c_uint64(0)
        if _lib.lib().bfq_bgzf_index(_ptr(a), len(a), None, 0, None, C.byref(raw), None) == 0:
            return int(raw.value) + 1                              # (+ the newline a part may lack)
    return len(a)


class HostText:
    """Host-side text helpers of libbfqhip.so (no GPU involved)."""
    bgzf_probe = staticmethod(bgzf_probe)
    bgzf_index = staticmethod(bgzf_index)
    bgzf_deflate_bound = staticmethod(bgzf_deflate_bound)
    bgzf_deflate_model = staticmethod(bgzf_deflate_model)
    gzip_probe = staticmethod(gzip_probe)
    gzip_inflate_host = staticmethod(gzip_inflate_host)
    bam_probe = staticmethod(bam_probe)
    bam_to_fastq_host = staticmethod(bam_to_fastq_host)
    bam_patch_host = staticmethod(bam_patch_host)
    fastq_to_bam_host = staticmethod(fastq_to_bam_host)
    fastq_deinterleave_host = staticmethod(fastq_deinterleave_host)
    fastq_interleave_host = staticmethod(fastq_interleave_host)
    fastq_repair_host = staticmethod(fastq_repair_host)
    fastq_dedup_host = staticmethod(fastq_dedup_host)
    FileRange = FileRange
    text_line_counts = staticmethod(text_line_counts)
    text_nth_newline = staticmethod(text_nth_newline)
    file_put = staticmethod(file_put)
    restore_groups = staticmethod(restore_groups)
    edits_info = staticmethod(lambda z: edits_info(z))
    fastq_edits_host = staticmethod(lambda a, b, out=None: fastq_edits_host(a, b, out))
    fastq_unedit_host = staticmethod(lambda t, z, out=None: fastq_unedit_host(t, z, out))


class Engine:
    """One GPU context (one stream, one device workspace). Not thread-safe."""
    host = HostText

    def __init__(self, device=0, **params):
        self.L = _lib.lib()
        self.params = make_params(**params)
        self.h = self.L.bfq_create(device, C.byref(self.params))
        if not self.h:
            raise BfqError(-2, self.L.bfq_create_error().decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.bfq_destroy(self.h)
            self.h = None

    __del__ = close

    def set_params(self, **params):
        self.params = make_params(**params)
        self._ck(self.L.bfq_set_params(self.h, C.byref(self.params)))

    def _ck(self, rc):
        if rc != 0:
            raise BfqError(rc, self.L.bfq_last_error(self.h).decode())

    # ---- step 1
    def build_ebwt(self, bases, quals, roff, term_out=ord("#")):
        bases = np.ascontiguousarray(bases, np.uint8); quals = np.ascontiguousarray(quals, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        N = len(roff) - 1
        n = int(roff[-1]) + N
        bwt = np.empty(n, np.uint8); qs = np.empty(n, np.uint8); lcp = np.empty(n, np.uint16)
        self._ck(self.L.bfq_build_ebwt(self.h, _ptr(bases), _ptr(quals), _ptr(roff), N, term_out,
                                       _ptr(bwt), _ptr(qs), _ptr(lcp)))
        return bwt, qs, lcp

    # ---- steps 2-4
    def smooth_invert(self, bwt, qs, lcp=None, out=None):
        """out: optional (bases u8[n-N], quals u8[n-N], roff u64[N+1]) arrays to fill (e.g. pinned)."""
        bwt = np.ascontiguousarray(bwt, np.uint8); qs = np.ascontiguousarray(qs, np.uint8)
        n = len(bwt)
        N = C.c_uint64(0)
        self.L.bfq_count_reads(_ptr(bwt), n, self.params.term & 0xFF, C.byref(N))
        N = N.value
        lcp_bytes = 0
        if lcp is not None:
            lcp = np.ascontiguousarray(lcp)
            lcp_bytes = lcp.dtype.itemsize
        if out is not None:
            ob, oq, oroff = out
            assert len(ob) >= n - N and len(oq) >= n - N and len(oroff) >= N + 1 and oroff.dtype == np.uint64
        else:
            ob = np.empty(max(n - N, 1), np.uint8); oq = np.empty(max(n - N, 1), np.uint8)
            oroff = np.empty(N + 1, np.uint64)
        st = _lib.Stats()
        self._ck(self.L.bfq_smooth_invert(self.h, _ptr(bwt), _ptr(qs), _ptr(lcp), lcp_bytes, n,
                                          _ptr(ob), _ptr(oq), _ptr(oroff), C.byref(st)))
        return ob[:n - N], oq[:n - N], oroff[:N + 1], st.as_dict()

    # ---- fused
    def run_reads(self, bases, quals, roff):
        bases = np.ascontiguousarray(bases, np.uint8); quals = np.ascontiguousarray(quals, np.uint8)
        roff = np.ascontiguousarray(roff, np.uint64)
        N = len(roff) - 1
        ob = np.empty(max(len(bases), 1), np.uint8); oq = np.empty(max(len(bases), 1), np.uint8)
        st = _lib.Stats()
        self._ck(self.L.bfq_run_reads(self.h, _ptr(bases), _ptr(quals), _ptr(roff), N, _ptr(ob), _ptr(oq),
                                      C.byref(st)))
        return ob[:len(bases)], oq[:len(bases)], st.as_dict()

    def run_reads_device(self, d_bases, d_quals, d_roff, N, total, d_out_bases, d_out_quals):
        """All arguments are raw device pointers (ints), e.g. torch tensor .data_ptr()."""
        st = _lib.Stats()
        self._ck(self.L.bfq_run_reads_device(self.h, d_bases, d_quals, d_roff, N, total, d_out_bases,
                                             d_out_quals, C.byref(st)))
        return st.as_dict()

    # ---- FASTQ text in / out, parsed and formatted on the GPU
    def fastq_build_ebwt(self, text, term_out=ord("#"), want_lcp=True, out=None):
        """gsufsort / eGap on the bytes of a FASTQ file -> (bwt, qs, lcp16).  out: optional (bwt, qs, lcp16 or None) arrays."""
        buf = _u8(text)
        if out is not None:
            bwt, qs, lcp = out
            cap = min(len(bwt), len(qs), len(lcp) if lcp is not None else len(bwt))
            want_lcp = lcp is not None
        else:
            cap = text_len(buf) // 2 + 1
            bwt = np.empty(cap, np.uint8); qs = np.empty(cap, np.uint8)
            lcp = np.empty(cap, np.uint16) if want_lcp else None
        n = C.c_uint64(0); N = C.c_uint64(0)
        self._ck(self.L.bfq_fastq_build_ebwt(self.h, _ptr(buf), len(buf), term_out, _ptr(bwt), _ptr(qs), _ptr(lcp), cap,
                                             C.byref(n), C.byref(N)))
        return bwt[:n.value], qs[:n.value], (lcp[:n.value] if want_lcp else None)

    def fastq_run(self, text, keep_headers=False):
        """The whole path on the bytes of a FASTQ file -> (smoothed FASTQ bytes, stats)."""
        buf = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        out = np.empty(text_len(buf) + 16, np.uint8)
        ol = C.c_uint64(0)
        st = _lib.Stats()
        self._ck(self.L.bfq_fastq_run(self.h, _ptr(buf), len(buf), 1 if keep_headers else 0, _ptr(out), len(out),
                                      C.byref(ol), C.byref(st)))
        return out[:ol.value].tobytes(), st.as_dict()

    def fastq_run_streams(self, text, want_headers=True):
        """The whole path with the result as the streams of BFQzip.py --m2/--m3 (BFQzip.py:19-21,192-251):
        (OUT.fq.dna bytes, OUT.fq.qs bytes, OUT.h bytes or None, stats)."""
        buf = np.frombuffer(text, np.uint8) if not isinstance(text, np.ndarray) else np.ascontiguousarray(text, np.uint8)
        cap = text_len(buf) + 16
        dna = np.empty(cap, np.uint8); qs = np.empty(cap, np.uint8)
        hdr = np.empty(cap, np.uint8) if want_headers else None
        sl = C.c_uint64(0); hl = C.c_uint64(0)
        st = _lib.Stats()
        self._ck(self.L.bfq_fastq_run_streams(self.h, _ptr(buf), len(buf), _ptr(dna), _ptr(qs), cap, C.byref(sl),
                                              _ptr(hdr) if want_headers else None, cap, C.byref(hl), C.byref(st)))
        return (dna[:sl.value].tobytes(), qs[:sl.value].tobytes(),
                hdr[:hl.value].tobytes() if want_headers else None, st.as_dict())

    def fastq_job(self, parts, keep_headers=False, fastq=True, streams=False, hdr=False, out=None, compress=False, names=False, quals=False,
                  edits=False):
        """One block of BFQzip_parallel.py in one call (bfq_fastq_run_job): `parts` = 1..4 byte ranges (bytes,
        uint8 arrays, memmap slices) processed as one collection; outputs as asked: the FASTQ text, the --m2
        streams (dna, qs), the --m3 header stream.  `out` may give reusable output arrays (e.g. PinnedBuffer.array)
        under the keys 'fastq', 'dna', 'qs', 'hdr'.  compress=True: the streams come back as BFQRANS2 containers
        (steps 1-5 of the reference in one call; stream_decompress gives the raw stream).  names=True (with compress): the
        header stream leaves as names_compress writes it (the tokenised BFQNAME1 container where that is shorter).  quals=True
        (with compress 1 or 3): the quality stream leaves as quals_compress writes it (BFQQUAL1 where that is shorter).
        edits=True (not with compress 2 or 3): .edits is the BFQEDIT1 member of the run's base edits -- the input's byte at
        every base the run changed (fastq_unedit / fastq_restore(edits=) write them back); out['edits'] may give its buffer
        (default: input length / 8 + 4096 bytes; too small: BfqError whose .needed is the size that suffices)."""
        arrs = [_u8(p) for p in parts]
        np_ = len(arrs)
        tp = (_lib.TextPart * np_)()
        for i, a in enumerate(arrs):
            tp[i].data = a.ctypes.data if len(a) else None
            tp[i].len = len(a)
        inlen = sum(text_len(a) for a in arrs)                  # (a BGZF part: its raw length)
        out = out or {}

        def buf(key, want, size):
            if not want:
                return None
            b = out.get(key)                      # a caller's buffer is used as it is (too small: BFQ_E_ARG)
            return b if b is not None else np.empty(size, np.uint8)
        J = _lib.FastqJob()
        J.parts = tp; J.nparts = np_; J.keep_headers = 1 if keep_headers else 0
        J.compress_streams = int(compress)                     # 0 raw, 1 containers of the streams, 2 eBWT-domain containers
        J.name_codec = 1 if names else 0
        J.qual_codec = 1 if quals else 0
        bf = buf("fastq", fastq, inlen + 5 * np_ + 16)
        zcap = (2 * int(self.L.bfq_stream_bound(inlen)) + 64) if compress else 0      # a tiny stream's container is larger than the stream
        bd, bq = buf("dna", streams, max(inlen + 16, zcap)), buf("qs", streams, max(inlen + 16, zcap))
        bh = buf("hdr", hdr, max(inlen + 16, zcap))
        be = buf("edits", edits, inlen // 8 + 4096)
        JE = _lib.JobEdits()
        if be is not None:
            JE.out_edits = be.ctypes.data; JE.cap_edits = len(be)
        if bf is not None:
            J.out_fastq = bf.ctypes.data; J.cap_fastq = len(bf)
        if bd is not None:
            J.out_dna = bd.ctypes.data; J.out_qs = bq.ctypes.data; J.cap_stream = min(len(bd), len(bq))
        if bh is not None:
            J.out_hdr = bh.ctypes.data; J.cap_hdr = len(bh)
        st = _lib.Stats()
        rc = (self.L.bfq_fastq_run_job_edits(self.h, C.byref(J), C.byref(JE), C.byref(st)) if be is not None else
              self.L.bfq_fastq_run_job(self.h, C.byref(J), C.byref(st)))
        if rc:
            e = BfqError(rc, self.L.bfq_last_error(self.h).decode())
            e.needed = int(JE.edits_bytes)                         # (cap_edits too small: the size that suffices)
            raise e
        r = JobResult()
        r.edits = be[:JE.edits_bytes] if be is not None else None
        r.fastq = bf[:J.fastq_len] if bf is not None else None
        r.dna = bd[:J.dna_bytes] if bd is not None else None
        r.qs = bq[:J.qs_bytes] if bq is not None else None
        r.hdr = bh[:J.hdr_bytes] if bh is not None else None
        r.n_reads, r.total_bases = int(J.n_reads), int(J.total_bases)
        r.part_reads = [int(J.part_reads[i]) for i in range(np_ + 1)]
        r.part_fastq_off = [int(J.part_fastq_off[i]) for i in range(np_ + 1)]
        r.part_stream_off = [int(J.part_stream_off[i]) for i in range(np_ + 1)]
        r.part_hdr_off = [int(J.part_hdr_off[i]) for i in range(np_ + 1)]
        r.stats = st.as_dict()
        return r

    # ---- global mode (one collection over several GPUs, unsharded result): the per-GPU pieces; tensors are torch
    #      uint8 tensors on this engine's device (bfqzip_amd/parallel.py run_global drives them)
    tensor_device = "cuda"

    def glob_begin(self, parts):
        arrs = [_u8(p) for p in parts]
        tp = (_lib.TextPart * max(len(arrs), 1))()
        for i, a in enumerate(arrs):
            tp[i].data = a.ctypes.data if len(a) else None
            tp[i].len = len(a)
        N = (C.c_uint64 * len(arrs))(); T = (C.c_uint64 * len(arrs))()
        self._ck(self.L.bfq_glob_begin(self.h, tp, len(arrs), N, T))
        return [int(x) for x in N], [int(x) for x in T]                  # reads / bases of every part

    def glob_local_text(self, t8, q8):
        self._ck(self.L.bfq_glob_local_text(self.h, t8.data_ptr(), q8.data_ptr()))

    def glob_pile_counts(self, t8, n):
        cnt = np.zeros(36, np.uint64)
        self._ck(self.L.bfq_glob_pile_counts(self.h, t8.data_ptr() if n else None, n, _ptr(cnt)))
        return cnt.reshape(6, 6)

    def glob_init_out(self, t8, q8, n, sym, qual):
        self._ck(self.L.bfq_glob_init_out(self.h, t8.data_ptr(), q8.data_ptr(), n, sym.data_ptr(), qual.data_ptr()))

    def glob_run_pile(self, t8, q8, n, s, s2, sym, qual):
        st = _lib.Stats()
        self._ck(self.L.bfq_glob_run_pile(self.h, t8.data_ptr(), q8.data_ptr(), n, s, s2, sym.data_ptr(), qual.data_ptr(), C.byref(st)))
        return st.as_dict()

    def glob_finish(self, dna, qs, keep_headers=False, fastq=True, streams=False, hdr=False, text_len=0, nparts=1, out=None):
        """dna / qs: this block's line streams (torch uint8, device).  Returns a JobResult like fastq_job.  `out`: reusable
        output arrays under 'fastq', 'dna', 'qs', 'hdr' (e.g. PinnedBuffer.array: direct DMA), used when large enough."""
        J = _lib.FastqJob()
        J.nparts = 0; J.keep_headers = 1 if keep_headers else 0
        sl = int(dna.numel())
        out = out or {}

        def buf(key, want, need, slack):
            if not want:
                return None
            b = out.get(key)                     # a caller's buffer of the exact size will do (e.g. a mapped file range)
            return b if (b is not None and len(b) >= need) else np.empty(need + slack, np.uint8)
        bf = buf("fastq", fastq, text_len, 32)
        bd = buf("dna", streams, sl, 16)
        bq = buf("qs", streams, sl, 16)
        bh = buf("hdr", hdr, text_len, 16)
        if bf is not None:
            J.out_fastq = bf.ctypes.data; J.cap_fastq = len(bf)
        if bd is not None:
            J.out_dna = bd.ctypes.data; J.out_qs = bq.ctypes.data; J.cap_stream = len(bd)
        if bh is not None:
            J.out_hdr = bh.ctypes.data; J.cap_hdr = len(bh)
        self._ck(self.L.bfq_glob_finish(self.h, dna.data_ptr() if sl else None, qs.data_ptr() if sl else None, C.byref(J)))
        r = JobResult()
        r.edits = None
        r.fastq = bf[:J.fastq_len] if bf is not None else None
        r.dna = bd[:J.dna_bytes] if bd is not None else None
        r.qs = bq[:J.qs_bytes] if bq is not None else None
        r.hdr = bh[:J.hdr_bytes] if bh is not None else None
        r.n_reads, r.total_bases = int(J.n_reads), int(J.total_bases)
        r.part_reads = [int(J.part_reads[i]) for i in range(nparts + 1)]
        r.part_fastq_off = [int(J.part_fastq_off[i]) for i in range(nparts + 1)]
        r.part_stream_off = [int(J.part_stream_off[i]) for i in range(nparts + 1)]
        r.part_hdr_off = [int(J.part_hdr_off[i]) for i in range(nparts + 1)]
        r.stats = {}
        return r

    def smooth_invert_fastq(self, bwt, qs, lcp=None, headers=None):
        """bfq_int / bfq_ext writing the FASTQ text; headers = bytes of the -H file or None."""
        bwt = np.ascontiguousarray(bwt, np.uint8); qs = np.ascontiguousarray(qs, np.uint8)
        n = len(bwt)
        N = C.c_uint64(0)
        self.L.bfq_count_reads(_ptr(bwt), n, self.params.term & 0xFF, C.byref(N))
        N = N.value
        lcp_bytes = 0
        if lcp is not None:
            lcp = np.ascontiguousarray(lcp); lcp_bytes = lcp.dtype.itemsize
        hb = np.frombuffer(headers, np.uint8) if headers is not None else None
        cap = int(self.L.bfq_fastq_out_bound(n - N, N, len(hb) if hb is not None else 0)) + 16
        out = np.empty(cap, np.uint8)
        ol = C.c_uint64(0)
        st = _lib.Stats()
        self._ck(self.L.bfq_smooth_invert_fastq(self.h, _ptr(bwt), _ptr(qs), _ptr(lcp), lcp_bytes, n, _ptr(hb),
                                                len(hb) if hb is not None else 0, _ptr(out), cap, C.byref(ol), C.byref(st)))
        return out[:ol.value].tobytes(), st.as_dict()

    def fetch_ebwt(self, n, out=None):
        bwt, qs, lcp = out if out is not None else (np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint16))
        self._ck(self.L.bfq_fetch_ebwt(self.h, _ptr(bwt), _ptr(qs), _ptr(lcp)))
        return bwt, qs, lcp

    # ---- synthetic reads
    def synth_device(self, spec, d_bases, d_quals, d_roff):
        self._ck(self.L.bfq_synth_device(self.h, C.byref(spec), d_bases, d_quals, d_roff))

    def synth_fastq(self, spec, out):
        """The synthetic reads of `spec` as FASTQ text (headers "@SYN.<n>") into the uint8 array `out`; returns the length."""
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_synth_fastq(self.h, C.byref(spec), _ptr(out), len(out), C.byref(ol)))
        return int(ol.value)

    # ---- stream codec (step 5 of the reference: BFQzip.py:253-275)
    def stream_compress(self, data, out=None):
        """BFQRANS2 container of the bytes `data` (uint8 array); returns a uint8 array (a view of `out` when given)."""
        data = _u8(data)
        cap = int(self.L.bfq_stream_bound(len(data)))
        if out is None:
            out = np.empty(cap, np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_stream_compress(self.h, _ptr(data), len(data), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def names_compress(self, data, always=False, out=None):
        """Read names (lines) as the tokenised BFQNAME1 container when the stream is eligible (not empty, a final newline, no
        line above 65 535 bytes) and the container is shorter than stream_compress's; else exactly what stream_compress
        gives.  always=True: BFQNAME1 whenever the stream is eligible.  stream_decompress and fastq_restore take either."""
        data = _u8(data)
        if out is None:
            out = np.empty(int(self.L.bfq_stream_bound(len(data))), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_names_compress(self.h, _ptr(data), len(data), 1 if always else 0, _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    @staticmethod
    def _quals_flags(always, rung):
        if rung is not None and rung not in (0, 1, 2, 3):
            raise ValueError("rung is None or 0..3")
        return (1 if always else 0) | (0 if rung is None else 2 | (int(rung) << 8))

    def quals_compress(self, data, always=False, rung=None, out=None):
        """Quality lines in read order as the BFQQUAL1 container (values coded by their place in the read) when the stream is
        eligible (a final newline, at least one value, no line above 65 535 bytes, at most 64 distinct values) and the
        container is shorter than stream_compress's; else exactly what stream_compress gives.  always=True: BFQQUAL1 whenever
        the stream is eligible.  rung=0..3 forces the model's rung (tests, diagnostics).  stream_decompress and fastq_restore
        take either."""
        data = _u8(data)
        if out is None:
            out = np.empty(int(self.L.bfq_stream_bound(len(data))), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_quals_compress(self.h, _ptr(data), len(data), self._quals_flags(always, rung), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def stream_decompress(self, blob, out=None):
        """The raw bytes of a container of the stream codec (BFQRANS2 / BFQDNAC1 / BFQLINE1 / BFQNAME1 / BFQQUAL1; several back to back)."""
        blob = _u8(blob)
        n = int(self.L.bfq_stream_raw_len(_ptr(blob), len(blob)))
        if n < 0:
            raise BfqError(-1, "not a BFQRANS2 / BFQDNAC1 / BFQLINE1 / BFQNAME1 / BFQQUAL1 stream (or a damaged one)")
        if out is None:
            out = np.empty(max(n, 1), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_stream_decompress(self.h, _ptr(blob), len(blob), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def bgzf_inflate(self, blob, out=None):
        """The text of a bgzip-compressed (BGZF) file, inflated on the GPU (bfq_bgzf_inflate) as a uint8 array.  `out`: a uint8
        array to fill (e.g. PinnedBuffer.array) of at least the raw length (HostText.bgzf_index); the result is a view of it.
        A damaged file raises BfqError (BFQ_E_ARG: "damaged BGZF input: member <i> at byte <off>: <reason>"); plain gzip is
        refused by name."""
        blob = _u8(blob)
        if out is None:
            raw, n = C.c_uint64(0), C.c_uint64(0)
            self.L.bfq_bgzf_index(_ptr(blob), len(blob), None, 0, C.byref(n), C.byref(raw), None)   # (a refused header: the call below words it)
            out = np.empty(max(int(raw.value), 1), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_bgzf_inflate(self.h, _ptr(blob), len(blob), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def bgzf_inflate_device(self, blob, d_out, cap):
        """bfq_bgzf_inflate_device: the text at the device address d_out (cap bytes); returns its length."""
        blob = _u8(blob)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_bgzf_inflate_device(self.h, _ptr(blob), len(blob), C.c_void_p(d_out), cap, C.byref(ol)))
        return int(ol.value)

    def bgzf_inflate_files(self, src, dst=None):
        """bfq_bgzf_inflate_fd on named files; dst None: inflate and verify only.  Returns the length of the text."""
        import os
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if dst is not None else -1)
            ol = C.c_uint64(0)
            self._ck(self.L.bfq_bgzf_inflate_fd(self.h, fds[0], os.fstat(fds[0]).st_size, fds[1], C.byref(ol)))
            return int(ol.value)
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- plain gzip: one deflate stream per member, inflated side by side (bfq_gzip_*, csrc/bfq_gzip.h)
    def _gzip_ck(self, rc, ol):
        if rc != 0:
            _gzip_raise(rc, self.L.bfq_last_error(self.h).decode(), ol.value)

    def gzip_measure(self, blob, chunk=0):
        """bfq_gzip_measure: (raw length, members, stats) of a gzip file from the candidate search and the counting pass alone."""
        blob = _u8(blob)
        raw, n, st = C.c_uint64(0), C.c_uint64(0), _lib.GzipStats()
        self._ck(self.L.bfq_gzip_measure(self.h, _ptr(blob) if len(blob) else None, len(blob), int(chunk), C.byref(raw), C.byref(n), C.byref(st)))
        return int(raw.value), int(n.value), st

    def gzip_inflate(self, blob, out=None, chunk=0):
        """(text, stats) of a gzip file -- what gzip, pigz and `cat a.gz b.gz` write, BGZF included -- inflated on the GPU
        (bfq_gzip_inflate); the text is a uint8 array.  `out`: a uint8 array to fill, the text is a view of it; without one
        the file is measured first (gzip_measure).  chunk: bytes per piece, a power of two >= 512, 0 = the default.  An `out`
        below the raw length raises BfqError with .needed = that length and is left untouched; a damaged file raises BfqError
        (BFQ_E_ARG: "damaged gzip input: member <i> at byte <off>: <reason>")."""
        blob = _u8(blob)
        if out is None:
            out = np.empty(max(self.gzip_measure(blob, chunk)[0], 1), np.uint8)
        ol, st = C.c_uint64(0), _lib.GzipStats()
        self._gzip_ck(self.L.bfq_gzip_inflate(self.h, _ptr(blob) if len(blob) else None, len(blob), int(chunk), _ptr(out), len(out), C.byref(ol),
                                              C.byref(st)), ol)
        return out[:int(ol.value)], st

    def gzip_inflate_device(self, blob, d_out, cap, chunk=0):
        """bfq_gzip_inflate_device: the text at the device address d_out (cap bytes); returns (its length, stats)."""
        blob = _u8(blob)
        ol, st = C.c_uint64(0), _lib.GzipStats()
        self._gzip_ck(self.L.bfq_gzip_inflate_device(self.h, _ptr(blob) if len(blob) else None, len(blob), int(chunk), C.c_void_p(d_out), cap,
                                                     C.byref(ol), C.byref(st)), ol)
        return int(ol.value), st

    def gzip_inflate_files(self, src, dst=None, chunk=0):
        """bfq_gzip_inflate_fd on named files; dst None: inflate and verify only.  Returns (the length of the text, stats)."""
        import os
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if dst is not None else -1)
            ol, st = C.c_uint64(0), _lib.GzipStats()
            self._gzip_ck(self.L.bfq_gzip_inflate_fd(self.h, fds[0], os.fstat(fds[0]).st_size, int(chunk), fds[1], C.byref(ol), C.byref(st)), ol)
            return int(ol.value), st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- BAM records to FASTQ text (bfq_bam_*, csrc/bfq_bam.h)
    def _bam_ck(self, rc, ol):
        if rc != 0:
            _bam_raise(rc, self.L.bfq_last_error(self.h).decode(), ol)

    def bam_measure(self, blob, **opts):
        """bfq_bam_measure: (the three text lengths, the three read counts, stats) of a BAM file; nothing is written."""
        blob = _u8(blob)
        O, st, ol, nr = bam_opts(**opts), _lib.BamStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        st.tags = getattr(O, "tag_stats", None)
        self._bam_ck(self.L.bfq_bam_measure(self.h, _ptr(blob) if len(blob) else None, len(blob), C.byref(O), ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def bam_to_fastq(self, blob, outs=None, **opts):
        """(texts[3], stats) of a BAM file -- BGZF as samtools, GATK and DRAGEN write it, or the inflated stream itself --
        converted on the GPU (bfq_bam_to_fastq); the texts are uint8 arrays: output 0, and with split=1 READ1-only records in
        1 and READ2-only records in 2.  opts: bam_opts() (exclude_flags, mate_suffix, default_qual, split, paired_check,
        piece).  `outs`: three uint8 arrays to fill; without them the file is measured first.  A buffer below its text raises
        BfqError with .needed = the three lengths and nothing is written; a damaged or unpaired file raises BfqError
        ("damaged BAM input: record <i> at byte <off>: <reason>", "unpaired BAM input: pair <k>: ...")."""
        blob = _u8(blob)
        if outs is None:
            outs = [np.empty(v, np.uint8) for v in self.bam_measure(blob, **dict(opts, paired_check=0))[0]]
        O, st, ol, nr = bam_opts(**opts), _lib.BamStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        st.tags = getattr(O, "tag_stats", None)
        ptrs, caps = _bam_outs(outs)
        self._bam_ck(self.L.bfq_bam_to_fastq(self.h, _ptr(blob) if len(blob) else None, len(blob), C.byref(O), ptrs, caps, ol, nr, C.byref(st)), ol)
        return [o[:int(n)] for o, n in zip(outs, ol)], st

    def bam_to_fastq_device(self, blob, d_outs, caps, **opts):
        """bfq_bam_to_fastq_device: the texts at the three device addresses d_outs (caps bytes each); returns (lengths, read counts, stats)."""
        blob = _u8(blob)
        O, st, ol, nr = bam_opts(**opts), _lib.BamStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        st.tags = getattr(O, "tag_stats", None)
        ptrs, cp = (C.c_void_p * 3)(*[int(p) if p else None for p in d_outs]), (C.c_uint64 * 3)(*[int(v) for v in caps])
        self._bam_ck(self.L.bfq_bam_to_fastq_device(self.h, _ptr(blob) if len(blob) else None, len(blob), C.byref(O), ptrs, cp, ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def bam_to_fastq_files(self, src, dsts=(None, None, None), **opts):
        """bfq_bam_to_fastq_fd on named files: dsts = the paths of outputs 0, 1, 2 (None: not written; all None: convert and
        verify only).  Returns (lengths, read counts, stats)."""
        import os
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            for d in dsts:
                fds.append(os.open(d, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if d is not None else -1)
            O, st, ol, nr = bam_opts(**opts), _lib.BamStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
            st.tags = getattr(O, "tag_stats", None)
            self._bam_ck(self.L.bfq_bam_to_fastq_fd(self.h, fds[0], os.fstat(fds[0]).st_size, C.byref(O), (C.c_int * 3)(*fds[1:4]), ol, nr, C.byref(st)), ol)
            return [int(v) for v in ol], [int(v) for v in nr], st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- FASTQ texts back into their BAM (bfq_bam_patch*, csrc/bfq_bam_patch.h)
    def bam_patch(self, blob, texts, level=1, out=None, **opts):
        """(the BAM file, stats): `blob` -- a BAM file as bam_to_fastq takes it -- with the sequence and quality lines of up
        to three FASTQ texts written back into the records they came from, patched on the GPU and compressed there
        (bfq_bam_patch); a uint8 array.  texts[k] (None: absent, its records stay) meets output k of bam_to_fastq with the same
        opts: bam_opts(), check_names=1 compares the names too.  level: as bgzf_deflate.  `out`: a uint8 array to fill; one
        below HostText.bgzf_deflate_bound(the stream's length) raises BfqError with .needed = that bound, nothing written;
        without one it is sized from the file's directory.  Refusals raise BfqError (BFQ_E_ARG: "BAM patch: text <k> ...", "FASTQ: ...",
        "damaged BAM input: ...").  An index of the input does not fit the result; MD / NM tags go stale where a base changed."""
        blob = _u8(blob)
        keep, ptrs, lens = _bam_texts(texts)
        if out is None:
            out = np.empty(bgzf_deflate_bound(text_len(blob)), np.uint8)    # (the directory gives the stream's length)
        O, st, ol = bam_opts(**opts), _lib.BamPatchStats(), C.c_uint64(0)
        rc = self.L.bfq_bam_patch(self.h, _ptr(blob) if len(blob) else None, len(blob), C.byref(O), ptrs, lens, int(level), _ptr(out) if len(out) else None,
                                  len(out), C.byref(ol), C.byref(st))
        if rc != 0:
            _bam_patch_raise(rc, self.L.bfq_last_error(self.h).decode(), ol.value)
        return out[:int(ol.value)], st

    def bam_patch_device(self, blob, d_texts, text_lens, d_out, cap, **opts):
        """bfq_bam_patch_device: the texts at the device addresses d_texts (None / 0: absent), the patched INFLATED stream at
        the device address d_out (cap bytes), not compressed; returns (its length, stats).  A cap below that length raises
        BfqError with .needed = the length, nothing written."""
        blob = _u8(blob)
        ptrs = (C.c_void_p * 3)(*[int(p) if p else None for p in d_texts])
        lens = (C.c_uint64 * 3)(*[int(v) for v in text_lens])
        O, st, rl = bam_opts(**opts), _lib.BamPatchStats(), C.c_uint64(0)
        rc = self.L.bfq_bam_patch_device(self.h, _ptr(blob) if len(blob) else None, len(blob), C.byref(O), ptrs, lens, C.c_void_p(d_out), int(cap), C.byref(rl),
                                         C.byref(st))
        if rc != 0:
            _bam_patch_raise(rc, self.L.bfq_last_error(self.h).decode(), rl.value)
        return int(rl.value), st

    def bam_patch_files(self, src, texts, dst, level=1, **opts):
        """bfq_bam_patch_fd on named files: the BAM file src with the FASTQ files texts[k] (None: absent) in it, written to dst
        (left empty on a refusal).  Returns (the length of dst, stats)."""
        import os
        texts = list(texts) + [None] * (3 - len(texts))
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            for t in texts[:3]:
                fds.append(os.open(t, os.O_RDONLY) if t is not None else -1)
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            O, st, ol = bam_opts(**opts), _lib.BamPatchStats(), C.c_uint64(0)
            rc = self.L.bfq_bam_patch_fd(self.h, fds[0], os.fstat(fds[0]).st_size, C.byref(O), (C.c_int * 3)(*fds[1:4]), int(level), fds[4], C.byref(ol),
                                         C.byref(st))
            if rc != 0:
                _bam_patch_raise(rc, self.L.bfq_last_error(self.h).decode(), ol.value)
            return int(ol.value), st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- FASTQ texts as an unaligned BAM (bfq_fastq_to_bam*, csrc/bfq_ubam.h)
    def fastq_to_bam_measure(self, texts, **opts):
        """bfq_fastq_to_bam_measure: (the exact length of the inflated stream, the three read counts, stats without
        unknown_bases) of up to three host texts; nothing is written."""
        keep, ptrs, lens = _bam_texts(texts)
        (O, held), st, rl, nr = ubam_opts(**opts), _lib.UbamStats(), C.c_uint64(0), (C.c_uint64 * 3)()
        st.tags = getattr(O, "tag_stats", None)
        rc = self.L.bfq_fastq_to_bam_measure(self.h, ptrs, lens, C.byref(O), C.byref(rl), nr, C.byref(st))
        if rc != 0:
            _ubam_raise(rc, self.L.bfq_last_error(self.h).decode(), 0)
        return int(rl.value), [int(v) for v in nr], st

    def fastq_to_bam(self, texts, out=None, **opts):
        """(the BAM file, stats): up to three FASTQ texts as an unaligned BAM, the records made on the GPU and compressed there
        (bfq_fastq_to_bam); a uint8 array.  texts[0]: unpaired reads (flag 4); texts[1] / texts[2]: the mates of a paired run
        (flags 77 / 141, interleaved, in front of the reads of texts[0]); None: absent.  opts: ubam_opts() (mate_suffix,
        paired_check, level, header_text, rg_id).  `out`: a uint8 array to fill; one below
        HostText.bgzf_deflate_bound(the stream's length) raises BfqError with .needed = that bound, nothing written; without
        one it is sized by fastq_to_bam_measure.  Refusals raise BfqError ("FASTQ to BAM: text <k> ...", "FASTQ: ...")."""
        keep, ptrs, lens = _bam_texts(texts)
        if out is None:
            out = np.empty(bgzf_deflate_bound(self.fastq_to_bam_measure(texts, **opts)[0]), np.uint8)
        (O, held), st, ol = ubam_opts(**opts), _lib.UbamStats(), C.c_uint64(0)
        st.tags = getattr(O, "tag_stats", None)
        rc = self.L.bfq_fastq_to_bam(self.h, ptrs, lens, C.byref(O), _ptr(out) if len(out) else None, len(out), C.byref(ol), C.byref(st))
        if rc != 0:
            _ubam_raise(rc, self.L.bfq_last_error(self.h).decode(), ol.value)
        return out[:int(ol.value)], st

    def fastq_to_bam_device(self, d_texts, text_lens, d_out, cap, **opts):
        """bfq_fastq_to_bam_device: the texts at the device addresses d_texts (None / 0: absent), the INFLATED stream at the
        device address d_out (cap bytes), not compressed; returns (its length, stats).  A cap below that length raises
        BfqError with .needed = the length, nothing written."""
        ptrs = (C.c_void_p * 3)(*[int(p) if p else None for p in d_texts])
        lens = (C.c_uint64 * 3)(*[int(v) for v in text_lens])
        (O, held), st, rl = ubam_opts(**opts), _lib.UbamStats(), C.c_uint64(0)
        st.tags = getattr(O, "tag_stats", None)
        rc = self.L.bfq_fastq_to_bam_device(self.h, ptrs, lens, C.byref(O), C.c_void_p(d_out), int(cap), C.byref(rl), C.byref(st))
        if rc != 0:
            _ubam_raise(rc, self.L.bfq_last_error(self.h).decode(), rl.value)
        return int(rl.value), st

    def fastq_to_bam_files(self, texts, dst, **opts):
        """bfq_fastq_to_bam_fd on named files: the FASTQ files texts[k] (None: absent) as the unaligned BAM dst (left empty
        on a refusal).  Returns (the length of dst, stats)."""
        import os
        texts = list(texts) + [None] * (3 - len(texts))
        fds = []
        try:
            for t in texts[:3]:
                fds.append(os.open(t, os.O_RDONLY) if t is not None else -1)
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            (O, held), st, ol = ubam_opts(**opts), _lib.UbamStats(), C.c_uint64(0)
            st.tags = getattr(O, "tag_stats", None)
            rc = self.L.bfq_fastq_to_bam_fd(self.h, (C.c_int * 3)(*fds[0:3]), C.byref(O), fds[3], C.byref(ol), C.byref(st))
            if rc != 0:
                _ubam_raise(rc, self.L.bfq_last_error(self.h).decode(), ol.value)
            return int(ol.value), st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- interleaved paired FASTQ (bfq_fastq_deinterleave* / bfq_fastq_interleave*, csrc/bfq_pairs.h)
    def _pairs_ck(self, rc, needed):
        if rc != 0:
            _pairs_raise(rc, self.L.bfq_last_error(self.h).decode(), needed)

    def fastq_deinterleave_measure(self, text, **opts):
        """bfq_fastq_deinterleave_measure: (the three text lengths, the three read counts, stats) of an interleaved FASTQ
        text; nothing is written.  An improperly paired text raises BfqError with the library's message."""
        text = _u8(text)
        O, st, ol, nr = pairs_opts(**opts), _lib.PairsStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        self._pairs_ck(self.L.bfq_fastq_deinterleave_measure(self.h, _ptr(text) if len(text) else None, len(text), C.byref(O), ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def fastq_deinterleave(self, text, outs=None, **opts):
        """(texts[3], stats): an interleaved paired FASTQ text (plain, not compressed) split on the GPU (bfq_fastq_deinterleave)
        into the mates texts[1] and texts[2]; with orphans=1 the singletons go to texts[0].  Records move byte for byte.
        opts: pairs_opts() (check_names, mate_suffix, orphans).  `outs`: three uint8 arrays to fill; without them the text is
        measured first.  A buffer below its text raises BfqError with .needed = the three lengths and nothing is written; an
        improperly paired text raises BfqError ("interleaved FASTQ: pair <k> (records <2k> and <2k+1>): the names differ",
        "interleaved FASTQ: <N> records, an odd number").  stats.n_reads: the reads per output."""
        text = _u8(text)
        if outs is None:
            outs = [np.empty(v, np.uint8) for v in self.fastq_deinterleave_measure(text, **opts)[0]]
        O, st, ol, nr = pairs_opts(**opts), _lib.PairsStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        ptrs, caps = _bam_outs(outs)
        self._pairs_ck(self.L.bfq_fastq_deinterleave(self.h, _ptr(text) if len(text) else None, len(text), C.byref(O), ptrs, caps, ol, nr, C.byref(st)), ol)
        st.n_reads = [int(v) for v in nr]
        return [o[:int(n)] for o, n in zip(outs, ol)], st

    def fastq_deinterleave_device(self, d_text, n, d_outs, caps, **opts):
        """bfq_fastq_deinterleave_device: the text of n bytes at the device address d_text, the three texts at the device
        addresses d_outs (caps bytes each; None / 0 with cap 0: none); returns (lengths, read counts, stats)."""
        O, st, ol, nr = pairs_opts(**opts), _lib.PairsStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        ptrs, cp = (C.c_void_p * 3)(*[int(p) if p else None for p in d_outs]), (C.c_uint64 * 3)(*[int(v) for v in caps])
        self._pairs_ck(self.L.bfq_fastq_deinterleave_device(self.h, C.c_void_p(d_text), int(n), C.byref(O), ptrs, cp, ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def fastq_deinterleave_files(self, src, dsts, **opts):
        """bfq_fastq_deinterleave_fd on named files: dsts = the paths of outputs 0 (singletons), 1, 2 (None: not written).
        The outputs are left empty on a refusal.  Returns (lengths, read counts, stats)."""
        import os
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            for d in dsts:
                fds.append(os.open(d, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if d is not None else -1)
            O, st, ol, nr = pairs_opts(**opts), _lib.PairsStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
            self._pairs_ck(self.L.bfq_fastq_deinterleave_fd(self.h, fds[0], os.fstat(fds[0]).st_size, C.byref(O), (C.c_int * 3)(*fds[1:4]), ol, nr, C.byref(st)), ol)
            return [int(v) for v in ol], [int(v) for v in nr], st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    def fastq_interleave_measure(self, texts, **opts):
        """bfq_fastq_interleave_measure: (the interleaved text's length, the read counts of the three texts, stats); nothing
        is written."""
        keep, ptrs, lens = _bam_texts(texts)
        O, st, ol, nr = pairs_opts(**opts), _lib.PairsStats(), C.c_uint64(0), (C.c_uint64 * 3)()
        self._pairs_ck(self.L.bfq_fastq_interleave_measure(self.h, ptrs, lens, C.byref(O), C.byref(ol), nr, C.byref(st)), 0)
        return int(ol.value), [int(v) for v in nr], st

    def fastq_interleave(self, texts, out=None, **opts):
        """(the interleaved text, stats): the mates texts[1] and texts[2] merged on the GPU (bfq_fastq_interleave) into one
        text with the mates alternating, the reads of an optional texts[0] behind the pairs (None: absent).  opts:
        pairs_opts() (check_names, mate_suffix).  `out`: a uint8 array to fill (the sum of the texts' lengths, + 1 for each
        that lacks its final newline); one that is too small raises BfqError with .needed = the length, nothing written.
        Refusals raise BfqError ("FASTQ interleave: text 1 holds <n> reads, text 2 holds <m>", "FASTQ interleave: pair <k>:
        the names differ")."""
        keep, ptrs, lens = _bam_texts(texts)
        if out is None:
            out = np.empty(sum(len(t) + 1 for t in keep if t is not None), np.uint8)
        O, st, ol = pairs_opts(**opts), _lib.PairsStats(), C.c_uint64(0)
        self._pairs_ck(self.L.bfq_fastq_interleave(self.h, ptrs, lens, C.byref(O), _ptr(out) if len(out) else None, len(out), C.byref(ol), C.byref(st)), ol.value)
        return out[:int(ol.value)], st

    def fastq_interleave_device(self, d_texts, text_lens, d_out, cap, **opts):
        """bfq_fastq_interleave_device: the texts at the device addresses d_texts (None / 0: absent), the interleaved text at
        the device address d_out (cap bytes); returns (its length, stats)."""
        ptrs = (C.c_void_p * 3)(*[int(p) if p else None for p in d_texts])
        lens = (C.c_uint64 * 3)(*[int(v) for v in text_lens])
        O, st, ol = pairs_opts(**opts), _lib.PairsStats(), C.c_uint64(0)
        self._pairs_ck(self.L.bfq_fastq_interleave_device(self.h, ptrs, lens, C.byref(O), C.c_void_p(d_out), int(cap), C.byref(ol), C.byref(st)), ol.value)
        return int(ol.value), st

    def fastq_interleave_files(self, texts, dst, **opts):
        """bfq_fastq_interleave_fd on named files: the FASTQ files texts[k] (None: absent) as the interleaved file dst (left
        empty on a refusal).  Returns (the length of dst, stats)."""
        import os
        texts = list(texts) + [None] * (3 - len(texts))
        fds = []
        try:
            for t in texts[:3]:
                fds.append(os.open(t, os.O_RDONLY) if t is not None else -1)
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            O, st, ol = pairs_opts(**opts), _lib.PairsStats(), C.c_uint64(0)
            self._pairs_ck(self.L.bfq_fastq_interleave_fd(self.h, (C.c_int * 3)(*fds[0:3]), C.byref(O), fds[3], C.byref(ol), C.byref(st)), ol.value)
            return int(ol.value), st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- repair paired FASTQ: the mates matched by name across the texts (bfq_fastq_repair*, csrc/bfq_pairs.h)
    def fastq_repair_measure(self, texts, **opts):
        """bfq_fastq_repair_measure: (the three text lengths, the three read counts, stats) of the repair of texts (see
        fastq_repair); nothing is written."""
        keep, ptrs, lens = _bam_texts(texts)
        O, st, ol, nr = repair_opts(**opts), _lib.RepairStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        self._pairs_ck(self.L.bfq_fastq_repair_measure(self.h, ptrs, lens, C.byref(O), ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def fastq_repair(self, texts, outs=None, **opts):
        """(texts[3], stats): the mates of paired FASTQ matched by name on the GPU (bfq_fastq_repair), wherever they stand.
        texts[1] and texts[2]: mate files (each may have lost reads of its own, in any order); texts[0]: a mixed file (its
        /1 and /2 suffixes say which mate a record is; without them equal names are paired two by two); None: absent.  Result
        texts[1] and texts[2]: the mates, pair k at place k of both, in the order of the first mates in the input; texts[0]:
        the singletons in input order.  Records move byte for byte.  opts: repair_opts() (mate_suffix; hash_bits and seed
        never show in the outputs).  `outs`: three uint8 arrays to fill; without them the texts are measured first.  A
        buffer below its text raises BfqError with .needed = the three lengths and nothing is written.  More than 1024
        records of one name: BfqError ("FASTQ repair: more than 1024 records share a name or a name hash ...").
        stats.n_reads: the reads per output."""
        if outs is None:
            outs = [np.empty(v, np.uint8) for v in self.fastq_repair_measure(texts, **opts)[0]]
        keep, ptrs, lens = _bam_texts(texts)
        O, st, ol, nr = repair_opts(**opts), _lib.RepairStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        optrs, caps = _bam_outs(outs)
        self._pairs_ck(self.L.bfq_fastq_repair(self.h, ptrs, lens, C.byref(O), optrs, caps, ol, nr, C.byref(st)), ol)
        st.n_reads = [int(v) for v in nr]
        return [o[:int(n)] for o, n in zip(outs, ol)], st

    def fastq_repair_device(self, d_texts, text_lens, d_outs, caps, **opts):
        """bfq_fastq_repair_device: the texts at the device addresses d_texts (None / 0: absent), the three texts at the
        device addresses d_outs (caps bytes each; None / 0 with cap 0: none); returns (lengths, read counts, stats)."""
        ptrs = (C.c_void_p * 3)(*[int(p) if p else None for p in d_texts])
        lens = (C.c_uint64 * 3)(*[int(v) for v in text_lens])
        optrs, cp = (C.c_void_p * 3)(*[int(p) if p else None for p in d_outs]), (C.c_uint64 * 3)(*[int(v) for v in caps])
        O, st, ol, nr = repair_opts(**opts), _lib.RepairStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
        self._pairs_ck(self.L.bfq_fastq_repair_device(self.h, ptrs, lens, C.byref(O), optrs, cp, ol, nr, C.byref(st)), ol)
        return [int(v) for v in ol], [int(v) for v in nr], st

    def fastq_repair_files(self, texts, dsts, **opts):
        """bfq_fastq_repair_fd on named files: the FASTQ files texts[k] (None: absent), dsts = the paths of outputs 0
        (singletons), 1, 2 (None: not written).  The outputs are left empty on a refusal.  Returns (lengths, read counts,
        stats)."""
        import os
        texts = list(texts) + [None] * (3 - len(texts))
        fds = []
        try:
            for t in texts[:3]:
                fds.append(os.open(t, os.O_RDONLY) if t is not None else -1)
            for d in dsts:
                fds.append(os.open(d, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if d is not None else -1)
            O, st, ol, nr = repair_opts(**opts), _lib.RepairStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
            self._pairs_ck(self.L.bfq_fastq_repair_fd(self.h, (C.c_int * 3)(*fds[0:3]), C.byref(O), (C.c_int * 3)(*fds[3:6]), ol, nr, C.byref(st)), ol)
            return [int(v) for v in ol], [int(v) for v in nr], st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- exact duplicate removal: reads or pairs with equal sequences leave one unit (bfq_fastq_dedup*, csrc/bfq_dedup.h)
    def fastq_dedup_measure(self, texts, **opts):
        """bfq_fastq_dedup_measure: (the two kept lengths, the two removed lengths, stats) of the dedup of texts (see
        fastq_dedup); nothing is written."""
        keep, ptrs, lens = _dedup_texts(texts)
        O, st, ol, dl = dedup_opts(**opts), _lib.DedupStats(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        self._pairs_ck(self.L.bfq_fastq_dedup_measure(self.h, ptrs, lens, C.byref(O), ol, dl, C.byref(st)), list(ol) + list(dl))
        return [int(v) for v in ol], [int(v) for v in dl], st

    def fastq_dedup(self, texts, outs=None, dups=False, **opts):
        """(kept[2], removed[2] or None, stats): exact duplicates removed on the GPU (bfq_fastq_dedup).  texts[0]: the reads
        or the first mates; texts[1]: the second mates (None: single-end) -- the k-th records of both are one unit.  Units
        with equal sequence lines (paired: both, in order) are a group; one unit of every group is kept -- the first, or with
        keep=1 the one whose qualities sum highest --, in input order, byte for byte; the others are the removed records.
        opts: dedup_opts() (hash_bits and seed never show in the outputs).  `outs`: two uint8 arrays to fill; `dups`: False
        (counted, not written), True, or two uint8 arrays; without buffers the texts are measured first.  A buffer below its
        text raises BfqError with .needed = the four lengths and nothing is written.  stats: units, kept, removed,
        dup_groups, max_group, max_group_first and the duplication levels (level_groups / level_units)."""
        if outs is None or dups is True:
            ol, dl, _ = self.fastq_dedup_measure(texts, **opts)
            outs = [np.empty(v, np.uint8) for v in ol] if outs is None else outs
            dups = [np.empty(v, np.uint8) for v in dl] if dups is True else dups
        fn = lambda *a: self.L.bfq_fastq_dedup(self.h, *a)
        return _dedup_call(fn, lambda: self.L.bfq_last_error(self.h).decode(), texts, outs, dups, opts)

    def fastq_dedup_device(self, d_texts, text_lens, d_outs, out_caps, d_dups=None, dup_caps=None, **opts):
        """bfq_fastq_dedup_device: the texts at the device addresses d_texts (None / 0: absent), the kept texts at the device
        addresses d_outs (out_caps bytes each), the removed ones at d_dups (None: not written); returns (kept lengths,
        removed lengths, stats)."""
        two = lambda v: (C.c_void_p * 2)(*[int(p) if p else None for p in list(v) + [None] * (2 - len(v))])
        cap = lambda v: (C.c_uint64 * 2)(*[int(x) for x in list(v) + [0] * (2 - len(v))])
        O, st, ol, dl = dedup_opts(**opts), _lib.DedupStats(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
        rc = self.L.bfq_fastq_dedup_device(self.h, two(d_texts), cap(text_lens), C.byref(O), two(d_outs), cap(out_caps),
                                           None if d_dups is None else two(d_dups), None if d_dups is None else cap(dup_caps), ol, dl, C.byref(st))
        self._pairs_ck(rc, list(ol) + list(dl))
        return [int(v) for v in ol], [int(v) for v in dl], st

    def fastq_dedup_files(self, texts, outs, dups=None, **opts):
        """bfq_fastq_dedup_fd on named files: the FASTQ files texts[k] (texts[1] None: single-end), outs = the paths of the
        kept records, dups = the paths of the removed ones (None: not written).  The outputs are left empty on a refusal.
        Returns (kept lengths, removed lengths, stats)."""
        import os
        pad = lambda v: list(v or []) + [None] * (2 - len(v or []))
        fds = []
        try:
            for t in pad(texts):
                fds.append(os.open(t, os.O_RDONLY) if t is not None else -1)
            for d in pad(outs) + pad(dups):
                fds.append(os.open(d, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if d is not None else -1)
            O, st, ol, dl = dedup_opts(**opts), _lib.DedupStats(), (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
            rc = self.L.bfq_fastq_dedup_fd(self.h, (C.c_int * 2)(*fds[0:2]), C.byref(O), (C.c_int * 2)(*fds[2:4]),
                                           (C.c_int * 2)(*fds[4:6]) if dups else None, ol, dl, C.byref(st))
            self._pairs_ck(rc, list(ol) + list(dl))
            return [int(v) for v in ol], [int(v) for v in dl], st
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    def bgzf_deflate(self, text, level=1, out=None):
        """The BGZF form (.fq.gz as bgzip writes it: members of 65 280 bytes, the EOF member) of a text, deflated on the GPU
        (bfq_bgzf_deflate), as a uint8 array; the same bytes as HostText.bgzf_deflate_model.  level 0: every member stored.
        `out`: a uint8 array to fill, of at least HostText.bgzf_deflate_bound(len(text)); the result is a view of it.  A
        smaller one, another level or a text that is already compressed (1f 8b) raise BfqError (BFQ_E_ARG), nothing written."""
        text = _u8(text)
        if out is None:
            out = np.empty(bgzf_deflate_bound(len(text)), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_bgzf_deflate(self.h, _ptr(text) if len(text) else None, len(text), int(level), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def bgzf_deflate_device(self, d_in, n, level=1):
        """bfq_bgzf_deflate_device: the BGZF form of the n bytes of text at the device address d_in, as a uint8 array."""
        out = np.empty(bgzf_deflate_bound(n), np.uint8)
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_bgzf_deflate_device(self.h, C.c_void_p(d_in), int(n), int(level), _ptr(out), len(out), C.byref(ol)))
        return out[:int(ol.value)]

    def bgzf_deflate_files(self, src, dst, level=1):
        """bfq_bgzf_deflate_fd on named files; returns the length of the BGZF file."""
        import os
        fds = []
        try:
            fds.append(os.open(src, os.O_RDONLY))
            fds.append(os.open(dst, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            ol = C.c_uint64(0)
            self._ck(self.L.bfq_bgzf_deflate_fd(self.h, fds[0], os.fstat(fds[0]).st_size, int(level), fds[1], C.byref(ol)))
            return int(ol.value)
        finally:
            for fd in fds:
                os.close(fd)

    def ebwt_decode(self, bwtz, qsz, out=None):
        """The line streams (dna, qs) of a pair of eBWT-domain containers (fastq_job(compress=2)); returns (dna, qs, n_reads)."""
        bwtz, qsz = _u8(bwtz), _u8(qsz)
        if len(bwtz) < 32 or bytes(bwtz[:8]) != b"BFQEBWT1":
            raise BfqError(-1, "not a BFQEBWT1 stream")
        n = int(np.frombuffer(bwtz[8:16].tobytes(), np.uint64)[0])
        dna, qs = out if out is not None else (np.empty(n + 16, np.uint8), np.empty(n + 16, np.uint8))
        sl, nr = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.bfq_stream_ebwt_decode(self.h, _ptr(bwtz), len(bwtz), _ptr(qsz), len(qsz), _ptr(dna), _ptr(qs),
                                               min(len(dna), len(qs)), C.byref(sl), C.byref(nr)))
        return dna[:int(sl.value)], qs[:int(sl.value)], int(nr.value)

    # ---- the way back: containers -> FASTQ text (bfq_fastq_restore)
    def fastq_restore(self, dna, qs, hdr=None, out=None, perm=None, groups=None, edits=None):
        """The FASTQ text of a collection from the containers of its streams (fastq_job(compress=1 / 2 / 3), stream_compress,
        the .bsc files of parallel.py --compress): (text as a uint8 array, n_reads).  hdr=None: every header line is "@".
        `out`: a uint8 array to fill (e.g. PinnedBuffer.array); the result is a view of it.  Streams that do not belong
        together raise BfqError (BFQ_E_ARG, the message names the first offending read) and leave `out` untouched.
        `perm`: the BFQPERM1 container of the reordering the collection went through (fastq_reorder(keep=True)): the records
        come back in the order before it (bfq_fastq_restore_ordered).
        `groups`: True, or (first, count) with count None = to the end: block by block (bfq_fastq_restore_grouped) -- the
        groups of HostText.restore_groups one after another in a device workspace sized by the largest of them, the same
        bytes as without; several BFQEBWT1 members are taken.  A failure after the first group may leave the texts of the
        groups before it in `out`.  Not with `perm`.
        `edits`: the BFQEDIT1 members of the run's base edits (fastq_job(edits=True), one per block, back to back): the text
        comes back with the input's bases (bfq_fastq_restore_edited); with `perm` too, the edits first.  Not with `groups`."""
        if groups is not None and groups is not False and perm is not None:
            raise ValueError("fastq_restore: groups and perm do not go together (records in the original order draw on all groups at once)")
        if groups is not None and groups is not False and edits is not None:
            raise ValueError("fastq_restore: groups and edits do not go together (a grouped text goes through fastq_unedit)")
        dna, qs = _u8(dna), _u8(qs)
        hdr = _u8(hdr) if hdr is not None else None
        perm = _u8(perm) if perm is not None else None
        hl = len(hdr) if hdr is not None else 0
        ol, nr = C.c_uint64(0), C.c_uint64(0)
        if groups is not None and groups is not False:
            first, count = (0, None) if groups is True else groups
            count = ALL_GROUPS if count is None else int(count)
            if out is None:
                plan = restore_groups(dna, qs, hdr)
                last = len(plan) if count == ALL_GROUPS else min(len(plan), first + count)
                out = np.empty(max(sum(g["text_bound"] for g in plan[first:last]), 1), np.uint8)
            self._ck(self.L.bfq_fastq_restore_grouped(self.h, _ptr(dna), len(dna), _ptr(qs), len(qs), _ptr(hdr), hl, int(first), count,
                                                      _ptr(out), len(out), C.byref(ol), C.byref(nr)))
            return out[:int(ol.value)], int(nr.value)
        if out is None:
            bound = int(self.L.bfq_fastq_restore_bound(_ptr(dna), len(dna), _ptr(qs), len(qs), _ptr(hdr), hl))
            if bound < 0:
                raise BfqError(-1, "not a container (BFQDNAC1 / BFQRANS2 / BFQLINE1 / BFQNAME1 / BFQQUAL1 / BFQEBWT1)")
            out = np.empty(max(bound, 1), np.uint8)
        if edits is not None:
            ez = _u8(edits)
            if not len(ez):
                raise BfqError(-1, "edits: not a BFQEDIT1 container (empty)")
            if perm is not None and not len(perm):
                raise BfqError(-1, "perm: not a BFQPERM1 container (empty)")
            self._ck(self.L.bfq_fastq_restore_edited(self.h, _ptr(dna), len(dna), _ptr(qs), len(qs), _ptr(hdr), hl,
                                                     _ptr(perm), len(perm) if perm is not None else 0, _ptr(ez), len(ez),
                                                     _ptr(out), len(out), C.byref(ol), C.byref(nr)))
        elif perm is not None:
            self._ck(self.L.bfq_fastq_restore_ordered(self.h, _ptr(dna), len(dna), _ptr(qs), len(qs), _ptr(hdr), hl,
                                                      _ptr(perm) if len(perm) else None, len(perm), _ptr(out), len(out), C.byref(ol), C.byref(nr)))
        else:
            self._ck(self.L.bfq_fastq_restore(self.h, _ptr(dna), len(dna), _ptr(qs), len(qs), _ptr(hdr), hl,
                                              _ptr(out), len(out), C.byref(ol), C.byref(nr)))
        return out[:int(ol.value)], int(nr.value)

    def fastq_restore_files(self, dna_path, qs_path, hdr_path, out_path, perm_path=None, grouped=False, bgzf=False, level=1, ubam=False,
                            edits_path=None, **ubam_kw):
        """bfq_fastq_restore_fd on named files (hdr_path may be None); returns (bytes written, n_reads).  perm_path: the
        BFQPERM1 file of the reordering (bfq_fastq_restore_ordered_fd): the text in the order before it.  grouped: True or
        (first, count) as fastq_restore's `groups` (bfq_fastq_restore_grouped_fd); not with perm_path.  bgzf: out_path is
        written as BGZF (bfq_fastq_restore_bgzf_fd: the text is deflated on the device at `level` and never crosses to the
        host); the bytes written are the compressed ones; not with grouped.  ubam: out_path is written as an unaligned BAM
        (bfq_fastq_restore_bam_fd: the restored text becomes records on the device, unpaired, deflated at `level`; further
        keywords: ubam_opts()); returns (bytes written, stats.records); not with grouped or bgzf.  edits_path: the BFQEDIT1
        file of the run's base edits (bfq_fastq_restore_edited_fd): the text with the input's bases; with perm_path too, the
        edits first; not with grouped, bgzf or ubam."""
        import os
        if edits_path is not None and (grouped or bgzf or ubam):
            raise ValueError("fastq_restore_files: edits_path does not go together with grouped, bgzf or ubam")
        if grouped and perm_path is not None:
            raise ValueError("fastq_restore_files: grouped and perm_path do not go together")
        if ubam and (grouped or bgzf):
            raise ValueError("fastq_restore_files: ubam does not go together with grouped or bgzf")
        if ubam_kw and not ubam:
            raise TypeError("fastq_restore_files: unexpected keywords %s" % sorted(ubam_kw))
        if grouped and bgzf:
            raise ValueError("fastq_restore_files: grouped and bgzf do not go together (the grouped restore writes plain text)")
        fds = []
        try:
            for p in (dna_path, qs_path, hdr_path, perm_path):
                fds.append(os.open(p, os.O_RDONLY) if p is not None else -1)
            fds.append(os.open(out_path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            fds.append(os.open(edits_path, os.O_RDONLY) if edits_path is not None else -1)
            ol, nr = C.c_uint64(0), C.c_uint64(0)
            size = lambda fd: os.fstat(fd).st_size if fd >= 0 else 0
            if edits_path is not None:
                self._ck(self.L.bfq_fastq_restore_edited_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]),
                                                            fds[3], size(fds[3]), fds[5], size(fds[5]), fds[4], C.byref(ol), C.byref(nr)))
            elif ubam:
                (O, held), st = ubam_opts(level=level, **ubam_kw), _lib.UbamStats()
                st.tags = getattr(O, "tag_stats", None)
                self._ck(self.L.bfq_fastq_restore_bam_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]),
                                                         fds[3], size(fds[3]), C.byref(O), fds[4], C.byref(ol), C.byref(st)))
                nr.value = st.records
            elif bgzf:
                raw = C.c_uint64(0)
                self._ck(self.L.bfq_fastq_restore_bgzf_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]),
                                                          fds[3], size(fds[3]), int(level), fds[4], C.byref(ol), C.byref(raw), C.byref(nr)))
            elif grouped:
                first, count = (0, None) if grouped is True else grouped
                self._ck(self.L.bfq_fastq_restore_grouped_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]),
                                                             int(first), ALL_GROUPS if count is None else int(count), fds[4],
                                                             C.byref(ol), C.byref(nr)))
            elif perm_path is not None:
                self._ck(self.L.bfq_fastq_restore_ordered_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]),
                                                             fds[3], size(fds[3]), fds[4], C.byref(ol), C.byref(nr)))
            else:
                self._ck(self.L.bfq_fastq_restore_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]), fds[4],
                                                     C.byref(ol), C.byref(nr)))
            return int(ol.value), int(nr.value)
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- the reads in another order before the input is cut into blocks (bfq_fastq_reorder; parallel.py --reorder)
    def fastq_reorder(self, parts, mode=2, k=21, seed=0, out=None, keep=False):
        """The records of a FASTQ text (parts = [text], or [mates 1, mates 2]: record i of both move together) in the order of
        include/bfqzip_hip.h: mode 2 by the smallest hashed k-mer of every read, mode 1 by a seeded hash of its index, ties
        in input order.  Returns ([text per part as uint8 arrays], perm) with perm[j] = input index of output record j.
        `out`: one uint8 array per part to fill (too small: BFQ_E_ARG, nothing written); the results are views of them.
        keep=True (bfq_fastq_reorder_keep): returns ([texts], container) instead, the permutation as the BFQPERM1 container
        that fastq_unreorder / fastq_restore(perm=) undo (perm_decode gives its entries)."""
        arrs, np_, tp, outs, ho, cap, ol = self._text_parts(parts, out)
        nr = C.c_uint64(0)
        O = _lib.ReorderOpts(mode=mode, k=k, seed=seed)
        nmax = (min(len(a) for a in arrs) if arrs else 0) // 4 + 1                                # a record has 4 bytes at least
        if keep:
            z = np.empty(int(self.L.bfq_perm_bound(nmax)), np.uint8)
            zl = C.c_uint64(0)
            self._ck(self.L.bfq_fastq_reorder_keep(self.h, tp, np_, C.byref(O), ho, cap, ol, _ptr(z), len(z), C.byref(zl), C.byref(nr)))
            return [o[:int(ol[i])] for i, o in enumerate(outs)], z[:int(zl.value)]
        perm = np.empty(max(nmax, 1), np.uint64)
        self._ck(self.L.bfq_fastq_reorder(self.h, tp, np_, C.byref(O), ho, cap, ol, _ptr(perm), C.byref(nr)))
        return [o[:int(ol[i])] for i, o in enumerate(outs)], perm[:int(nr.value)]

    @staticmethod
    def _text_parts(parts, out):
        arrs = [_u8(p) for p in parts]
        np_ = len(arrs)
        tp = (_lib.TextPart * max(np_, 1))()
        for i, a in enumerate(arrs):
            tp[i].data = a.ctypes.data if len(a) else None
            tp[i].len = len(a)
        outs = list(out) if out is not None else [np.empty(len(a) + 1, np.uint8) for a in arrs]
        ho = (C.c_void_p * max(np_, 1))(*[o.ctypes.data for o in outs])
        cap = (C.c_uint64 * max(np_, 1))(*[len(o) for o in outs])
        ol = (C.c_uint64 * max(np_, 1))()
        return arrs, np_, tp, outs, ho, cap, ol

    def fastq_unreorder(self, parts, perm, out=None):
        """The records of a reordered FASTQ text (parts as in fastq_reorder) back in their input order: output record perm[j]
        is input record j.  perm: the BFQPERM1 container fastq_reorder(keep=True) returned.  Returns [text per part].  A
        container that is not one, is of another read count or is not a permutation raises BfqError (BFQ_E_ARG; the message
        names the counts / the first offending position) and leaves `out` untouched."""
        z = _u8(perm)
        arrs, np_, tp, outs, ho, cap, ol = self._text_parts(parts, out)
        nr = C.c_uint64(0)
        self._ck(self.L.bfq_fastq_unreorder(self.h, tp, np_, _ptr(z) if len(z) else None, len(z), ho, cap, ol, C.byref(nr)))
        return [o[:int(ol[i])] for i, o in enumerate(outs)]

    def _reorder_files(self, inputs, outputs, perm_path, perm_write, call):
        import os
        assert len(inputs) == len(outputs)
        fin, fout, fperm = [], [], []
        try:
            for p in inputs:
                fin.append(os.open(p, os.O_RDONLY))
            for p in outputs:
                fout.append(os.open(p, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            if perm_path is not None:
                fperm.append(os.open(perm_path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) if perm_write else os.open(perm_path, os.O_RDONLY))
            n = len(fin)
            ol = (C.c_uint64 * max(n, 1))()
            nr = C.c_uint64(0)
            call((C.c_int * max(n, 1))(*fin), (C.c_uint64 * max(n, 1))(*[os.fstat(fd).st_size for fd in fin]), n, (C.c_int * max(n, 1))(*fout),
                 fperm[0] if fperm else -1, ol, nr)
            return [int(ol[i]) for i in range(n)], int(nr.value)
        finally:
            for fd in fin + fout + fperm:
                os.close(fd)

    def fastq_reorder_files(self, inputs, outputs, mode=2, k=21, seed=0, perm_path=None):
        """bfq_fastq_reorder_fd on named files (one, or the two files of mates); returns (bytes written per file, n_reads).
        On failure the output files are left empty.  perm_path: also write the permutation there as a BFQPERM1 container
        (bfq_fastq_reorder_keep_fd)."""
        O = _lib.ReorderOpts(mode=mode, k=k, seed=seed)

        def call(fin, sizes, n, fout, fperm, ol, nr):
            if perm_path is None:
                self._ck(self.L.bfq_fastq_reorder_fd(self.h, fin, sizes, n, C.byref(O), fout, ol, C.byref(nr)))
            else:
                zl = C.c_uint64(0)
                self._ck(self.L.bfq_fastq_reorder_keep_fd(self.h, fin, sizes, n, C.byref(O), fout, fperm, ol, C.byref(zl), C.byref(nr)))
        return self._reorder_files(inputs, outputs, perm_path, True, call)

    def fastq_unreorder_files(self, inputs, outputs, perm_path):
        """bfq_fastq_unreorder_fd on named files: the reordered file(s) and the BFQPERM1 file -> the records in their input
        order; returns (bytes written per file, n_reads).  On failure the output files are left empty."""
        import os

        def call(fin, sizes, n, fout, fperm, ol, nr):
            self._ck(self.L.bfq_fastq_unreorder_fd(self.h, fin, sizes, n, fperm, os.fstat(fperm).st_size, fout, ol, C.byref(nr)))
        return self._reorder_files(inputs, outputs, perm_path, False, call)

    # ---- what a run changed: two FASTQ texts compared on the GPU (bfq_fastq_compare)
    def fastq_compare(self, a_parts, b_parts, perm=None, max_diffs=0, diffs_out=None):
        """A ("before") against B ("after"), each a list of 1..4 texts taken as one: a CompareReport.  perm: the BFQPERM1
        container of the run that gave B its order (record j of B pairs with record perm[j] of A; every read index reported
        is A's).  max_diffs: list that many differing positions at most (.diffs).  diffs_out: a DIFF_DTYPE array of at least
        max_diffs entries to fill; .diffs is a view of it.  Texts that do not pair (record counts, a read's length), a bad
        permutation or malformed text raise BfqError and leave diffs_out untouched."""
        pa, pb = [_u8(p) for p in a_parts], [_u8(p) for p in b_parts]

        def parts(arrs):
            tp = (_lib.TextPart * max(len(arrs), 1))()
            for i, x in enumerate(arrs):
                tp[i].data = x.ctypes.data if len(x) else None
                tp[i].len = len(x)
            return tp
        z = _u8(perm) if perm is not None else None
        buf = diffs_out if diffs_out is not None else np.zeros(max(int(max_diffs), 1), DIFF_DTYPE)
        assert buf.dtype == DIFF_DTYPE and len(buf) >= max_diffs
        raw = _lib.CompareReport()
        self._ck(self.L.bfq_fastq_compare(self.h, parts(pa), len(pa), parts(pb), len(pb), _ptr(z) if z is not None else None,
                                          len(z) if z is not None else 0, C.byref(raw), _ptr(buf) if max_diffs else None, int(max_diffs)))
        return CompareReport(raw, buf[:min(int(raw.n_diffs), int(max_diffs))])

    def fastq_compare_files(self, a_path, b_path, perm_path=None, max_diffs=0):
        """fastq_compare on named files (bfq_fastq_compare_fd)."""
        import os
        fds = []
        try:
            for p in (a_path, b_path, perm_path):
                fds.append(os.open(p, os.O_RDONLY) if p is not None else -1)
            size = lambda fd: os.fstat(fd).st_size if fd >= 0 else 0
            buf = np.zeros(max(int(max_diffs), 1), DIFF_DTYPE)
            raw = _lib.CompareReport()
            self._ck(self.L.bfq_fastq_compare_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), fds[2], size(fds[2]), C.byref(raw),
                                                 _ptr(buf) if max_diffs else None, int(max_diffs)))
            return CompareReport(raw, buf[:min(int(raw.n_diffs), int(max_diffs))])
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    # ---- bases back exactly: a run's base edits as a BFQEDIT1 container (bfq_fastq_edits / bfq_fastq_unedit)
    @staticmethod
    def _parts(arrs):
        tp = (_lib.TextPart * max(len(arrs), 1))()
        for i, x in enumerate(arrs):
            tp[i].data = x.ctypes.data if len(x) else None
            tp[i].len = len(x)
        return tp

    def fastq_edits(self, a_parts, b_parts, out=None):
        """The BFQEDIT1 member of the run that made B (its output) from A (its input), each a list of 1..4 texts taken as one,
        in the same read order: (member as a uint8 array, EditStats).  `out`: a uint8 array to fill (default: input length / 8
        + 4096 bytes); too small, texts that do not pair or malformed text raise BfqError and leave it untouched."""
        pa, pb = [_u8(p) for p in a_parts], [_u8(p) for p in b_parts]
        out = out if out is not None else np.empty(sum(text_len(a) for a in pa) // 8 + 4096, np.uint8)
        ol, st = C.c_uint64(0), _lib.EditStats()
        self._ck(self.L.bfq_fastq_edits(self.h, self._parts(pa), len(pa), self._parts(pb), len(pb), _ptr(out), len(out), C.byref(ol), C.byref(st)))
        return out[:int(ol.value)], st

    def fastq_edits_device(self, d_a, a_len, d_b, b_len, d_out, cap):
        """fastq_edits with both plain texts and the member in device memory (pointers, e.g. torch data_ptr()): (length, EditStats)."""
        ol, st = C.c_uint64(0), _lib.EditStats()
        self._ck(self.L.bfq_fastq_edits_device(self.h, d_a, a_len, d_b, b_len, d_out, cap, C.byref(ol), C.byref(st)))
        return int(ol.value), st

    def edits_make_device(self, d_in_bases, d_out_bases, d_roff, N, total, d_out, cap):
        """bfq_edits_make_device: the member of two base arrays that share their read offsets (the layout of run_reads_device),
        everything in device memory: (length, EditStats).  cap too small: BfqError; .needed holds the size that suffices."""
        ol, st = C.c_uint64(0), _lib.EditStats()
        rc = self.L.bfq_edits_make_device(self.h, d_in_bases, d_out_bases, d_roff, N, total, d_out, cap, C.byref(ol), C.byref(st))
        if rc:
            e = BfqError(rc, self.L.bfq_last_error(self.h).decode())
            e.needed = int(st.bytes)
            raise e
        return int(ol.value), st

    def edits_apply_device(self, edits, d_bases, d_roff, N, total, lines=False):
        """bfq_edits_apply_device: the members of `edits` (host memory) validated against and written into a base array (or,
        lines=True, a line stream) in device memory: EditStats.  Any refusal leaves the target untouched."""
        z, st = _u8(edits), _lib.EditStats()
        self._ck(self.L.bfq_edits_apply_device(self.h, _ptr(z) if len(z) else None, len(z), d_bases, d_roff, N, total, 1 if lines else 0, C.byref(st)))
        return st

    def _two_files(self, paths, out_path, call):
        import os
        fds = []
        try:
            for p in paths:
                fds.append(os.open(p, os.O_RDONLY))
            fds.append(os.open(out_path, os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644))
            ol, st = C.c_uint64(0), _lib.EditStats()
            self._ck(call(fds, [os.fstat(fd).st_size for fd in fds], C.byref(ol), C.byref(st)))
            return int(ol.value), st
        finally:
            for fd in fds:
                os.close(fd)

    def fastq_edits_files(self, a_path, b_path, out_path):
        """bfq_fastq_edits_fd on named files; returns (bytes written, EditStats).  On failure out_path is left empty."""
        return self._two_files((a_path, b_path), out_path,
                               lambda fd, sz, ol, st: self.L.bfq_fastq_edits_fd(self.h, fd[0], sz[0], fd[1], sz[1], fd[2], ol, st))

    def fastq_unedit(self, text, edits, out=None):
        """`text` (a run's output, plain or BGZF) with the input's bases written back from the BFQEDIT1 members of `edits`
        (one per block, back to back); every other byte stays: (text as a uint8 array, EditStats).  Members that are damaged,
        of another collection (reads, bases, read lengths) or of another output (target_sum) raise BfqError and leave `out`
        untouched."""
        t, z = _u8(text), _u8(edits)
        out = out if out is not None else np.empty(text_len(t) + 1, np.uint8)
        ol, st = C.c_uint64(0), _lib.EditStats()
        self._ck(self.L.bfq_fastq_unedit(self.h, _ptr(t) if len(t) else None, len(t), _ptr(z) if len(z) else None, len(z), _ptr(out), len(out),
                                         C.byref(ol), C.byref(st)))
        return out[:int(ol.value)], st

    def fastq_unedit_files(self, text_path, edits_path, out_path):
        """bfq_fastq_unedit_fd on named files; returns (bytes written, EditStats).  On failure out_path is left empty."""
        return self._two_files((text_path, edits_path), out_path,
                               lambda fd, sz, ol, st: self.L.bfq_fastq_unedit_fd(self.h, fd[0], sz[0], fd[1], sz[1], fd[2], ol, st))

    edits_info = staticmethod(lambda z: edits_info(z))
    fastq_edits_host = staticmethod(lambda a, b, out=None: fastq_edits_host(a, b, out))
    fastq_unedit_host = staticmethod(lambda t, z, out=None: fastq_unedit_host(t, z, out))

    # ---- which k-mers a run removed, kept and created (bfq_fastq_kmers)
    def fastq_kmers(self, a_parts, b_parts=None, k=21, solid=3, canonical=True, max_list=0, list_out=None, part_records=0):
        """The k-mer spectrum of A, or of A ("before") against B ("after"), each a list of 1..4 texts taken as one: a
        KmerReport.  Nothing is paired: the order of the reads does not matter.  max_list: list that many k-mers at most
        that went solid -> absent or absent -> solid (.listed).  list_out: a KMER_DTYPE array of at least max_list entries to
        fill.  part_records: the records of a value range at most (0: what the memory allows).  Malformed text or options
        out of range raise BfqError and leave list_out untouched."""
        pa, pb = [_u8(p) for p in a_parts], [_u8(p) for p in (b_parts or [])]

        def parts(arrs):
            tp = (_lib.TextPart * max(len(arrs), 1))()
            for i, x in enumerate(arrs):
                tp[i].data = x.ctypes.data if len(x) else None
                tp[i].len = len(x)
            return tp
        return _kmer_call(lambda po, pr, pl, cap: self._ck(self.L.bfq_fastq_kmers(self.h, parts(pa), len(pa), parts(pb) if pb else None, len(pb),
                                                                                   po, pr, pl, cap)), k, solid, canonical, max_list, list_out, part_records)

    def fastq_kmers_files(self, a_path, b_path=None, k=21, solid=3, canonical=True, max_list=0, list_out=None, part_records=0):
        """fastq_kmers on named files (bfq_fastq_kmers_fd)."""
        import os
        fds = []
        try:
            for p in (a_path, b_path):
                fds.append(os.open(p, os.O_RDONLY) if p is not None else -1)
            size = lambda fd: os.fstat(fd).st_size if fd >= 0 else 0
            return _kmer_call(lambda po, pr, pl, cap: self._ck(self.L.bfq_fastq_kmers_fd(self.h, fds[0], size(fds[0]), fds[1], size(fds[1]), po, pr, pl, cap)),
                              k, solid, canonical, max_list, list_out, part_records)
        finally:
            for fd in fds:
                if fd >= 0:
                    os.close(fd)

    @staticmethod
    def fastq_kmers_host(a, b=None, k=21, solid=3, canonical=True, max_list=0, list_out=None, part_records=0):
        return fastq_kmers_host(a, b, k=k, solid=solid, canonical=canonical, max_list=max_list, list_out=list_out, part_records=part_records)

    # ---- the permutation as a container (host only)
    @staticmethod
    def perm_encode(perm, mode=0, k=0, seed=0):
        return perm_encode(perm, mode=mode, k=k, seed=seed)

    @staticmethod
    def perm_decode(permz):
        return perm_decode(permz)

    def stream_compress_device(self, d_in, n, d_out, cap):
        """Device-resident form (after stream_reserve(n)); returns the container's length."""
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_stream_compress_device(self.h, d_in, n, d_out, cap, C.byref(ol)))
        return int(ol.value)

    def names_compress_device(self, d_in, n, d_out, cap, always=False):
        """names_compress with both buffers in device memory (pointers, e.g. torch data_ptr()); the call sizes the engine's
        workspace itself.  Returns the container's length."""
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_names_compress_device(self.h, d_in, n, 1 if always else 0, d_out, cap, C.byref(ol)))
        return int(ol.value)

    def quals_compress_device(self, d_in, n, d_out, cap, always=False, rung=None):
        """quals_compress with both buffers in device memory (pointers, e.g. torch data_ptr()); the call sizes the engine's
        workspace itself.  Returns the container's length."""
        ol = C.c_uint64(0)
        self._ck(self.L.bfq_quals_compress_device(self.h, d_in, n, self._quals_flags(always, rung), d_out, cap, C.byref(ol)))
        return int(ol.value)

    def stream_reserve(self, n):
        self._ck(self.L.bfq_stream_reserve(self.h, n))

    def stream_bound(self, n):
        return int(self.L.bfq_stream_bound(n))

    # ---- profiling
    def posbin_sparse_last(self):
        """(polarity, rows_sent) of the last call's position bins: 0 = keep, 1 = const, -1 = every row travelled or none ran."""
        pol, sent = C.c_int(-1), C.c_uint64(0)
        self._ck(self.L.bfq_posbin_sparse_last(self.h, C.byref(pol), C.byref(sent)))
        return int(pol.value), int(sent.value)

    def refine_form(self):
        """The refinement's chunk kernel in use: 1 = text words by two loads side by side, 0 = BFQ_REFINE_PIPE=0 (as set_params() read it)."""
        return int(self.L.bfq_refine_form(self.h))

    def prof_reset(self):
        self.L.bfq_prof_reset(self.h)

    def prof(self):
        out = {}
        name = C.create_string_buffer(64)
        for i in range(self.L.bfq_prof_count(self.h)):
            ms = C.c_double(); ln = C.c_uint64(); by = C.c_double()
            self.L.bfq_prof_get(self.h, i, name, 64, C.byref(ms), C.byref(ln), C.byref(by))
            if ln.value:
                out[name.value.decode()] = {"ms": ms.value, "launches": ln.value, "alg_bytes": by.value}
        return out

    def prof_trace_select(self, kernel):
        """Keep the per-launch durations of `kernel` (a name prof() reports, or None) from now on."""
        name = C.create_string_buffer(64)
        idx = -1
        for i in range(self.L.bfq_prof_count(self.h)):
            self.L.bfq_prof_get(self.h, i, name, 64, None, None, None)
            if kernel is not None and name.value.decode() == kernel:
                idx = i
        if kernel is not None and idx < 0:
            raise KeyError(kernel)
        self._ck(self.L.bfq_prof_trace_select(self.h, idx))

    def prof_trace(self):
        """Per-launch milliseconds of the selected kernel since the last prof_reset(), launch order (float32 array)."""
        k = int(self.L.bfq_prof_trace(self.h, None, 0))
        out = np.empty(max(k, 0), np.float32)
        if k > 0:
            self.L.bfq_prof_trace(self.h, _ptr(out), k)
        return out

    def workspace_bytes(self):
        return int(self.L.bfq_workspace_bytes(self.h))

    def workspace_read(self, off, length):
        """The workspace's bytes [off, off + length) as they are once the queued work has finished (cut at its end): a test hook
        (BFQ_POISON)."""
        out = np.empty(int(length), np.uint8)
        got = int(self.L.bfq_workspace_read(self.h, int(off), out.ctypes.data, len(out))) if len(out) else 0
        return out[:got]


def reorder_key(seq, k=21):
    """The mode-2 sort key of one sequence line (bfq_reorder_key: host only, no GPU)."""
    a = _u8(seq)
    return int(_lib.lib().bfq_reorder_key(_ptr(a) if len(a) else None, len(a), k))


class PermError(BfqError):
    """perm_encode / perm_decode refused their input; first_bad: the first offending position, None for a fault in the header
    (or, from perm_encode, which reports no position)."""

    def __init__(self, code, msg, first_bad=None):
        super().__init__(code, msg)
        self.first_bad = first_bad


class EditsError(BfqError):
    """A BFQEDIT1 container was refused; first_bad: its first offending edit, None for a fault in the header or the table."""

    def __init__(self, code, msg, first_bad=None):
        super().__init__(code, msg)
        self.first_bad = first_bad


def _edits_err():
    return _lib.lib().bfq_edits_host_error().decode()


def edits_bound(n_edits, total_bases):
    """A capacity that always suffices for the BFQEDIT1 container of n_edits edits in total_bases bases (host only)."""
    return int(_lib.lib().bfq_edits_bound(n_edits, total_bases))


def edits_info(edits):
    """dict(n_reads, total_bases, n_edits, members) of the BFQEDIT1 members of a buffer, from their headers and tables
    (bfq_edits_info: host only, no GPU)."""
    z = _u8(edits)
    v = [C.c_uint64(0) for _ in range(4)]
    rc = _lib.lib().bfq_edits_info(_ptr(z) if len(z) else None, len(z), *[C.byref(x) for x in v])
    if rc:
        raise EditsError(rc, _edits_err())
    return dict(zip(("n_reads", "total_bases", "n_edits", "members"), (int(x.value) for x in v)))


def edits_members(edits):
    """The members of a buffer as views of it, one per block of a sharded run."""
    z, L, out, at = _u8(edits), _lib.lib(), [], 0
    while at < len(z):
        n = int(L.bfq_edits_member_len(_ptr(z[at:]), len(z) - at))
        if n < 0:
            raise EditsError(-1, "member %d: not a well-formed BFQEDIT1 member" % len(out))
        out.append(z[at:at + n])
        at += n
    return out


def edits_encode(pos, byte, n_reads, total_bases, shape, target_sum):
    """The edit list (pos: ascending uint64 positions, byte: the input's bytes there) -> one BFQEDIT1 member (bfq_edits_encode:
    host only)."""
    p, b = np.ascontiguousarray(pos, np.uint64), np.ascontiguousarray(byte, np.uint8)
    assert len(p) == len(b)
    out = np.empty(max(edits_bound(len(p), total_bases), 64), np.uint8)
    ol = C.c_uint64(0)
    rc = _lib.lib().bfq_edits_encode(_ptr(p) if len(p) else None, _ptr(b) if len(b) else None, len(p), n_reads, total_bases, shape, target_sum,
                                     _ptr(out), len(out), C.byref(ol))
    if rc:
        raise EditsError(rc, "bfq_edits_encode: positions not ascending or not below the bases, or a byte outside 33..126")
    return out[:int(ol.value)]


def edits_decode(member):
    """ONE BFQEDIT1 member -> dict(pos, byte, n_reads, total_bases, n_edits, shape, target_sum) (bfq_edits_decode: host only).
    A member that is not well formed: EditsError with first_bad."""
    z = _u8(member)
    cap = max(len(z), 1)                                           # a member holds a byte per edit
    p, b = np.empty(cap, np.uint64), np.empty(cap, np.uint8)
    v = [C.c_uint64(0) for _ in range(6)]
    rc = _lib.lib().bfq_edits_decode(_ptr(z) if len(z) else None, len(z), _ptr(p), _ptr(b), cap, *[C.byref(x) for x in v])
    if rc:
        fb = None if v[5].value == (1 << 64) - 1 else int(v[5].value)
        raise EditsError(rc, "bfq_edits_decode: " + _edits_err() + ("" if fb is None else f": edit {fb}"), fb)
    n = int(v[2].value)
    return dict(pos=p[:n], byte=b[:n], n_reads=int(v[0].value), total_bases=int(v[1].value), n_edits=n, shape=int(v[3].value),
                target_sum=int(v[4].value))


def fastq_edits_host(a, b, out=None):
    """bfq_fastq_edits_host: the BFQEDIT1 member of the run that made text b from text a, on one thread of the host (the
    statement the device path is tested against).  Returns (member, EditStats)."""
    a, b = _u8(a), _u8(b)
    out = out if out is not None else np.empty(max(edits_bound(len(a) // 2, len(a) // 2), 64), np.uint8)
    ol, st = C.c_uint64(0), _lib.EditStats()
    rc = _lib.lib().bfq_fastq_edits_host(_ptr(a) if len(a) else None, len(a), _ptr(b) if len(b) else None, len(b), _ptr(out), len(out),
                                         C.byref(ol), C.byref(st))
    if rc:
        raise EditsError(rc, _edits_err())
    return out[:int(ol.value)], st


def fastq_unedit_host(text, edits, out=None):
    """bfq_fastq_unedit_host: text with the input's bases written back from the members of `edits`.  Returns (text, EditStats)."""
    t, z = _u8(text), _u8(edits)
    out = out if out is not None else np.empty(max(len(t), 1), np.uint8)
    ol, st = C.c_uint64(0), _lib.EditStats()
    rc = _lib.lib().bfq_fastq_unedit_host(_ptr(t) if len(t) else None, len(t), _ptr(z) if len(z) else None, len(z), _ptr(out), len(out),
                                          C.byref(ol), C.byref(st))
    if rc:
        raise EditsError(rc, _edits_err())
    return out[:int(ol.value)], st


def perm_bound(n_reads):
    """The exact length of the BFQPERM1 container of n_reads entries."""
    return int(_lib.lib().bfq_perm_bound(n_reads))


def perm_reads(permz):
    """N of a BFQPERM1 container, or -1 when its magic, entry width, length or padding are wrong (host only)."""
    z = _u8(permz)
    return int(_lib.lib().bfq_perm_reads(_ptr(z) if len(z) else None, len(z)))


def perm_encode(perm, mode=0, k=0, seed=0):
    """perm (uint64 array: perm[j] = input index of output record j) -> its BFQPERM1 container as a uint8 array
    (bfq_perm_encode: host only, no GPU).  Not a permutation: PermError."""
    p = np.ascontiguousarray(perm, np.uint64)
    out = np.empty(perm_bound(len(p)), np.uint8)
    O = _lib.ReorderOpts(mode=mode, k=k, seed=seed)
    ol = C.c_uint64(0)
    rc = _lib.lib().bfq_perm_encode(_ptr(p) if len(p) else None, len(p), C.byref(O), _ptr(out), len(out), C.byref(ol))
    if rc:
        raise PermError(rc, "bfq_perm_encode: not a permutation")
    return out[:int(ol.value)]


def perm_decode(permz):
    """BFQPERM1 container -> (perm as a uint64 array, dict(mode, k, seed)) (bfq_perm_decode: host only, no GPU).  A container
    that is not well formed: PermError with first_bad."""
    z = _u8(permz)
    L = _lib.lib()
    n = max(int(L.bfq_perm_reads(_ptr(z) if len(z) else None, len(z))), 0)
    p = np.empty(max(n, 1), np.uint64)
    N, bad = C.c_uint64(0), C.c_uint64(0)
    O = _lib.ReorderOpts()
    rc = L.bfq_perm_decode(_ptr(z) if len(z) else None, len(z), _ptr(p), n, C.byref(N), C.byref(O), C.byref(bad))
    if rc:
        fb = None if bad.value == (1 << 64) - 1 else int(bad.value)
        raise PermError(rc, "bfq_perm_decode: not a well-formed BFQPERM1 container" + ("" if fb is None else f": entry {fb}"), fb)
    return p[:int(N.value)], dict(mode=int(O.mode), k=int(O.k), seed=int(O.seed))


def synth_spec(N, L, Lmax=None, seed=20240807, **kw):
    s = _lib.Synth()
    _lib.lib().bfq_synth_default(C.byref(s), N, L)
    s.seed = seed
    if Lmax is not None:
        s.Lmax = Lmax
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def synth_host(spec):
    """Generate the synthetic reads on the host (same bytes as the device generator)."""
    L = _lib.lib()
    total = int(L.bfq_synth_total(C.byref(spec)))
    bases = np.empty(max(total, 1), np.uint8); quals = np.empty(max(total, 1), np.uint8)
    roff = np.empty(spec.N + 1, np.uint64)
    rc = L.bfq_synth_host(C.byref(spec), _ptr(bases), _ptr(quals), _ptr(roff))
    if rc:
        raise BfqError(rc, "bfq_synth_host")
    return bases[:total], quals[:total], roff
