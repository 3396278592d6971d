"""A model of the BAM input (csrc/bfq_bam.h): BAM files written with struct from record lists, the FASTQ texts and the
counts expected of them computed from the same lists (never by parsing), and the record-start rule, the walkers, the chain
and the repair restated in Python for the statistics of a piece size.  BGZF wrapping: tests/bgzf_model.bgzf()."""
import functools
import random
import struct
from collections import namedtuple
from tests import bgzf_model as B

SEQ = b"=ACMGRSVTWYHKDBN"
COMP = b"=TGKCYSBAWRDMHVN"
MAX_READ_LEN = 65000
MAX_BLOCK = 1 << 24
DEF_PIECE = 65536
PIECES = (256, 1024, 4096, 0)
NONE = None

# reason codes of bfq_bam.h, in its order, and how the messages word them
REASONS = ("OK", "MAGIC", "HDR_SHORT", "L_TEXT", "N_REF", "L_NAME", "REF_NUL", "SMALL", "BIG", "PAST", "NAME0", "LAYOUT", "NAME", "REF", "TOO_LONG")
R = {k: i for i, k in enumerate(REASONS)}
REASON_TEXT = (
    "ok", "no BAM magic (42 41 4d 01 expected)", "the stream ends inside the header", "negative header text length",
    "reference count outside [0, 1048576]", "reference name length below 1", "reference name without its final NUL", "block size below 32",
    "block size above 16777216", "the record runs past the end of the stream", "read name length 0",
    "name, CIGAR, sequence and qualities do not fit the block", "read name without its final NUL or with a NUL inside",
    "reference index outside [-1, n_ref)", "read longer than 65000 bases")
E_ARG, E_TOO_LONG = -1, -5

# name: bytes without the NUL; seq: bytes over SEQ; qual: raw phred bytes, or None = absent; cigar: u32 values; aux: bytes
Rec = namedtuple("Rec", "name flag seq qual cigar ref pos nref npos aux")


def rec(name, flag, seq, qual, cigar=(), ref=-1, pos=-1, nref=-1, npos=-1, aux=b""):
    return Rec(name, flag, seq, qual, tuple(cigar), ref, pos, nref, npos, aux)


def encode(r):
    l = len(r.seq)
    packed = bytearray((l + 1) // 2)
    for i, ch in enumerate(r.seq):
        packed[i >> 1] |= SEQ.index(ch) << (0 if i & 1 else 4)
    qual = r.qual if r.qual is not None else b"\xff" * l
    assert len(qual) == l and len(r.name) <= 254
    body = struct.pack("<iiBBHHHIiii", r.ref, r.pos, len(r.name) + 1, 0, 4680, len(r.cigar), r.flag, l, r.nref, r.npos, 0)
    body += r.name + b"\0" + b"".join(struct.pack("<I", c) for c in r.cigar) + bytes(packed) + qual + r.aux
    return struct.pack("<I", len(body)) + body


def header(text=b"", refs=()):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        h += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    return h


def aux_z(tag, value):
    return tag + b"Z" + value + b"\0"


def aux_b(tag, data):
    return tag + b"BC" + struct.pack("<I", len(data)) + data


class Case:
    """One good input: recs, the inflated stream, the file (BGZF unless raw), where the records begin, n_ref."""
    def __init__(self, recs, text=b"", refs=(), level=6, raw=False):
        self.recs, self.n_ref = list(recs), len(refs)
        h = header(text, refs)
        self.hdr_end = len(h)
        self.stream = h + b"".join(encode(r) for r in self.recs)
        self.blob = self.stream if raw else B.bgzf(self.stream, level=level)


# ---------------------------------------------------------------- what a record list becomes
def mate(flag):
    return 1 if flag & 0x40 and not flag & 0x80 else 2 if flag & 0x80 and not flag & 0x40 else 0


def expected(recs, exclude_flags=0x900, mate_suffix=1, default_qual=1, split=0, **_):
    """(the three texts, the counts that depend on the records alone)"""
    out = [bytearray(), bytearray(), bytearray()]
    st = dict(records=len(recs), written=[0, 0, 0], skipped=0, reversed=0, no_qual=0, clamped_quals=0)
    for r in recs:
        if r.flag & exclude_flags:
            st["skipped"] += 1
            continue
        k = mate(r.flag) if split else 0
        seq = r.seq
        if r.qual is None or (len(r.qual) and r.qual[0] == 0xFF):
            qual = bytes([default_qual + 33]) * len(seq)
            st["no_qual"] += 1 if len(seq) else 0
        else:
            st["clamped_quals"] += sum(1 for q in r.qual if q > 93)
            qual = bytes(min(q, 93) + 33 for q in r.qual)
        if r.flag & 0x10:
            seq = bytes(COMP[SEQ.index(ch)] for ch in reversed(seq))
            qual = qual[::-1]
            st["reversed"] += 1
        sfx = (b"/1", b"/2")[mate(r.flag) - 1] if mate_suffix and mate(r.flag) else b""
        out[k] += b"@" + r.name + sfx + b"\n" + seq + b"\n+\n" + qual + b"\n"
        st["written"][k] += 1
    return [bytes(o) for o in out], st


# ---------------------------------------------------------------- the rule, the walkers, the chain (bfq_bam.h restated)
def check(s, o, nref, strict=False):
    """(reason, where the record ends) of the record at s[o]; reason 255: well-formed, but no candidate"""
    n = len(s)
    if n - o < 4:
        return R["PAST"], 0
    bs = struct.unpack_from("<I", s, o)[0]
    if bs < 32:
        return R["SMALL"], 0
    if bs > MAX_BLOCK:
        return R["BIG"], 0
    if bs > n - o - 4:
        return R["PAST"], 0
    ref, pos, ln, _, _, nc, flag, lseq, nref2, npos, _ = struct.unpack_from("<iiBBHHHIiii", s, o + 4)
    if ln == 0:
        return R["NAME0"], 0
    if 32 + ln + 4 * nc + (lseq + 1) // 2 + lseq > bs:
        return R["LAYOUT"], 0
    name = s[o + 36:o + 36 + ln]
    if name[-1] != 0 or 0 in name[:-1]:
        return R["NAME"], 0
    if not (-1 <= ref < nref and -1 <= nref2 < nref):
        return R["REF"], 0
    if lseq > MAX_READ_LEN:
        return R["TOO_LONG"], 0
    if strict and (pos < -1 or npos < -1 or any(c < 0x21 or c > 0x7e for c in name[:-1])):
        return 255, 0
    return 0, o + 4 + bs


def candidate(s, o, nref):
    r, nxt = check(s, o, nref, True)
    return r == 0 and (nxt == len(s) or check(s, nxt, nref, True)[0] == 0)


def walk(s, start, end, nref):
    """(landing, dead, records) of a walker"""
    o, n = start, 0
    while o < end:
        r, nxt = check(s, o, nref)
        if r:
            return o, True, n
        o, n = nxt, n + 1
    return o, False, n


@functools.lru_cache(maxsize=None)
def _chain(s, h, nref, piece):
    n = len(s)
    np_ = max(1, -(-(n - h) // piece))
    starts, land, dead = [], [], []
    for k in range(np_):
        lo, hi = h + k * piece, min(n, h + (k + 1) * piece)
        c = h if k == 0 else next((o for o in range(lo, hi) if candidate(s, o, nref)), NONE)
        starts.append(c)
        l, d, _ = walk(s, c, hi, nref) if c is not NONE else (0, False, 0)
        land.append(l)
        dead.append(d)
    st = dict(pieces=np_, walkers=sum(c is not NONE for c in starts), dead=sum(dead), repaired=0, rounds=1)
    pos = h
    while pos < n:
        k = (pos - h) // piece
        if starts[k] != pos:
            land[k], d, _ = walk(s, pos, min(n, h + (k + 1) * piece), nref)
            assert not d
            st["repaired"] += 1
            st["rounds"] += 1
        pos = land[k]
    return st, sum(c is NONE for c in starts)


def chain(case, piece):
    """(pieces, walkers, dead, repaired, rounds of a good input at a piece size; the pieces that start no walker)"""
    return _chain(case.stream, case.hdr_end, case.n_ref, piece or DEF_PIECE)


@functools.lru_cache(maxsize=None)
def _expect(case, opts):
    return expected(case.recs, **dict(opts))


def expect(case, **opts):
    """expected() of a good input, computed once per option set"""
    return _expect(case, tuple(sorted(opts.items())))


def stats(case, piece, **opts):
    """every field of bfq_bam_stats for a good input"""
    st = dict(expect(case, **opts)[1], n_ref=case.n_ref, header_bytes=case.hdr_end)
    st["written"] = list(st["written"])
    st.update(chain(case, piece)[0])
    return st


# ---------------------------------------------------------------- inputs
RG = aux_z(b"RG", b"grp1")


def rand_rec(rng, i, flags, lmax=250, lmin=0, qmax=40, prefix=b"r"):
    l = rng.randint(lmin, lmax)
    flag = rng.choice(flags)
    aux = RG + (aux_b(b"XB", bytes(rng.getrandbits(8) for _ in range(rng.randint(1, 120)))) if i % 50 == 49 else b"")
    return rec(prefix + b"%d:%d" % (i // 2, rng.randint(0, 99999)), flag, bytes(rng.choice(b"ACGTN") for _ in range(l)),
               bytes(rng.randint(0, qmax) for _ in range(l)), aux=aux)


UBAM_FLAGS = (4, 77, 141, 77 | 16, 141 | 16, 0x104, 0x804)


def ubam(n=4000, seed=5):
    rng = random.Random(seed)
    return [rand_rec(rng, i, UBAM_FLAGS) for i in range(n)]


def edges():
    rng = random.Random(6)
    q = lambda l, hi=60: bytes(rng.randint(0, hi) for _ in range(l))
    out = [rec(b"e%d" % l, 4, bytes(rng.choice(b"ACGT") for _ in range(l)), q(l)) for l in (0, 1, 2, 3, 7, 8, 63, 64, 65, 129)]
    out += [rec(b"", 4, b"ACGT", q(4)), rec(b"", 77, b"", b""), rec(b"n" * 254, 141, b"ACGTA", q(5)), rec(b"n" * 254, 77 | 16, b"", b"")]
    out += [rec(b"all16", 4, SEQ, q(16)), rec(b"all16r", 4 | 16, SEQ, q(16)), rec(b"all15r", 16, SEQ[:15], q(15)), rec(b"all16r1", 77 | 16, SEQ * 5, q(80))]
    out += [rec(b"noq", 4, b"ACGTACGTAC", None), rec(b"noqr", 77 | 16, b"AACCGGTTN", None), rec(b"noq0", 4, b"", None)]
    out += [rec(b"hiq", 4, b"ACGTACG", bytes([93, 94, 255, 0, 200, 92, 254])), rec(b"hiqr", 141 | 16, b"ACGTAC", bytes([10, 255, 94, 93, 95, 1]))]
    out += [rec(b"both", 4 | 0x40 | 0x80, b"ACGT", q(4)), rec(b"bothr", 0xC0 | 16, b"ACGTT", q(5)), rec(b"sec", 0x100 | 0x40, b"AC", q(2)), rec(b"sup", 0x800, b"ACG", q(3))]
    out += [rec(b"cig", 0, b"ACGTACGTAC", q(10), cigar=(10 << 4,)), rec(b"cig3", 16, b"ACGTACGTACG", q(11), cigar=(3 << 4 | 4, 5 << 4, 3 << 4 | 4))]
    return out


def long_read():
    rng = random.Random(8)
    recs = [rand_rec(rng, i, (4, 77, 141), lmax=80) for i in range(40)]
    recs.insert(20, rec(b"long", 4, bytes(rng.choice(b"ACGT") for _ in range(60000)), bytes(rng.randint(2, 40) for _ in range(60000)), aux=RG))
    return recs


def embedded(resync, seed=9):
    """Records of which one carries, first in a piece of every size up to the default, a B array that holds two well-formed
    records: followed by garbage (a walker that starts there dies), or -- resync -- ending exactly where the carrier ends, so
    that the walker falls back into step with counts that are wrong."""
    rng = random.Random(seed)
    hdr = len(header())
    boundary = hdr + DEF_PIECE                                     # a piece boundary at 256, 1024, 4096 and 65536
    recs, at, i = [], hdr, 0
    while True:
        r = rand_rec(rng, i, (4, 77, 141), lmax=200, lmin=100)
        if at + len(encode(r)) > boundary - 60:
            break
        recs.append(r)
        at += len(encode(r))
        i += 1
    inner = encode(rec(b"ghost1", 4, b"ACGTACGT", bytes(8 * [30]))) + encode(rec(b"ghost2", 77, b"ACGT", bytes(4 * [31])))
    inner += b"" if resync else b"\xff" * 40
    for l in range(0, 1200):                                       # the B array's data begins at or just behind the boundary
        carrier = rec(b"carrier", 4, bytes(rng.choice(b"ACGT") for _ in range(l)), bytes(rng.randint(0, 40) for _ in range(l)), aux=aux_b(b"XB", inner))
        if at + len(encode(carrier)) - len(inner) >= boundary:
            break
    assert at < boundary <= at + len(encode(carrier)) - len(inner) < boundary + 4
    recs.append(carrier)
    recs += [rand_rec(rng, i + 1 + j, (4, 77, 141), lmax=200) for j in range(60)]
    return recs


def paired(n=500, seed=10):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        name = b"p%d" % i
        for flag in (77, 141):
            l = rng.randint(20, 120)
            out.append(rec(name, flag, bytes(rng.choice(b"ACGT") for _ in range(l)), bytes(rng.randint(2, 40) for _ in range(l)), aux=RG))
    return out


def from_fastq(text):
    lines = text.split(b"\n")[:-1]
    return [rec(lines[i][1:].split(b" ")[0], 4, lines[i + 1], bytes(c - 33 for c in lines[i + 3])) for i in range(0, len(lines), 4)]


GOLDEN = "synth_var"


@functools.lru_cache(maxsize=None)
def good():
    rng = random.Random(12)
    refs = ((b"chr1", 1000000), (b"chr2", 500000), (b"chrM", 16569))
    mapped = [rec(b"m%d" % i, rng.choice((0, 16, 99, 147, 0x100, 0x800 | 16)), bytes(rng.choice(b"ACGT") for _ in range(50)),
                  bytes(rng.randint(2, 40) for _ in range(50)), cigar=(50 << 4,), ref=rng.randint(0, 2), pos=rng.randint(0, 16000), nref=rng.randint(-1, 2),
                  npos=rng.randint(-1, 16000), aux=RG) for i in range(300)]
    small = ubam(300, seed=13)
    g = {
        "a-ubam": Case(ubam()),
        "b-edges": Case(edges()),
        "c-long": Case(long_read()),
        "d-false": Case(embedded(False)),
        "e-resync": Case(embedded(True)),
        "f-header-0": Case(small),
        "f-header-refs": Case(mapped, text=b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n", refs=refs),
        "f-header-big": Case(small, text=b"@CO\t" + b"x" * 99995 + b"\n"),
        "g-empty": Case([], text=b"@HD\tVN:1.6\tSO:unsorted\n"),
        "h-paired": Case(paired()),
        "i-golden": Case(from_fastq(B.golden_text(GOLDEN + ".fastq"))),
        "j-raw": Case(ubam(), raw=True),
        "k-level0": Case(small, level=0),
    }
    return g


GOOD_NAMES = ("a-ubam", "b-edges", "c-long", "d-false", "e-resync", "f-header-0", "f-header-refs", "f-header-big", "g-empty", "h-paired", "i-golden",
              "j-raw", "k-level0")
OPTION_SETS = (dict(), dict(split=1), dict(mate_suffix=0), dict(exclude_flags=0), dict(default_qual=30))


# ---------------------------------------------------------------- refusals
def message(kind, reason, rec_index=0, off=0):
    if kind == "header":
        return "damaged BAM input: header at byte %d: %s" % (off, REASON_TEXT[R[reason]])
    return "damaged BAM input: record %d at byte %d: %s" % (rec_index, off, REASON_TEXT[R[reason]])


def _patched(recs, i, patch, refs=(), cut=None):
    """the stream of recs with patch(bytearray of record i) applied (or the stream cut `cut` bytes into record i);
    (stream, the record's offset)"""
    h = header(refs=refs)
    enc = [bytearray(encode(r)) for r in recs]
    off = len(h) + sum(len(e) for e in enc[:i])
    if cut is not None:
        return h + b"".join(bytes(e) for e in enc[:i]) + bytes(enc[i][:cut]), off
    patch(enc[i])
    return h + b"".join(bytes(e) for e in enc), off


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (file bytes, the inflated stream or None, code, message).  Good records stand in front of the bad one, so that index and offset are not zero."""
    recs = ubam(40, seed=21)
    out = {}

    def put(name, stream, code, msg, wrap=True):
        out[name] = (B.bgzf(stream) if wrap else stream, stream, code, msg)

    def field(fmt, at, value):
        return lambda e: struct.pack_into(fmt, e, at, value)

    good_stream = Case(recs).stream
    put("bad-magic", b"BAM\2" + good_stream[4:], E_ARG, message("header", "MAGIC", off=0))
    put("bad-magic-raw", b"BAX\1" + good_stream[4:], E_ARG, message("header", "MAGIC", off=0), wrap=False)
    put("header-cut-text", header(text=b"@HD\tVN:1.6\n")[:12], E_ARG, message("header", "HDR_SHORT", off=8))
    put("header-cut-nref", header(text=b"@HD\n")[:14], E_ARG, message("header", "HDR_SHORT", off=12))
    put("header-cut-ref", header(refs=((b"chr1", 5), (b"chr2", 6)))[:-3], E_ARG, message("header", "HDR_SHORT", off=12 + 13))
    put("header-l-text", b"BAM\1" + struct.pack("<i", -5) + good_stream[8:], E_ARG, message("header", "L_TEXT", off=4))
    put("header-n-ref", b"BAM\1" + struct.pack("<ii", 0, (1 << 20) + 1) + good_stream[12:], E_ARG, message("header", "N_REF", off=8))
    put("header-l-name", b"BAM\1" + struct.pack("<iii", 0, 1, 0) + good_stream[12:], E_ARG, message("header", "L_NAME", off=12))
    put("header-ref-nul", b"BAM\1" + struct.pack("<iii", 0, 1, 4) + b"chr1" + struct.pack("<i", 9) + good_stream[12:], E_ARG, message("header", "REF_NUL", off=12))
    i = 17
    for name, reason, patch in (
            ("rec-small", "SMALL", field("<I", 0, 31)), ("rec-big", "BIG", field("<I", 0, MAX_BLOCK + 1)), ("rec-past", "PAST", field("<I", 0, 1 << 20)),
            ("rec-name0", "NAME0", field("<B", 12, 0)), ("rec-layout", "LAYOUT", field("<I", 20, 100000)), ("rec-layout-cigar", "LAYOUT", field("<H", 16, 60000)),
            ("rec-name-nul", "NAME", lambda e: e.__setitem__(36 + e[12] - 1, 65)), ("rec-name-inner", "NAME", lambda e: e.__setitem__(37, 0)),
            ("rec-ref", "REF", field("<i", 4, 0)), ("rec-ref-low", "REF", field("<i", 4, -2)), ("rec-next-ref", "REF", field("<i", 24, 7))):
        s, off = _patched(recs, i, patch)
        put(name, s, E_ARG, message("record", reason, i, off))
    s, off = _patched(recs, 39, None, cut=50)
    put("stream-ends-in-record", s, E_ARG, message("record", "PAST", 39, off))
    s, off = _patched(recs, 39, None, cut=2)
    put("stream-ends-in-size", s, E_ARG, message("record", "PAST", 39, off))
    rng = random.Random(22)
    longer = list(recs)
    longer[i] = rec(b"toolong", 4, bytes(rng.choice(b"ACGT") for _ in range(65001)), bytes(rng.randint(2, 40) for _ in range(65001)))
    s, off = _patched(longer, i, lambda e: None)
    put("too-long", s, E_TOO_LONG, message("record", "TOO_LONG", i, off))
    blob = bytearray(B.bgzf(good_stream))
    blob[len(blob) // 2] ^= 0x55                                     # the deflate data or the CRC32 of the first member
    d = B.directory(bytes(blob))
    out["bgzf-damaged"] = (bytes(blob), None, E_ARG, "damaged BGZF input: member 0 at byte 0: ")
    assert len(d) == 2                                             # one member and the EOF member
    return out


def pair_refusals():
    """name -> (Case, message): a paired file with one mate missing; one with another name at pair 17"""
    recs = paired(40)
    short = recs[:30] + recs[31:]
    bad = list(recs)
    bad[35] = bad[35]._replace(name=b"other")
    return {
        "pair-count": (Case(short), "unpaired BAM input: pair 39: no mate (39 READ1 records, 40 READ2 records); collate the file by name first"),
        "pair-name": (Case(bad), "unpaired BAM input: pair 17: the names of READ1 and READ2 differ; collate the file by name first"),
    }
