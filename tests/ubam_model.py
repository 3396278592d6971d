"""A model of the unaligned BAM output (csrc/bfq_ubam.h): "these FASTQ texts as an unaligned BAM", stated in plain Python on
top of tests/bam_model.py's encode() and header() -- the stream, the statistics and every refusal's message --, and the
cases: the smallest shapes at which the kernels can go wrong."""
import functools
import random
from tests import bam_model as M

MAX_READ_LEN = M.MAX_READ_LEN
E_ARG, E_TOO_LONG = M.E_ARG, M.E_TOO_LONG
PIECE = 65280                                                      # bytes of stream per BGZF member
DEFAULT_HEADER = b"@HD\tVN:1.6\tSO:unsorted\n"
FLAGS = (4, 77, 141)                                               # of the records of text 0, 1, 2


class Refused(Exception):
    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code, self.msg = code, msg


def read_msg(k, i, why):
    return "FASTQ to BAM: text %d read %d: %s" % (k, i, why)


W_HDR = "the header line does not begin with '@'"
W_LONG = "name longer than 254 bytes"
W_BYTE = "a byte outside [!-?A-~] in the name"
W_PAIR = "the name differs from that of its mate in text 2"
W_PLUS = "the third line does not begin with '+'"
W_TOO_LONG = "read longer than 65000 bases"
W_QUAL = "a quality byte outside [33, 126]"
MSG_LINES = "FASTQ: number of lines is not a multiple of 4"
MSG_FASTQ = "FASTQ: len(DNA) != len(QS) in a record"
MSG_RG = "FASTQ to BAM: rg_id: empty, longer than 255 bytes, or a byte outside [ -~]"
MSG_LEVEL = "level: 0 (every member stored) or 1 (the compressor)"


def msg_gzip(k):
    return "FASTQ to BAM: text %d is compressed (it begins with 1f 8b): inflate the text first" % k


def msg_pairs(n, m):
    return "FASTQ to BAM: text 1 holds %d reads, text 2 holds %d" % (n, m)


def lines_of(text):
    """the lines of a text, CR before LF stripped; a last line without its LF counts"""
    ls = text.split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in ls]


def name_of(hdr, k, mate_suffix):
    """(why it is refused or None, the name, whether a comment was dropped) of a header line of text k"""
    if not hdr.startswith(b"@"):
        return W_HDR, b"", False
    body = hdr[1:]
    end = min([p for p in (body.find(b" "), body.find(b"\t")) if p >= 0] or [len(body)])
    if end > 254:
        return W_LONG, b"", False
    name = body[:end]
    if mate_suffix and k and len(name) > 2 and name.endswith(b"/%d" % k):
        name = name[:-2]
    if any(c < 33 or c > 126 or c == 64 for c in name):
        return W_BYTE, b"", False
    return None, name, end < len(body)


def members(raw_len):
    return -(-raw_len // PIECE) + 1


def header_of(header_text=None, rg_id=None):
    if header_text is None:
        header_text = DEFAULT_HEADER + (b"@RG\tID:" + rg_id + b"\n" if rg_id is not None else b"")
    return M.header(header_text)


def convert(texts, mate_suffix=1, paired_check=0, header_text=None, rg_id=None, level=1):
    """(the inflated stream, the statistics) of up to three texts (None: absent), or Refused"""
    texts = list(texts) + [None] * (3 - len(texts))
    if rg_id is not None and (not 0 < len(rg_id) <= 255 or any(c < 32 or c > 126 for c in rg_id)):
        raise Refused(E_ARG, MSG_RG)
    if level not in (0, 1):
        raise Refused(E_ARG, MSG_LEVEL)
    for k, t in enumerate(texts):
        if t is not None and t[:2] == b"\x1f\x8b":
            raise Refused(E_ARG, msg_gzip(k))
    ls = []
    for k, t in enumerate(texts):
        ls.append(lines_of(t) if t is not None else [])
        if len(ls[k]) % 4:
            raise Refused(E_ARG, MSG_LINES)
    n = [len(l) // 4 for l in ls]
    if n[1] != n[2] or (texts[1] is None) != (texts[2] is None):
        raise Refused(E_ARG, msg_pairs(n[1], n[2]))
    order = [(1 + (r & 1), r >> 1) for r in range(2 * n[1])] + [(0, i) for i in range(n[0])]
    st = dict(records=len(order), written=n, named=0, comments_dropped=0, unknown_bases=0)
    aux = M.aux_z(b"RG", rg_id) if rg_id is not None else b""
    out = [header_of(header_text, rg_id)]
    for k, i in order:
        hdr, seq, plus, qual = ls[k][4 * i:4 * i + 4]
        why, name, comment = name_of(hdr, k, mate_suffix)
        if why:
            raise Refused(E_ARG, read_msg(k, i, why))
        if paired_check and k == 1:
            w2, mate, _ = name_of(ls[2][4 * i], 2, mate_suffix)
            if w2 or mate != name:
                raise Refused(E_ARG, read_msg(k, i, W_PAIR))
        if not plus.startswith(b"+"):
            raise Refused(E_ARG, read_msg(k, i, W_PLUS))
        if len(seq) != len(qual):
            raise Refused(E_ARG, MSG_FASTQ)
        if len(seq) > MAX_READ_LEN:
            raise Refused(E_TOO_LONG, read_msg(k, i, W_TOO_LONG))
        if any(c < 33 or c > 126 for c in qual):
            raise Refused(E_ARG, read_msg(k, i, W_QUAL))
        if not name:
            name = b"%d" % ((i if k else n[1] + i) + 1)
            st["named"] += 1
        st["comments_dropped"] += 1 if comment else 0
        up = seq.upper()
        known = bytes(c if c in M.SEQ else 78 for c in up)
        st["unknown_bases"] += sum(1 for c in up if c not in M.SEQ)
        out.append(M.encode(M.rec(name, FLAGS[k], known, bytes(c - 33 for c in qual), aux=aux)))
    stream = b"".join(out)
    st["raw_len"], st["members"] = len(stream), members(len(stream))
    return stream, st


def normalised(text, k=0, mate_suffix=1, pairs=0):
    """what bam_to_fastq gives back of a text that went through convert() as text k: the first word of the name (an empty
    one: the read's number, text 0 counting on behind `pairs` pairs), upper-case bases over the alphabet, a bare '+'"""
    ls = lines_of(text)
    out = bytearray()
    for i in range(0, len(ls), 4):
        _, name, _ = name_of(ls[i], k, mate_suffix)
        name = name or b"%d" % ((i // 4 if k else pairs + i // 4) + 1)
        sfx = b"/%d" % k if k and mate_suffix else b""
        seq = bytes(c if c in M.SEQ else 78 for c in ls[i + 1].upper())
        out += b"@" + name + sfx + b"\n" + seq + b"\n+\n" + ls[i + 3] + b"\n"
    return bytes(out)


# ---------------------------------------------------------------- inputs
def fq(reads, eol=b"\n"):
    """a text of (header line without '@', bases, qualities[, the '+' line]) tuples"""
    return b"".join(b"@" + r[0] + eol + r[1] + eol + (r[3] if len(r) > 3 else b"+") + eol + r[2] + eol for r in reads)


def _bases(rng, l, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(l))


def _quals(rng, l, lo=33, hi=73):
    return bytes(rng.randint(lo, hi) for _ in range(l))


EDGE_LENGTHS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def edge_reads(seed=31):
    rng = random.Random(seed)
    out = [(b"e%d" % l, _bases(rng, l), _quals(rng, l)) for l in EDGE_LENGTHS]
    out += [(b"x", _bases(rng, 5), _quals(rng, 5)), (b"n" * 254, _bases(rng, 9), _quals(rng, 9)), (b"n" * 254 + b" tail", b"", b"")]
    out += [(b"", _bases(rng, 4), _quals(rng, 4)), (b"", b"", b""), (b" only a comment", b"AC", b"II"), (b"\tanother", b"A", b"!")]
    out += [(b"blank 1:N:0:ACGT", _bases(rng, 33), _quals(rng, 33)), (b"tab\tBC:Z:AC GT", _bases(rng, 34), _quals(rng, 34), b"+tab")]
    out += [(b"lower", b"acgtnacgtn=", _quals(rng, 11)), (b"iupac", M.SEQ + M.SEQ.lower(), _quals(rng, 32)), (b"junk", b"AC.G-T*Xx@u!~\t ", _quals(rng, 15))]
    out += [(b"qlo", b"ACGTA", b"!!!!!"), (b"qhi", b"ACGTAC", b"~~~~~~"), (b"qmix", _bases(rng, 70), bytes(33 + (j * 37) % 94 for j in range(70)))]
    out += [(b"/1", b"ACG", b"III"), (b"/2", b"ACGT", b"IIII"), (b"a/1", b"AC", b"II"), (b"a/2", b"ACGTA", b"IIIII"), (b"a/1/1", b"A", b"I"), (b"b/3", b"C", b"I")]
    out += [(b"~}|{zyx;:?<=>", b"ACGTT", b"IIIII", b"+~}|{zyx")]
    return out


def lane_reads(seed=32):
    rng = random.Random(seed)
    return [(b"l%d" % l, _bases(rng, l, b"ACGTN"), _quals(rng, l)) for l in range(200)]


def pair_reads(n=300, seed=33):
    rng = random.Random(seed)
    r1, r2 = [], []
    for i in range(n):
        name = b"p%d:%d" % (i, rng.randint(0, 99999))
        l1, l2 = rng.randint(0, 160), rng.randint(0, 160)
        r1.append((name + b"/1 1:N:0", _bases(rng, l1), _quals(rng, l1)))
        r2.append((name + b"/2\t2:N:0", _bases(rng, l2), _quals(rng, l2)))
    return r1, r2


def many_reads(n=5000, l=100, seed=34):
    rng = random.Random(seed)
    return [(b"m%d" % i, _bases(rng, l), _quals(rng, l)) for i in range(n)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (texts[3], opts)"""
    rng = random.Random(35)
    e = edge_reads()
    r1, r2 = pair_reads()
    r0 = [(b"s%d extra" % i, _bases(rng, 10 + i), _quals(rng, 10 + i)) for i in range(7)]
    t1, t2, t0 = fq(r1), fq(r2), fq(r0)
    un1 = [(b"", b, q) for _, b, q in r1[:40]]                      # a run without kept headers: "@" alone
    un2 = [(b"", b, q) for _, b, q in r2[:40]]
    un0 = [(b"", b, q) for _, b, q in r0]
    c = {
        "empty": ([b"", None, None], {}),
        "none": ([None, None, None], {}),
        "edges": ([fq(e), None, None], {}),
        "edges-crlf": ([fq(e, b"\r\n"), None, None], {}),
        "edges-no-final-lf": ([fq(e)[:-1], None, None], {}),
        "edges-rg": ([fq(e), None, None], dict(rg_id=b"grp 1")),
        "edges-as-mates": ([None, fq(e), fq(e)], {}),
        "edges-as-mates-kept": ([None, fq(e), fq(e)], dict(mate_suffix=0)),
        "lanes": ([fq(lane_reads()), None, None], {}),
        "lanes-rg": ([fq(lane_reads()), None, None], dict(rg_id=b"x")),
        "pairs": ([None, t1, t2], {}),
        "pairs-check": ([None, t1, t2], dict(paired_check=1)),
        "pairs+0": ([t0, t1, t2], {}),
        "pairs+0-rg": ([t0, t1, t2], dict(rg_id=b"lane3.A", paired_check=1)),
        "pairs-header": ([t0, t1, t2], dict(header_text=b"@HD\tVN:1.6\tSO:queryname\n@RG\tID:given\tSM:s\n@CO\tkept as it is\n", rg_id=b"given")),
        "pairs-header-empty": ([None, t1, t2], dict(header_text=b"")),
        "pairs-kept": ([None, t1, t2], dict(mate_suffix=0)),
        "unnamed": ([fq(un0), fq(un1), fq(un2)], dict(paired_check=1)),
        "many": ([fq(many_reads()), None, None], {}),
        "long": ([fq([(b"long", _bases(rng, MAX_READ_LEN), _quals(rng, MAX_READ_LEN))]), None, None], {}),
    }
    return c


NAMES = ("empty", "none", "edges", "edges-crlf", "edges-no-final-lf", "edges-rg", "edges-as-mates", "edges-as-mates-kept", "lanes", "lanes-rg", "pairs",
         "pairs-check", "pairs+0", "pairs+0-rg", "pairs-header", "pairs-header-empty", "pairs-kept", "unnamed", "many", "long")


@functools.lru_cache(maxsize=None)
def expect(name):
    """convert() of a case, computed once"""
    texts, opts = cases()[name]
    return convert(texts, **opts)


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (texts[3], opts, code, message).  Good reads stand in front of the bad one, so that its index is not zero."""
    rng = random.Random(36)
    good = [(b"g%d" % i, _bases(rng, 20 + i), _quals(rng, 20 + i)) for i in range(90)]

    def one(i, bad):
        return fq(good[:i] + [bad] + good[i + 1:])

    def bad_read(i, hdr=None, seq=None, qual=None, plus=b"+"):
        g = good[i]
        return (g[0] if hdr is None else hdr, g[1] if seq is None else seq, g[2] if qual is None else qual, plus)

    g = fq(good)
    m1 = fq([(h + b"/1", b, q) for h, b, q in good])
    m2 = fq([(h + b"/2", b, q) for h, b, q in good])
    out = {}

    def put(name, texts, opts, code, msg):
        out[name] = (list(texts) + [None] * (3 - len(texts)), opts, code, msg)

    put("gzip-0", [b"\x1f\x8b\x08\x04" + g], {}, E_ARG, msg_gzip(0))
    put("gzip-2", [None, m1, b"\x1f\x8b"], {}, E_ARG, msg_gzip(2))
    put("lines", [g + b"@x\nAC\n+\n"], {}, E_ARG, MSG_LINES)
    put("lines-one", [b"@"], {}, E_ARG, MSG_LINES)
    put("lines-mate", [None, m1, m2[:-1] + b"\n\n"], {}, E_ARG, MSG_LINES)
    put("only-1", [None, m1, None], {}, E_ARG, msg_pairs(90, 0))
    put("only-2", [g, None, m2], {}, E_ARG, msg_pairs(0, 90))
    put("pair-counts", [None, m1, fq([(h + b"/2", b, q) for h, b, q in good[:89]])], {}, E_ARG, msg_pairs(90, 89))
    put("pair-empty", [None, m1, b""], {}, E_ARG, msg_pairs(90, 0))
    put("no-at", [fq(good[:17]) + b">" + fq(good[17:])[1:]], {}, E_ARG, read_msg(0, 17, W_HDR))
    put("empty-header-line", [fq(good[:5]) + b"\nAC\n+\nII\n"], {}, E_ARG, read_msg(0, 5, W_HDR))
    put("name-255", [one(40, bad_read(40, hdr=b"n" * 255))], {}, E_ARG, read_msg(0, 40, W_LONG))
    put("name-255-comment", [one(41, bad_read(41, hdr=b"n" * 255 + b" c"))], {}, E_ARG, read_msg(0, 41, W_LONG))
    put("name-long-mate", [None, m1, one(3, bad_read(3, hdr=b"q" * 600))], {}, E_ARG, read_msg(2, 3, W_LONG))
    put("name-256-suffix", [None, one(8, bad_read(8, hdr=b"n" * 254 + b"/1")), m2], {}, E_ARG, read_msg(1, 8, W_LONG))
    put("name-byte-at", [one(33, bad_read(33, hdr=b"a@b"))], {}, E_ARG, read_msg(0, 33, W_BYTE))
    put("name-byte-ctl", [one(34, bad_read(34, hdr=b"a\x01b c"))], {}, E_ARG, read_msg(0, 34, W_BYTE))
    put("name-byte-high", [None, m1, one(35, bad_read(35, hdr=b"caf\xc3\xa9/2"))], {}, E_ARG, read_msg(2, 35, W_BYTE))
    put("name-byte-del", [one(36, bad_read(36, hdr=b"x\x7f"))], {}, E_ARG, read_msg(0, 36, W_BYTE))
    put("plus", [one(50, bad_read(50, plus=b"-"))], {}, E_ARG, read_msg(0, 50, W_PLUS))
    put("plus-empty", [one(51, bad_read(51, plus=b""))], {}, E_ARG, read_msg(0, 51, W_PLUS))
    put("lengths", [one(60, bad_read(60, qual=good[60][2] + b"I"))], {}, E_ARG, MSG_FASTQ)
    put("lengths-mate", [None, m1, one(61, bad_read(61, hdr=good[61][0] + b"/2", seq=good[61][1][:-1]))], {}, E_ARG, MSG_FASTQ)
    too = _bases(rng, MAX_READ_LEN + 1)
    put("too-long", [one(70, bad_read(70, seq=too, qual=b"I" * (MAX_READ_LEN + 1)))], {}, E_TOO_LONG, read_msg(0, 70, W_TOO_LONG))
    put("qual-32", [one(80, bad_read(80, qual=good[80][2][:-1] + b" "))], {}, E_ARG, read_msg(0, 80, W_QUAL))
    put("qual-32-first", [one(81, bad_read(81, qual=b" " + good[81][2][1:]))], {}, E_ARG, read_msg(0, 81, W_QUAL))
    put("qual-127", [None, one(82, bad_read(82, hdr=good[82][0] + b"/1", qual=good[82][2][:40] + b"\x7f" + good[82][2][41:])), m2], {}, E_ARG,
        read_msg(1, 82, W_QUAL))
    put("qual-tab", [one(83, bad_read(83, qual=good[83][2][:3] + b"\t" + good[83][2][4:]))], {}, E_ARG, read_msg(0, 83, W_QUAL))
    other = [(h + b"/2", b, q) for h, b, q in good]
    other[44] = (b"other/2", other[44][1], other[44][2])
    other[77] = (b"g77x/2", other[77][1], other[77][2])
    put("pair-names", [None, m1, fq(other)], dict(paired_check=1), E_ARG, read_msg(1, 44, W_PAIR))
    put("pair-names-kept-suffix", [None, m1, m2], dict(paired_check=1, mate_suffix=0), E_ARG, read_msg(1, 0, W_PAIR))
    # of all offending reads, the one whose record comes first in the file: read 9 of text 2 is record 19, read 10 of text 1 record 20,
    # read 0 of text 0 stands behind all pairs
    first = [fq([bad_read(0, qual=b" " * 20)] + good[1:]), one(10, bad_read(10, hdr=b"a@b")), one(9, bad_read(9, plus=b"x"))]
    put("first-of-three", first, {}, E_ARG, read_msg(2, 9, W_PLUS))
    put("first-is-the-pair-name", [None, m1, fq(other[:44] + [bad_read(44, hdr=b"n" * 300)] + other[45:])], dict(paired_check=1), E_ARG, read_msg(1, 44, W_PAIR))
    put("rg-empty", [g], dict(rg_id=b""), E_ARG, MSG_RG)
    put("rg-tab", [g], dict(rg_id=b"a\tb"), E_ARG, MSG_RG)
    put("rg-long", [g], dict(rg_id=b"r" * 256), E_ARG, MSG_RG)
    put("level", [g], dict(level=2), E_ARG, MSG_LEVEL)
    for name, (texts, opts, code, msg) in out.items():             # the model refuses them so
        try:
            convert(texts, **opts)
        except Refused as e:
            assert (e.code, e.msg) == (code, msg), (name, e.msg, msg)
        else:
            raise AssertionError(name)
    return out
