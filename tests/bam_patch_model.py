"""A model of the BAM output (csrc/bfq_bam_patch.h): "this BAM, with the reads of these FASTQ texts in it", stated in plain
Python over the record lists of tests/bam_model.py (imported unchanged) -- where a record's SEQ and QUAL lie follows from the
list, never from parsing the stream; only the bytes stored there are read from it --, the counts and the messages of every
refusal, a byte mask of what a patch may touch, a seeded edit of texts for the round trip, and the cases."""
import functools
import random
from tests import bam_model as M
from tests import bgzf_model as B

PIECES = (256, 1024, 0)
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)
LONG = 20001

NIB = bytearray([15]) * 256                                        # text byte -> nibble, case-insensitive; anything else: N
KNOWN = bytearray(256)
for _i, _ch in enumerate(M.SEQ):
    for _c in {_ch, ord(bytes([_ch]).lower())}:
        NIB[_c], KNOWN[_c] = _i, 1
NIB, KNOWN = bytes(NIB), bytes(KNOWN)
REV_NIB = bytes(M.COMP.index(M.SEQ[n]) for n in NIB)               # ... of the complement: the n with COMP[n] == the letter


class Refused(Exception):
    """a refusal of the definition: code BFQ_E_ARG, str() = the message"""


def lines_of(text):
    """the lines of a text without LF and CR; a last line without its LF counts"""
    ls = text.split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in ls]


def fields(case):
    """per record: (where it starts, where SEQ starts, where QUAL starts) in the stream, from the record list"""
    out, off = [], case.hdr_end
    for r in case.recs:
        seq = off + 36 + len(r.name) + 1 + 4 * len(r.cigar)
        out.append((off, seq, seq + (len(r.seq) + 1) // 2))
        off += len(M.encode(r))
    assert off == len(case.stream)
    return out


def outputs(case, exclude_flags=0x900, split=0, **_):
    """per output k: the indices of its kept records, in file order"""
    outs = [[], [], []]
    for i, r in enumerate(case.recs):
        if not r.flag & exclude_flags:
            outs[M.mate(r.flag) if split else 0].append(i)
    return outs


def text_name(line, suffix):
    """the name a header line states: behind '@' up to the first blank, less the suffix the way in added; None: it has none"""
    if not line.startswith(b"@"):
        return None
    name = line[1:].replace(b"\t", b" ").split(b" ")[0]
    if suffix:
        if not name.endswith(suffix):
            return None
        name = name[:-len(suffix)]
    return name


def _model(case, texts, exclude_flags=0x900, mate_suffix=1, default_qual=1, split=0, check_names=0, **_):
    texts = list(texts) + [None] * (3 - len(texts))
    for k, t in enumerate(texts):
        if t is not None and t[:2] == b"\x1f\x8b":
            raise Refused("BAM patch: text %d is compressed (it begins with 1f 8b): inflate the text first" % k)
    outs, lines = outputs(case, exclude_flags, split), [None] * 3
    for k, t in enumerate(texts):
        if t is None:
            continue
        lines[k] = lines_of(t)
        if len(lines[k]) % 4:
            raise Refused("FASTQ: number of lines is not a multiple of 4")
        if len(lines[k]) // 4 != len(outs[k]):
            raise Refused("BAM patch: text %d holds %d reads, the BAM file holds %d records for it" % (k, len(lines[k]) // 4, len(outs[k])))
    where = fields(case)
    meets = {}                                                     # record -> (k, i)
    for k in range(3):
        if lines[k] is not None:
            meets.update((r, (k, i)) for i, r in enumerate(outs[k]))
    for ri in sorted(meets):                                       # the checking walk, in file order
        k, i = meets[ri]
        r, (off, _, _) = case.recs[ri], where[ri]
        hdr, seq, qual = lines[k][4 * i], lines[k][4 * i + 1], lines[k][4 * i + 3]
        if len(seq) != len(qual):
            raise Refused("FASTQ: len(DNA) != len(QS) in a record")
        if len(seq) != len(r.seq):
            raise Refused("BAM patch: text %d read %d: %d bases, record %d at byte %d holds %d" % (k, i, len(seq), ri, off, len(r.seq)))
        sfx = b"/%d" % M.mate(r.flag) if mate_suffix and M.mate(r.flag) else b""
        if check_names and text_name(hdr, sfx) != r.name:
            raise Refused("BAM patch: text %d read %d: the name differs from that of record %d at byte %d" % (k, i, ri, off))
    s, mask = bytearray(case.stream), bytearray(len(case.stream))
    st = dict(records=len(case.recs), patched=[len(outs[k]) if lines[k] is not None else 0 for k in range(3)], reversed=0, reads_changed=0, bases_changed=0,
              quals_changed=0, unknown_bases=0, kept_high_quals=0, kept_absent=0, raw_len=len(s))
    st["skipped"] = st["records"] - sum(st["patched"])
    for ri in sorted(meets):
        k, i = meets[ri]
        r, (_, so, qo) = case.recs[ri], where[ri]
        l, rev = len(r.seq), bool(r.flag & 0x10)
        seq, qual = lines[k][4 * i + 1], lines[k][4 * i + 3]
        mask[so:qo + l] = b"\1" * (qo + l - so)
        st["reversed"] += rev
        st["unknown_bases"] += l - sum(seq.translate(KNOWN))
        nibs = seq.translate(REV_NIB)[::-1] if rev else seq.translate(NIB)
        old = bytes(s[so:qo])
        oldn = [v for b in old for v in (b >> 4, b & 15)]
        newn = list(nibs) + oldn[l:]                               # the spare nibble keeps its value
        changed = sum(a != b for a, b in zip(oldn, newn))
        st["bases_changed"] += changed
        s[so:qo] = bytes(newn[j] << 4 | newn[j + 1] for j in range(0, len(newn), 2))
        oldq = bytes(s[qo:qo + l])
        absent = l > 0 and oldq[0] == 0xFF
        if absent and qual == bytes([default_qual + 33]) * l:
            st["kept_absent"] += 1
        else:
            newq = bytearray((c - 33) & 0xFF for c in (qual[::-1] if rev else qual))
            for j in range(l):
                if not absent and newq[j] == 93 and oldq[j] > 93:
                    newq[j] = oldq[j]
                    st["kept_high_quals"] += 1
            q = sum(a != b for a, b in zip(oldq, newq))
            st["quals_changed"] += q
            changed += q
            s[qo:qo + l] = newq
        st["reads_changed"] += changed > 0
    return bytes(s), st, bytes(mask)


_CACHE = {}


def _cached(case, texts, opts):
    opts = {k: v for k, v in opts.items() if k != "piece"}         # nothing here depends on the piece
    key = (id(case), tuple(texts), tuple(sorted(opts.items())))
    if key not in _CACHE:
        try:
            _CACHE[key] = _model(case, texts, **opts)
        except Refused as e:
            _CACHE[key] = e
    if isinstance(_CACHE[key], Refused):
        raise _CACHE[key]
    return _CACHE[key]


def patched(case, texts, **opts):
    """(the patched stream, every field of bfq_bam_patch_stats) of a case and up to three texts (bytes; None: absent); raises
    Refused with the message of the definition"""
    s, st, _ = _cached(case, texts, opts)
    ch = M.chain(case, opts.get("piece", 0))[0]
    return s, dict(st, patched=list(st["patched"]), pieces=ch["pieces"], repaired=ch["repaired"])


def mask(case, texts, **opts):
    """1 for every byte of the stream a patch with these texts may change: SEQ and QUAL of the records that meet a read"""
    return _cached(case, texts, opts)[2]


def edited(case, texts, seed, exclude_flags=0x900, split=0, **_):
    """texts with a seeded edit: bases to another letter of ACGTN, qualities to another character of '!'..'~' (never '~' where
    the record holds more than 93).  Returns (texts, the bases that differ, the qualities that differ) -- both counted in
    record space: a read without stored qualities that gets one edited quality has all of them written."""
    rng = random.Random(seed)
    outs, where = outputs(case, exclude_flags, split), fields(case)
    res, nb, nq = [], 0, 0
    for k, t in enumerate(list(texts) + [None] * (3 - len(texts))):
        if t is None:
            res.append(None)
            continue
        ls = [bytearray(l) for l in t.split(b"\n")[:-1]]
        for i, ri in enumerate(outs[k]):
            r, (_, _, qo) = case.recs[ri], where[ri]
            l, rev = len(r.seq), bool(r.flag & 0x10)
            stored = case.stream[qo:qo + l]
            absent, touched = l > 0 and stored[0] == 0xFF, 0
            for p in range(l):
                if rng.random() < 0.08:
                    ls[4 * i + 1][p] = rng.choice([c for c in b"ACGTN" if c != ls[4 * i + 1][p]])
                    nb += 1
                if rng.random() < 0.1:
                    high = not absent and stored[l - 1 - p if rev else p] > 93
                    ls[4 * i + 3][p] = rng.choice([c for c in range(33, 126 if high else 127) if c != ls[4 * i + 3][p]])
                    touched += 1
            nq += l if absent and touched else touched
        res.append(b"".join(bytes(l) + b"\n" for l in ls))
    return res, nb, nq


# ---------------------------------------------------------------- cases
class SpareCase(M.Case):
    """a Case whose odd-length records hold a non-zero spare nibble behind their last base"""
    def __init__(self, recs, **kw):
        super().__init__(recs, **kw)
        s = bytearray(self.stream)
        for i, (r, (_, so, qo)) in enumerate(zip(self.recs, fields(self))):
            if len(r.seq) & 1:
                s[qo - 1] |= 1 + (7 * i + 3) % 15
        self.stream = bytes(s)
        self.blob = B.bgzf(self.stream)


def lane_edges():
    """every length at which a lane or a byte ends, forward and reversed by turns, with tags behind QUAL, absent and high
    qualities, and excluded records between the kept ones"""
    rng = random.Random(41)
    out = []
    for n, l in enumerate(LENGTHS + (LONG,) + LENGTHS):
        flag = (4, 4 | 16, 77, 141 | 16)[n % 4]
        seq = bytes(rng.choice(b"ACGTN") for _ in range(l))
        qual = None if n % 5 == 3 else bytes(rng.choice((0, 2, 40, 93, 94, 200, 254)) if n % 5 == 1 else rng.randint(0, 60) for _ in range(l))
        out.append(M.rec(b"L%d.%d" % (l, n), flag, seq, qual, aux=M.RG + M.aux_b(b"XB", bytes(rng.getrandbits(8) for _ in range(n % 7)))))
        if n % 3 == 0:
            out.append(M.rec(b"x%d" % n, (0x100 | 4, 0x800 | 16)[n % 2], b"ACGTACG", bytes(7 * [20]), aux=M.RG))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    g = dict(M.good())
    g["p-lanes"] = SpareCase(lane_edges())
    g["p-straddle"] = SpareCase(M.ubam(120, seed=43))
    return g


NAMES = M.GOOD_NAMES + ("p-lanes", "p-straddle")


def identity_texts(case, **opts):
    """the texts the way in makes of a case"""
    return M.expect(case, **{k: v for k, v in opts.items() if k in ("exclude_flags", "mate_suffix", "default_qual", "split")})[0]


def variants(texts):
    """name -> the same reads written another way: CRLF line ends; lowercase bases; no final LF"""
    crlf = [None if t is None else t.replace(b"\n", b"\r\n") for t in texts]
    lower = []
    for t in texts:
        if t is None:
            lower.append(None)
            continue
        ls = t.split(b"\n")
        ls[1::4] = [l.lower() for l in ls[1::4]]
        lower.append(b"\n".join(ls))
    return {"crlf": crlf, "lower": lower, "no-final-lf": [None if t is None else t[:-1] for t in texts]}


def non_alphabet(texts):
    """(texts whose sequence lines hold bytes outside the alphabet -- the first base of every read and every seventh behind
    it, as '.', 'x' or '*' by turns --, how many such bytes, the texts the way in gives back: 'N' there)"""
    out, back, n = [], [], 0
    for t in texts:
        if t is None:
            out.append(None)
            back.append(None)
            continue
        ls, lb = t.split(b"\n"), t.split(b"\n")
        for i in range(1, len(ls), 4):
            a, b = bytearray(ls[i]), bytearray(ls[i])
            for p in range(0, len(a), 7):
                a[p], b[p] = b".x*"[(i + p) % 3], ord("N")
                n += 1
            ls[i], lb[i] = bytes(a), bytes(b)
        out.append(b"\n".join(ls))
        back.append(b"\n".join(lb))
    return out, n, back


def refusals():
    """name -> (case, texts, opts, message): built on h-paired with split, so that texts 1 and 2 are in play; the read that
    is refused lies in the middle of a piece at every piece size"""
    c = cases()["h-paired"]
    opts = dict(split=1)
    t = identity_texts(c, **opts)
    out = {}

    def put(name, texts, o=opts):
        try:
            patched(c, texts, **o)
            raise AssertionError(name)
        except Refused as e:
            out[name] = (c, texts, o, str(e))

    l2 = t[2].split(b"\n")
    put("count", [None, t[1], b"\n".join(l2[4:])])
    put("lines", [None, t[1] + b"@x\nA\n", t[2]])
    short = list(l2)
    short[4 * 333 + 1] = short[4 * 333 + 1][:-1]
    short[4 * 333 + 3] = short[4 * 333 + 3][:-1]
    put("length", [None, t[1], b"\n".join(short)])
    two = list(short)
    two[4 * 400 + 1] += b"A"
    two[4 * 400 + 3] += b"I"
    l1 = t[1].split(b"\n")
    l1[4 * 350 + 1] += b"C"
    l1[4 * 350 + 3] += b"I"
    put("length-lowest-of-three", [None, b"\n".join(l1), b"\n".join(two)])
    uneven = list(l2)
    uneven[4 * 100 + 3] += b"I"
    put("dna-qs", [None, t[1], b"\n".join(uneven)])
    named = list(l2)
    named[4 * 250] = b"@other/2"
    put("name", [None, t[1], b"\n".join(named)], dict(opts, check_names=1))
    nosfx = list(l2)
    nosfx[4 * 251] = nosfx[4 * 251][:-2]
    put("name-suffix", [None, t[1], b"\n".join(nosfx)], dict(opts, check_names=1))
    put("gzip", [None, b"\x1f\x8b" + t[1], t[2]])
    return out
