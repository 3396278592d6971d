"""A model of the aux tags in FASTQ header lines, both ways (csrc/bfq_bam.h, csrc/bfq_ubam.h), in plain Python on top of
tests/bam_model.py (records, their encoding, the untagged texts) and tests/ubam_model.py (the untagged stream): the tag-area
parser, the record -> header line text, the header line -> tag bytes, the counts and the messages; and the cases, the
smallest shapes at which the kernels can go wrong."""
import functools
import random
import struct
from tests import bam_model as M
from tests import ubam_model as U

E_ARG = M.E_ARG
INT_FMT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
B_SIZE = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
MSG_TAGS = "malformed tag area"
MAX_FIELD, MAX_TAGS = 1 << 20, 1 << 23


class Malformed(Exception):
    pass


class Refused(Exception):
    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code, self.msg = code, msg


def aux_int(tag, ty, value):
    return tag + ty + struct.pack(INT_FMT[ty], value)


def aux_a(tag, ch):
    return tag + b"A" + ch


def aux_h(tag, value):
    return tag + b"H" + value + b"\0"


def aux_f(tag, value):
    return tag + b"f" + struct.pack("<f", value)


def key_ok(k):
    alpha = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    return len(k) == 2 and k[0] in alpha and k[1] in alpha + b"0123456789"


def printable(b):
    return all(0x20 <= c <= 0x7e for c in b)


# ---------------------------------------------------------------- the way in
def parse_tags(aux):
    """[(key, stored type, value)] of a tag area -- value: bytes (A, Z, H), an int, or None (f, B) --, or Malformed"""
    out, p, n = [], 0, len(aux)
    while p < n:
        if n - p < 3:
            raise Malformed()
        key, ty, v = aux[p:p + 2], aux[p + 2:p + 3], p + 3
        if ty in (b"Z", b"H"):
            e = aux.find(b"\0", v)
            if e < 0:
                raise Malformed()
            out.append((key, ty, aux[v:e]))
            p = e + 1
        elif ty == b"B":
            if n - v < 5 or aux[v:v + 1] not in B_SIZE:
                raise Malformed()
            size = struct.unpack_from("<I", aux, v + 1)[0] * B_SIZE[aux[v:v + 1]]
            if size > n - v - 5:
                raise Malformed()
            out.append((key, ty, None))
            p = v + 5 + size
        elif ty == b"A" or ty == b"f" or ty in INT_FMT:
            w = 1 if ty == b"A" else 4 if ty == b"f" else struct.calcsize(INT_FMT[ty])
            if n - v < w:
                raise Malformed()
            out.append((key, ty, aux[v:v + 1] if ty == b"A" else None if ty == b"f" else struct.unpack_from(INT_FMT[ty], aux, v)[0]))
            p = v + w
        else:
            raise Malformed()
    return out


def tag_text(key, ty, value):
    """the bytes "\\tXX:T:value" of a tag, or None where it cannot be carried"""
    if not key_ok(key) or ty in (b"f", b"B"):
        return None
    if ty in INT_FMT:
        return b"\t" + key + b":i:%d" % value
    return b"\t" + key + b":" + ty + b":" + value if printable(value) else None


def selected(key, tags):
    return not tags or key in tags


def keys_of(tags):
    """"*" -> [] (every tag); "BC,RX" -> [b"BC", b"RX"]"""
    return [] if tags == "*" else [k.encode() for k in tags.split(",")]


def msg_record(i, off, why):
    return "damaged BAM input: record %d at byte %d: %s" % (i, off, why)


def msg_carry(i, off, key, ty):
    word = lambda b: "".join(chr(c) if 0x21 <= c <= 0x7e else "?" for c in b)
    return "BAM tags: record %d at byte %d: tag %s of type %s cannot be carried" % (i, off, word(key), word(ty))


def expected(recs, tags="*", strict=0, hdr_end=12, **opts):
    """(the three texts, the counts of bam_model.expected, the tag counts) of a record list whose fixed fields are fine,
    or Refused with the message that names the first offending record of the file"""
    keys = keys_of(tags)
    exclude, split = opts.get("exclude_flags", 0x900), opts.get("split", 0)
    out = [bytearray(), bytearray(), bytearray()]
    ts = dict(tags_written=0, tags_dropped=0, tag_bytes=0)
    off = hdr_end
    for i, r in enumerate(recs):
        here, off = off, off + len(M.encode(r))
        if r.flag & exclude:
            continue
        try:
            parsed = parse_tags(r.aux)
        except Malformed:
            raise Refused(E_ARG, msg_record(i, here, MSG_TAGS))
        text, lost = b"", None
        for key, ty, value in parsed:
            if not selected(key, keys):
                continue
            t = tag_text(key, ty, value)
            if t is None:
                ts["tags_dropped"] += 1
                lost = lost or (key, ty)
            else:
                ts["tags_written"] += 1
                text += t
        if strict and lost:
            raise Refused(E_ARG, msg_carry(i, here, *lost))
        ts["tag_bytes"] += len(text)
        one = M.expected([r], **opts)[0][M.mate(r.flag) if split else 0]
        cut = one.index(b"\n")                                      # (no name of these cases holds a line feed)
        out[M.mate(r.flag) if split else 0] += one[:cut] + text + one[cut:]
    return [bytes(o) for o in out], M.expected(recs, **opts)[1], ts


# ---------------------------------------------------------------- the way out
def field_tag(field, keys, rg):
    """the stored bytes of the tag a field becomes, or None: dropped"""
    if len(field) < 5 or not key_ok(field[:2]) or field[2:3] != b":" or field[4:5] != b":":
        return None
    key, ty, v = field[:2], field[3:4], field[5:]
    if (rg and key == b"RG") or not selected(key, keys):
        return None
    if ty == b"A":
        return key + b"A" + v if len(v) == 1 and printable(v) else None
    if ty == b"i":
        digits = v[1:] if v.startswith(b"-") else v
        if not 1 <= len(digits) <= 10 or not digits.isdigit():
            return None
        n = int(v)
        if not -(1 << 31) <= n < (1 << 32):
            return None
        ty = (b"C" if n <= 255 else b"S" if n <= 65535 else b"I") if n >= 0 else (b"c" if n >= -128 else b"s" if n >= -32768 else b"i")
        return aux_int(key, ty, n)
    if ty == b"Z":
        return key + b"Z" + v + b"\0" if printable(v) and len(v) <= MAX_FIELD else None
    if ty == b"H":
        hexd = all(c in b"0123456789abcdefABCDEF" for c in v)
        return key + b"H" + v + b"\0" if hexd and len(v) % 2 == 0 and len(v) <= MAX_FIELD else None
    return None


def line_tags(hdr, keys, rg):
    """(the tag bytes, tags written, fields dropped, some byte behind the name did not become a tag) of a header line"""
    body = hdr[1:]
    end = min([p for p in (body.find(b" "), body.find(b"\t")) if p >= 0] or [len(body)])
    rest, junk = body[end:], False
    if rest.startswith(b" "):
        junk = True
        rest = rest[rest.index(b"\t"):] if b"\t" in rest else b""
    out, written, dropped = b"", 0, 0
    for field in rest.split(b"\t")[1:]:
        t = field_tag(field, keys, rg)
        if t is None or len(out) + len(t) > MAX_TAGS:
            dropped += 1
            junk = True
        else:
            out += t
            written += 1
    return out, written, dropped, junk


def convert(texts, tags="*", **opts):
    """(the inflated stream, the statistics, the tag counts) of up to three texts with the fields of their header lines as
    tags: ubam_model.convert's stream with every record's tags put in front of its RG tag"""
    keys = keys_of(tags)
    stream, st = U.convert(texts, **opts)
    texts = list(texts) + [None] * (3 - len(texts))
    ls = [U.lines_of(t) if t is not None else [] for t in texts]
    n = [len(l) // 4 for l in ls]
    order = [(1 + (r & 1), r >> 1) for r in range(2 * n[1])] + [(0, i) for i in range(n[0])]
    rg = opts.get("rg_id")
    tail = 4 + len(rg) if rg is not None else 0
    o = 12 + struct.unpack_from("<i", stream, 4)[0]
    out = [stream[:o]]
    ts = dict(tags_written=0, fields_dropped=0, tag_bytes=0)
    st["comments_dropped"] = 0
    for k, i in order:
        bs = struct.unpack_from("<I", stream, o)[0]
        t, written, dropped, junk = line_tags(ls[k][4 * i], keys, rg is not None)
        body = stream[o + 4:o + 4 + bs]
        out.append(struct.pack("<I", bs + len(t)) + body[:bs - tail] + t + body[bs - tail:])
        ts["tags_written"] += written
        ts["fields_dropped"] += dropped
        ts["tag_bytes"] += len(t)
        st["comments_dropped"] += 1 if junk else 0
        o += 4 + bs
    assert o == len(stream)
    stream = b"".join(out)
    st["raw_len"], st["members"] = len(stream), U.members(len(stream))
    return stream, st, ts


# ---------------------------------------------------------------- inputs: the way in
Z_LENGTHS = (0, 1, 63, 64, 65, 200)
INT_ENDS = ((b"c", -128, 127), (b"C", 0, 255), (b"s", -32768, 32767), (b"S", 0, 65535), (b"i", -(1 << 31), (1 << 31) - 1), (b"I", 0, (1 << 32) - 1))
PIECES = (64, 256, 65536)
BAD_AT = 150                                                       # the record the malformations and the f tag of `strict` stand at


def _read(rng, name, flag, aux, lmax=60, lmin=0):
    l = rng.randint(lmin, lmax)
    return M.rec(name, flag, bytes(rng.choice(b"ACGTN") for _ in range(l)), bytes(rng.randint(0, 60) for _ in range(l)), aux=aux)


@functools.lru_cache(maxsize=None)
def way_in_recs():
    """about 300 records: every shape the definition names, between records that carry RG, RX and BC as a run's do"""
    rng = random.Random(41)
    word = lambda n, abc=b"ACGT": bytes(rng.choice(abc) for _ in range(n))
    out = []
    for i in range(300):
        flag = (77, 141)[i & 1] | (16 if i % 7 == 3 else 0)
        out.append(_read(rng, b"q%d" % (i // 2), flag, M.RG + M.aux_z(b"RX", word(8)) + M.aux_z(b"BC", word(8) + b"-" + word(8))))
    special = [M.aux_z(b"Z%d" % (j % 10), word(l, b"abc xyz~!")) for j, l in enumerate(Z_LENGTHS)]
    special += [aux_int(b"I%d" % j, ty, lo) + aux_int(b"J%d" % j, ty, hi) for j, (ty, lo, hi) in enumerate(INT_ENDS)]
    special += [aux_a(b"XA", b"q") + aux_h(b"XH", b"0aF9") + aux_a(b"XS", b" ") + aux_h(b"XE", b""), b""]
    special += [aux_f(b"XF", 1.5) + M.aux_b(b"XB", bytes(range(9))), M.aux_z(b"ZU", b"a\x01b") + aux_a(b"AU", b"\x7f") + M.aux_z(b"1X", b"badkey") + M.RG]
    special += [M.aux_z(b"ZL", word(200)) + aux_int(b"XI", b"i", -7) + M.aux_z(b"ZM", word(130)) + aux_int(b"XJ", b"S", 300) + M.RG]
    for j, aux in enumerate(special):
        out[16 * j + 5] = out[16 * j + 5]._replace(aux=aux)
    out[40] = _read(rng, b"excluded", 0x100 | 77, b"XZZno-nul")           # excluded: its tag area is not looked at
    out[41] = _read(rng, b"excluded2", 0x800, b"X")
    out[42] = _read(rng, b"single", 4, M.aux_z(b"BC", b"ACGT") + aux_int(b"NM", b"C", 0))
    out[43] = _read(rng, b"rev", 4 | 16, M.aux_z(b"OX", b"ACGTAC"), lmax=9)
    assert out[BAD_AT].aux.startswith(M.RG)
    return tuple(out)


def bad_tag_recs():
    """name -> (records, the reason's words): record BAD_AT of way_in_recs with a tag area that does not parse"""
    good = way_in_recs()
    r = good[BAD_AT]
    one = lambda aux: good[:BAD_AT] + (r._replace(aux=aux),) + good[BAD_AT + 1:]
    return {
        "unknown-type": one(M.RG + b"XXq1234"),
        "value-past-block": one(M.RG + b"XII\x01\x02"),
        "array-past-block": one(M.RG + b"XBBC" + struct.pack("<I", 9) + b"12345678"),
        "z-without-nul": one(M.RG + b"XZZ" + b"x" * 150),
        "short-tag": one(M.RG + b"XZ"),
    }


REPAIRED = ("d-false", "e-resync")                                 # bam_model's cases whose chain walks a piece again, with RG and XB tags


def strict_recs():
    good = way_in_recs()
    return good[:BAD_AT] + (good[BAD_AT]._replace(aux=M.RG + aux_f(b"XF", 2.5) + M.aux_b(b"XB", b"12")),) + good[BAD_AT + 1:]


WAY_IN_OPTS = (dict(tags="*"), dict(tags="BC,RX"), dict(tags="*", split=1), dict(tags="XA,Z1,I4,XF", split=1), dict(tags="*", mate_suffix=0))


def identity_recs(paired):
    """uBAM records whose way in and way out give the stream back: flags 4 / 77 / 141, qualities <= 93, tags of types A /
    Z / H or integers at their smallest width, printable values"""
    rng = random.Random(43)
    word = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))
    ints = (0, 255, 256, 65535, 65536, (1 << 32) - 1, -1, -128, -129, -32768, -32769, -(1 << 31))
    out = []
    for i in range(300):
        n = ints[i % len(ints)]
        ty = (b"C" if n <= 255 else b"S" if n <= 65535 else b"I") if n >= 0 else (b"c" if n >= -128 else b"s" if n >= -32768 else b"i")
        aux = M.aux_z(b"RX", word(8)) + aux_int(b"XN", ty, n) + M.aux_z(b"BC", word(rng.choice((0, 1, 17, 64, 90)))) + aux_a(b"XA", b"k") + aux_h(b"XH", b"00ff") + M.RG
        if i % 11 == 0:
            aux = b""
        flag = (77, 141)[i & 1] if paired else 4
        out.append(_read(rng, b"id%d" % (i // 2 if paired else i), flag, aux, lmin=30)._replace(qual=None))
    return [r._replace(qual=bytes(rng.randint(0, 93) for _ in range(len(r.seq)))) for r in out]


IDENTITY_HEADER = b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:grp1\tSM:s\n"


# ---------------------------------------------------------------- inputs: the way out
INTS = (0, 255, 256, 65535, 65536, 4294967295, -1, -128, -129, -32768, -32769, -2147483648)
INTS_DROPPED = (4294967296, -2147483649)
MALFORMED = (b"XF:f:1.5", b"XB:B:c,1,2", b"XP:i:+5", b"XE:i:", b"XM:i:-", b"XD:i:12a", b"XL:i:00000000001", b"X:Z:a", b"1X:Z:a", b"XX-Z:a", b"XXZa", b"", b"XY:H:abc",
             b"XY:H:zz", b"XQ:A:ab", b"XQ:A:", b"XU:Z:a\x01b", b"XT:z:a", b"XV:i:99999999999")


def _fq(reads, eol=b"\n"):
    return U.fq(reads, eol)


@functools.lru_cache(maxsize=None)
def way_out_cases():
    """name -> (texts[3], opts)"""
    rng = random.Random(44)
    b = lambda l: bytes(rng.choice(b"ACGT") for _ in range(l))
    q = lambda l: bytes(rng.randint(33, 73) for _ in range(l))

    def read(hdr, l=None):
        l = rng.randint(0, 40) if l is None else l
        return (hdr, b(l), q(l))

    ints = b"".join(b"\tI%d:i:%d" % (j % 10, v) for j, v in enumerate(INTS[:10])) + b"\tJ0:i:%d\tJ1:i:%d" % INTS[10:]
    shapes = [read(b"nameonly"), read(b"cmt a comment\tBC:Z:ACGT-AC\tRX:Z:TTTT"), read(b"cmt2 no fields at all"), read(b"cmt3 \tBC:Z:A"),
              read(b"n" * 240 + b"\tAA:Z:" + b"x" * 40 + b"\tBB:i:77"), read(b"emptyz\tBC:Z:\tXH:H:\tXA:A:a\tXS:A: "), read(b"ints" + ints),
              read(b"over" + b"".join(b"\tO%d:i:%d" % (j, v) for j, v in enumerate(INTS_DROPPED)) + b"\tOK:i:-0\tOL:i:007"),
              read(b"bad" + b"".join(b"\t" + f for f in MALFORMED) + b"\tOK:Z:fine"), read(b"rg\tRG:Z:fromtext\tBC:Z:AC"), read(b"\tBC:Z:unnamed"),
              read(b"hex\tXH:H:0aF9\tXZ:Z:" + bytes(range(0x20, 0x7f)).replace(b"\t", b"")), read(b"trailing\tBC:Z:A\t"), read(b"long\tZL:Z:" + b"y" * 700 + b"\tXI:i:5")]
    many = [read(b"m%d\tRX:Z:%s\tBC:Z:%s\tXN:i:%d" % (i, b(8), b(17), rng.choice(INTS))) for i in range(300)]
    r1 = [read(b"p%d/1 c\tBC:Z:%s" % (i, b(6))) for i in range(150)]
    r2 = [read(b"p%d/2\tRX:Z:%s\tXK:i:%d" % (i, b(4), -i)) for i in range(150)]
    c = {
        "none": ([b"", None, None], dict(tags="*")),
        "one": ([_fq(shapes[1:2]), None, None], dict(tags="*")),
        "nine": ([_fq(shapes[:9]), None, None], dict(tags="*")),
        "shapes": ([_fq(shapes), None, None], dict(tags="*")),
        "shapes-crlf": ([_fq(shapes, b"\r\n"), None, None], dict(tags="*")),
        "shapes-rg": ([_fq(shapes), None, None], dict(tags="*", rg_id=b"grp 1")),
        "shapes-list": ([_fq(shapes), None, None], dict(tags="BC,OK,I3,XH")),
        "shapes-no-final-lf": ([_fq(shapes)[:-1], None, None], dict(tags="*")),
        "many": ([_fq(many), None, None], dict(tags="*")),
        "many-list-rg": ([_fq(many), None, None], dict(tags="RX,XN", rg_id=b"x")),
        "pairs": ([None, _fq(r1), _fq(r2)], dict(tags="*", paired_check=1)),
        "pairs+0": ([_fq(shapes), _fq(r1), _fq(r2)], dict(tags="*", rg_id=b"lane3")),
    }
    return c


WAY_OUT_NAMES = ("none", "one", "nine", "shapes", "shapes-crlf", "shapes-rg", "shapes-list", "shapes-no-final-lf", "many", "many-list-rg", "pairs", "pairs+0")


@functools.lru_cache(maxsize=None)
def expect_out(name):
    texts, opts = way_out_cases()[name]
    return convert(texts, **opts)
