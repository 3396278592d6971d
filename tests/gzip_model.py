"""Plain gzip as the tests state it: the inputs (zlib writers with control of level, memLevel, strategy and flushes; hand-made
streams from bgzf_model's bit writer and block builders), and steps 1-3 of csrc/bfq_gzip.h in Python: the member header parse,
the block-start rule with the candidate of every piece, and the chain.  The expected text of every good input is what
zlib.decompressobj(31) gives member by member: nothing here is inflated by this project's code.

The chain is stated from the stream's true block starts (one walk over the bits from the front, walk()): a decoder of the
chain passes true block starts only, so it lands on the first one behind its own start that is the candidate of its piece."""
import functools
import random
import struct
import zlib
import numpy as np
from tests import bgzf_model as B

WIN = 32768
DEF_CHUNK = 131072
CHUNKS = (512, 1024, 4096, 32768, 0)

# reason codes of bfq_gzip.h behind bfq_bgzf.h's, and how bfq_last_error words them
REASONS = B.REASONS + ("RESERVED", "HCRC", "FIELD", "GARBAGE", "TRAILER")
R = {k: i for i, k in enumerate(REASONS)}
REASON_TEXT = B.REASON_TEXT + (
    "reserved gzip flag bits are set", "header CRC16 mismatch", "a header field runs past the end of the input",
    "trailing bytes that are neither zero nor a gzip member", "the input ends inside the member trailer")
# the codes a plain gzip input can meet (the others are BGZF's: its extra field, its member size, its 64 KiB bound)
REACHABLE = ("SHORT", "NOT_GZIP", "PAYLOAD_END", "DIST_FAR", "OVERSUB", "INCOMPLETE", "LITSYM", "DISTSYM", "NO_EOB", "REP_FIRST", "REP_OVER",
             "HLIT_HDIST", "STORED_LEN", "STORED_RUN", "BTYPE", "BADCODE", "LENGTH", "CRC", "RESERVED", "HCRC", "FIELD", "GARBAGE", "TRAILER")


def message(member, off, reason):
    return "damaged gzip input: member %d at byte %d: %s" % (member, off, REASON_TEXT[reason])


# ---------------------------------------------------------------- writers
def gz(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return co.compress(text) + co.flush()


def raw(text, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return co.compress(text) + co.flush()


def member(payload, text=b"", crc=None, isize=None, flg=0, extra=None, name=None, comment=None, hcrc=None, cm=8):
    """One member around a raw deflate payload; FLG follows from the fields given (flg: bits to add), every field can be forced.
    hcrc: True = the right CRC16, an int = that value."""
    f = flg | (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc is not None else 0)
    h = b"\x1f\x8b" + bytes([cm, f]) + b"\0\0\0\0\0\xff"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc is not None:
        h += struct.pack("<H", (zlib.crc32(h) & 0xFFFF) if hcrc is True else hcrc)
    return h + payload + struct.pack("<II", zlib.crc32(text) if crc is None else crc, (len(text) & 0xFFFFFFFF) if isize is None else isize)


def expected(blob):
    """the text by zlib.decompressobj(31), member by member; zero bytes may follow the last member"""
    out = []
    while blob:
        d = zlib.decompressobj(31)
        out.append(d.decompress(blob))
        out.append(d.flush())
        assert d.eof
        blob = d.unused_data
        if not blob.strip(b"\0"):
            break
    return b"".join(out)


# ---------------------------------------------------------------- step 1: the member header (RFC 1952)
def member_header(blob, off):
    """(reason, where the deflate data begins)"""
    p = blob[off:]
    if len(p) < 2:
        return R["SHORT"], 0
    if p[:2] != b"\x1f\x8b":
        return R["NOT_GZIP"], 0
    if len(p) < 10:
        return R["SHORT"], 0
    if p[2] != 8:
        return R["NOT_GZIP"], 0
    flg, q = p[3], 10
    if flg & 0xE0:
        return R["RESERVED"], 0
    if flg & 4:
        if len(p) - q < 2:
            return R["FIELD"], 0
        xlen = p[q] | p[q + 1] << 8
        q += 2
        if len(p) - q < xlen:
            return R["FIELD"], 0
        q += xlen
    for f in (8, 16):
        if flg & f:
            z = p.find(b"\0", q)
            if z < 0:
                return R["FIELD"], 0
            q = z + 1
    if flg & 2:
        if len(p) - q < 2:
            return R["FIELD"], 0
        if zlib.crc32(p[:q]) & 0xFFFF != p[q] | p[q + 1] << 8:
            return R["HCRC"], 0
        q += 2
    return 0, off + q


# ---------------------------------------------------------------- bits
class Reader:
    """bits of a blob by absolute bit offset; past the end they read as zero"""
    def __init__(self, blob):
        a = np.frombuffer(blob + b"\0" * 8, np.uint8).astype(np.uint64)
        n = len(blob)
        w = np.zeros(n + 1, np.uint64)
        for i in range(4):
            w[:n] |= a[i:i + n] << np.uint64(8 * i)
        self.w, self.n, self.bit = w.tolist(), n, 0

    def peek(self, k):                                   # k <= 25
        return (self.w[self.bit >> 3] >> (self.bit & 7)) & ((1 << k) - 1)

    def take(self, k):
        v = self.peek(k)
        self.bit += k
        if self.bit > 8 * self.n:
            raise EOFError
        return v


def table(lens):
    """code lengths -> {(length, code read bit by bit, first bit highest): symbol}, and whether the set is complete"""
    codes = B.canonical(lens)
    left = 1
    for n in range(1, 16):
        left = 2 * left - sum(1 for l in lens if l == n)
    return {(n, c): s for s, (c, n) in codes.items()}, left


def fast_table(lens, bits=10):
    """decode by the next `bits` bits: entry = (symbol, length), None = longer code"""
    t = [None] * (1 << bits)
    long_codes = {}
    for s, (c, n) in B.canonical(lens).items():
        rev = int(format(c, "0%db" % n)[::-1], 2)
        if n <= bits:
            for j in range(rev, 1 << bits, 1 << n):
                t[j] = (s, n)
        else:
            long_codes[(n, c)] = s
    return t, long_codes


def decode(r, t, bits=10):
    fast, slow = t
    e = fast[r.peek(bits)]
    if e is not None:
        r.take(e[1])
        return e[0]
    c = 0
    for n in range(1, 16):
        c = c << 1 | r.take(1)
        if (n, c) in slow:
            return slow[(n, c)]
    raise ValueError("no code")


def read_lengths(r):
    """the code lengths of a dynamic header behind its three type bits; None where the inflate refuses them"""
    hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
    if hlit > 286 or hdist > 30:
        return None
    cl = [0] * 19
    for i in range(hclen):
        cl[B.ORDER[i]] = r.take(3)
    tab, left = table(cl)
    if left != 0:
        return None
    clt = fast_table(cl, 7)
    lens = []
    while len(lens) < hlit + hdist:
        s = decode(r, clt, 7)
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                return None
            lens += [lens[-1]] * (3 + r.take(2))
        elif s == 17:
            lens += [0] * (3 + r.take(3))
        else:
            lens += [0] * (11 + r.take(7))
    if len(lens) > hlit + hdist:
        return None
    return lens[:hlit], lens[hlit:]


def is_start(r, bit):
    """step 2's rule at a bit offset: BFINAL 0, BTYPE 2 and a header that passes every check of the inflate"""
    r.bit = bit
    try:
        if r.take(3) != 4:
            return False
        got = read_lengths(r)
    except (EOFError, ValueError):
        return False
    if got is None:
        return False
    ll, dl = got
    if ll[256] == 0 or table(ll)[1] != 0:
        return False
    left = table(dl)[1]
    used = [l for l in dl if l]
    return left == 0 or not used or used == [1]


def cheap_offsets(blob):
    """the bit offsets that pass the cheap tests, in order: three type bits, HLIT, HDIST, a complete code-length code"""
    n = len(blob)
    a = np.frombuffer(blob + b"\0" * 16, np.uint8).astype(np.uint64)
    w = [np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)]          # 64 bits from byte i, i + 2, i + 3
    for k, o in enumerate((0, 2, 3)):
        for i in range(8):
            w[k] |= a[o + i:o + i + n] << np.uint64(8 * i)
    out = []
    for o in range(8):
        v = w[0] >> np.uint64(o)
        ok = ((v & np.uint64(7)) == 4) & (((v >> np.uint64(3)) & np.uint64(31)) <= 29) & (((v >> np.uint64(8)) & np.uint64(31)) <= 29)
        idx = np.nonzero(ok)[0]
        hclen = ((v[idx] >> np.uint64(13)) & np.uint64(15)) + np.uint64(4)
        c = (w[1][idx] >> np.uint64(o + 1)) if o < 7 else w[2][idx]
        kraft = np.zeros(len(idx), np.uint64)
        for i in range(19):
            l = (c >> np.uint64(3 * i)) & np.uint64(7)
            kraft += np.where((np.uint64(i) < hclen) & (l > 0), np.uint64(128) >> l, np.uint64(0))
        fits = idx.astype(np.uint64) * np.uint64(8) + np.uint64(o + 17) + np.uint64(3) * hclen <= np.uint64(8 * n)
        out.append(idx[(kraft == 128) & fits] * 8 + o)
    return np.sort(np.concatenate(out))


@functools.lru_cache(None)
def rule_offsets(blob):
    """every bit offset of the blob where the rule holds, in order: the cheap tests, then the full parse for the survivors"""
    r = Reader(blob)
    return tuple(bit for bit in cheap_offsets(blob).tolist() if is_start(r, bit))


def candidates(blob, chunk):
    """step 2: per piece the first bit offset inside it where the rule holds (None: nowhere; piece 0 has none)"""
    cand = [None] * max(1, -(-len(blob) // chunk))
    for bit in rule_offsets(blob):
        k = bit // (8 * chunk)
        if k and cand[k] is None:
            cand[k] = bit
    return cand


# ---------------------------------------------------------------- step 3: the stream's block starts, the chain
FIXED = (fast_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), fast_table([5] * 30, 8))


@functools.lru_cache(None)
def walk(blob):
    """One pass over a good input from the front: (bit offsets of all block starts, members, bit offset where the stream ends)."""
    r = Reader(blob)
    starts, members, off = [], 0, 0
    while True:
        reason, data = member_header(blob, off)
        assert reason == 0
        r.bit = data * 8
        while True:
            starts.append(r.bit)
            last, typ = r.take(1), r.take(2)
            if typ == 0:
                r.bit = (r.bit + 7) & ~7
                n = r.take(16)
                r.take(16)
                r.bit += 8 * n
            else:
                if typ == 1:
                    lt, dt = FIXED
                else:
                    ll, dl = read_lengths(r)
                    lt, dt = fast_table(ll), fast_table(dl, 8)
                while True:
                    s = decode(r, lt)
                    if s < 256:
                        continue
                    if s == 256:
                        break
                    if 265 <= s < 285:
                        r.take((s - 261) >> 2)
                    d = decode(r, dt, 8)
                    if d >= 4:
                        r.take((d >> 1) - 1)
            if last:
                break
        members += 1
        off = ((r.bit + 7) >> 3) + 8
        if off >= len(blob) or blob[off] != 0x1F:
            return starts, members, 8 * len(blob)


def chain(blob, chunk):
    """bfq_gzip_stats as a dict, and the bit offsets the chain's decoders start at"""
    chunk = chunk or DEF_CHUNK
    cand = candidates(blob, chunk)
    starts, members, end = walk(blob)
    on = [starts[0]]
    for s in starts[1:]:
        k = s // (8 * chunk)
        if 0 < k < len(cand) and cand[k] == s:
            on.append(s)
    started = 1 + sum(c is not None for c in cand)
    off = [c for c in cand if c is not None and c not in on[1:]]
    return dict(members=members, pieces=len(cand), decoders=started, chain=len(on), skipped=len(off), discarded=started - len(on)), on, off


# ---------------------------------------------------------------- good inputs
@functools.lru_cache(None)
def big_text():
    return B.expected(B.big())[:3_000_000]


DYN_L, DYN_D = [8] * 226 + [9] * 60, [4, 4] + [5] * 28      # complete sets with every length and distance symbol


def far_reach(head_len):
    """A member: one stored block of seeded random bytes, then a dynamic block whose first token is a match of length 258 at
    distance 32 768.  head_len = 32 768: it reaches the oldest byte of the window; less: before the member's first byte."""
    rng = random.Random(3)
    head = bytes(rng.getrandbits(8) for _ in range(head_len))
    w = B.Bits()
    B.stored(w, 0, head)
    at = 8 * len(w.out)
    b = B.dynamic(w, 0, DYN_L, DYN_D)
    b.match(258, 32768); b.lit(b"xyz"); b.end()
    b = B.fixed(w, 1); b.lit(b"end\n"); b.end()
    text = head + head[:258] + b"xyz" + b"end\n" if head_len >= 32768 else b""
    return member(w.bytes(), text), 80 + at              # (the plain header is 10 bytes)


def false_start():
    """A member whose third stored block carries, behind 132 070 bytes of 0xFF in all, a complete valid dynamic block header:
    a later piece's candidate at every chunk up to the default, and never a block of the stream."""
    h = B.Bits()
    b = B.dynamic(h, 0, DYN_L, DYN_D)
    b.lit(b"not a block"); b.end()
    fill = b"\xff" * 65535
    payload = b"\xff" * 1000 + h.bytes() + b"\xff" * 100
    w = B.Bits()
    B.stored(w, 0, fill)
    B.stored(w, 0, fill)
    B.stored(w, 0, payload)
    b = B.fixed(w, 1); b.lit(b"tail\n"); b.end()
    return member(w.bytes(), fill + fill + payload + b"tail\n"), 8 * (10 + 2 * (5 + 65535) + 5 + 1000)


def three_members(first_total):
    """text member | empty member | member with FEXTRA + FNAME + FCOMMENT + FHCRC | zero padding.  first_total: the first
    member is padded (FEXTRA) to that many bytes, 0: as it comes."""
    t1, t3 = B.synth_var()[:150000], B.synth_var()[150000:]
    p1 = raw(t1, 6, 1)
    extra = None
    if first_total:
        pad = first_total - (10 + 2 + len(p1) + 8)
        assert 4 <= pad < 65536
        extra = b"PD" + struct.pack("<H", pad - 4) + b"\0" * (pad - 4)
    m1 = member(p1, t1, extra=extra)
    assert not first_total or len(m1) == first_total
    m2 = member(raw(b""), b"")
    m3 = member(raw(t3, 6, 1), t3, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"a comment", hcrc=True)
    return m1 + m2 + m3 + b"\0" * 700


def flushed(text):
    co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
    out = []
    for at in range(0, len(text), 5000):
        out.append(co.compress(text[at:at + 5000]))
        out.append(co.flush(zlib.Z_FULL_FLUSH if (at + 5000) % 20000 == 0 else zlib.Z_SYNC_FLUSH))
    out.append(co.flush())
    return b"".join(out)


GOOD_NAMES = ("a-l1-m1", "a-l1-m8", "a-l6-m1", "a-l6-m8", "a-l9-m1", "a-l9-m8", "b-huff", "b-rle", "b-fixed", "b-l0", "c-random", "d-big-m1",
              "d-big-m8", "e-repeat", "f-inside", "f-boundary", "g-flush", "h-reach", "i-false", "j-bgzf")


@functools.lru_cache(None)
def good():
    """name -> gzip bytes: the issue's inputs (a) to (j)"""
    text = B.synth_var()
    out = {}
    for level in (1, 6, 9):
        for mem in (1, 8):
            out["a-l%d-m%d" % (level, mem)] = gz(text, level, mem)
    out["b-huff"] = gz(text, 6, 8, zlib.Z_HUFFMAN_ONLY)
    out["b-rle"] = gz(text, 6, 8, zlib.Z_RLE)
    out["b-fixed"] = gz(text, 6, 8, zlib.Z_FIXED)
    out["b-l0"] = gz(text, 0)
    rng = random.Random(5)
    out["c-random"] = gz(bytes(rng.getrandbits(8) for _ in range(200000)), 6)
    out["d-big-m1"] = gz(big_text(), 6, 1)
    out["d-big-m8"] = gz(big_text(), 6, 8)
    # (e) a random string of quality characters, not of bytes: zlib leaves random bytes in stored blocks, which start no
    # decoder, and the 20 pieces under them would leave a chain of 16 at chunk 1024; this one is coded in dynamic blocks
    # from its first byte, and the 99 repeats are matches at distance 20 000 all the same
    rng = random.Random(9)
    out["e-repeat"] = gz(bytes(rng.choices(bytes(range(33, 74)), k=20000)) * 100, 6, 1)
    out["f-inside"] = three_members(0)
    out["f-boundary"] = three_members(98304)
    out["g-flush"] = flushed(text)
    out["h-reach"] = far_reach(32768)[0]
    out["i-false"] = false_start()[0]
    out["j-bgzf"] = B.bgzf(text, 65280, 6)
    assert tuple(out) == GOOD_NAMES
    return out


# ---------------------------------------------------------------- refusals
def refusals():
    """name -> (bytes, reason, member index, byte offset of that member's header)"""
    rec = b"@r\nACGT\n+\nIIII\n"
    g = gz(rec)
    G = len(g)
    out = {}
    _, _, bare = B.refusals()

    def payload(name):                                   # the deflate data and the trailer of a BGZF refusal case
        return bare[name][18:-8], bare[name][-8:]

    # deflate data that the inflate refuses where it stands: member 1 behind a good one
    for name, reason in (("dist-far", "DIST_FAR"), ("oversub", "OVERSUB"), ("incomplete", "INCOMPLETE"), ("incomplete-dist", "INCOMPLETE"),
                         ("litsym-286", "LITSYM"), ("litsym-287", "LITSYM"), ("distsym-30", "DISTSYM"), ("distsym-31", "DISTSYM"),
                         ("no-eob", "NO_EOB"), ("rep-first", "REP_FIRST"), ("rep-over", "REP_OVER"), ("hlit-287", "HLIT_HDIST"),
                         ("hdist-31", "HLIT_HDIST"), ("stored-len", "STORED_LEN"), ("stored-run", "STORED_RUN"), ("btype-3", "BTYPE"),
                         ("badcode", "BADCODE"), ("wrong-isize", "LENGTH"), ("crc-only", "CRC")):
        pay, trailer = payload(name)
        out[name] = (g + b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + pay + trailer, R[reason], 1, G)   # ("dist-far": before the SECOND member's start)
    pay, trailer = payload("dist-far")
    out["dist-far-piece0"] = (b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + pay + trailer, R["DIST_FAR"], 0, 0)
    out["dist-far-later-piece"] = (far_reach(20000)[0], R["DIST_FAR"], 0, 0)
    out["dist-far-later-piece-member1"] = (g + far_reach(20000)[0], R["DIST_FAR"], 1, G)
    # truncation: in a header, in a header field, in deflate data, in a trailer
    big = gz(B.synth_var()[:20000], 6, 1)
    out["empty"] = (b"", R["SHORT"], 0, 0)
    out["short-header"] = (g + g[:5], R["SHORT"], 1, G)
    out["short-extra"] = (g + member(raw(rec), rec, extra=b"XY\x03\x00abc")[:14], R["FIELD"], 1, G)
    out["short-name"] = (g + member(raw(rec), rec, name=b"reads.fq")[:15], R["FIELD"], 1, G)
    out["short-hcrc"] = (g + member(raw(rec), rec, hcrc=True)[:11], R["FIELD"], 1, G)
    out["short-data"] = (g + big[:5000], R["PAYLOAD_END"], 1, G)
    out["short-data-later-piece"] = (big[:-2000], R["PAYLOAD_END"], 0, 0)
    out["short-trailer"] = (g + g[:-3], R["TRAILER"], 1, G)
    # headers
    out["not-gzip"] = (rec, R["NOT_GZIP"], 0, 0)
    out["not-deflate"] = (g + member(raw(rec), rec, cm=7), R["NOT_GZIP"], 1, G)
    out["reserved"] = (g + member(raw(rec), rec, flg=0x20), R["RESERVED"], 1, G)
    out["hcrc"] = (g + member(raw(rec), rec, name=b"x", hcrc=0x1234), R["HCRC"], 1, G)
    out["garbage"] = (g + b"junk", R["GARBAGE"], 1, G)
    out["garbage-behind-zeros"] = (g + b"\0" * 100 + b"\x01", R["GARBAGE"], 1, G)
    # CRC32 and ISIZE: named only where no structure is broken, lowest member first
    flip = lambda m: m[:-8] + bytes([m[-8] ^ 1]) + m[-7:]
    out["crc-member0"] = (flip(g) + g, R["CRC"], 0, 0)
    out["crc-member1"] = (g + flip(g), R["CRC"], 1, G)
    out["crc-both"] = (flip(big) + flip(g), R["CRC"], 0, 0)
    out["isize"] = (g[:-4] + struct.pack("<I", len(rec) + 1), R["LENGTH"], 0, 0)
    out["crc0-then-btype1"] = (flip(g) + out["btype-3"][0][G:], R["BTYPE"], 1, G)
    return out
