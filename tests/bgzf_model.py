"""BGZF as the tests state it: a writer over zlib (raw deflate, wbits -15) with control of chunk size, level, strategy and a
mid-member full flush; a bit writer for hand-made deflate blocks; the case lists (matrix, extremes, crafted blocks, refusals)
shared by the host program's test and the GPU test.  A BGZF file is a valid multi-member gzip: the expected text of every
good case is what gzip.decompress gives."""
import gzip
import os
import random
import struct
import zlib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # htslib's 28 bytes

# reason codes of bfq_bgzf.h, in its order
REASONS = ("OK", "SHORT", "NOT_GZIP", "FLG", "SUBFIELD", "NO_BC", "TOTAL", "ISIZE", "PAYLOAD_END", "OUT_OVER", "DIST_FAR", "OVERSUB",
           "INCOMPLETE", "LITSYM", "DISTSYM", "NO_EOB", "REP_FIRST", "REP_OVER", "HLIT_HDIST", "STORED_LEN", "STORED_RUN", "BTYPE",
           "BADCODE", "LENGTH", "CRC", "TRAILING")
R = {k: i for i, k in enumerate(REASONS)}
# ... and how bfq_last_error words them
REASON_TEXT = (
    "ok", "the input ends inside the member header", "no gzip member here (1f 8b 08 expected)",
    "gzip flags are not 4 (extra field only): not a BGZF member", "an extra subfield runs past XLEN", "no BC subfield: not a BGZF member",
    "the member size in the BC subfield is too small or runs past the end of the input", "ISIZE above 65536",
    "the deflate data runs past the payload", "the deflate data produces more than ISIZE bytes",
    "a match distance reaches before the start of the member", "over-subscribed code lengths", "incomplete code lengths",
    "literal/length symbol 286 or 287", "distance symbol 30 or 31", "no end-of-block code", "repeat code with no length before it",
    "a repeat runs past HLIT + HDIST", "HLIT above 286 or HDIST above 30", "stored block: LEN is not the complement of NLEN",
    "stored block: the run goes past the payload", "block type 3", "bits that are no code of the block's code set",
    "the inflated length differs from ISIZE", "CRC32 mismatch", "payload bytes left over after the final block")


def member(payload, text=None, crc=None, isize=None, extra=None, flg=4, bsize=None):
    """One member around a raw deflate payload; every field can be forced."""
    if extra is None:
        extra = b"BC\x02\x00\x00\x00"
    total = 12 + len(extra) + len(payload) + 8
    if b"BC\x02\x00\x00\x00" in extra:
        at = extra.index(b"BC\x02\x00\x00\x00")
        extra = extra[:at + 4] + struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xFFFF) + extra[at + 6:]
    if crc is None:
        crc = zlib.crc32(text)
    if isize is None:
        isize = len(text)
    return b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + struct.pack("<H", len(extra)) + extra + payload + struct.pack("<II", crc, isize)


def deflate_raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is not None and flush_at < len(data):
        return co.compress(data[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[flush_at:]) + co.flush()
    return co.compress(data) + co.flush()


def bgzf(text, chunk=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, eof=True):
    out = []
    for at in range(0, len(text), chunk):
        piece = text[at:at + chunk]
        out.append(member(deflate_raw(piece, level, strategy, flush_at), piece))
    if eof:
        out.append(EOF)
    return b"".join(out)


def directory(blob):
    """(in_off, out_off, in_len, out_len) of every member, by the BC subfield of a well-formed file (BC first)."""
    d, at, raw = [], 0, 0
    while at < len(blob):
        total = struct.unpack_from("<H", blob, at + 16)[0] + 1
        isize = struct.unpack_from("<I", blob, at + total - 4)[0]
        d.append((at, raw, total, isize))
        at += total
        raw += isize
    return d


# ---------------------------------------------------------------- hand-made deflate
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                 # n bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                # a Huffman code of n bits, most significant first
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code of every symbol with a non-zero length (RFC 1951 3.2.2)"""
    codes, code = {}, 0
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = (code, n)
                code += 1
        code <<= 1
    return codes


FIXED_L = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = {s: (s, 5) for s in range(32)}
ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_LENS = [4] * 13 + [5] * 6                               # a complete code over all 19 code-length symbols
CL = canonical(CL_LENS)


def len_sym(n):
    if n == 258:
        return 285, 0, 0
    i = n - 3
    if i < 8:
        return 257 + i, 0, 0
    for idx in range(8, 28):
        ext = (idx >> 2) - 1
        base = 3 + ((4 + (idx & 3)) << ext)
        if base <= n < base + (1 << ext):
            return 257 + idx, n - base, ext


def dist_sym(d):
    if d <= 4:
        return d - 1, 0, 0
    for s in range(4, 30):
        ext = (s >> 1) - 1
        base = 1 + ((2 + (s & 1)) << ext)
        if base <= d < base + (1 << ext):
            return s, d - base, ext


class Block:
    """Tokens into a Bits: lit(b), match(len, dist), sym(s) (any literal/length symbol, raw), end()."""
    def __init__(self, w, lc, dc):
        self.w, self.lc, self.dc = w, lc, dc

    def sym(self, s):
        self.w.code(*self.lc[s])

    def lit(self, data):
        for b in data:
            self.sym(b)

    def match(self, n, d, dsym=None):
        s, x, e = len_sym(n)
        self.sym(s)
        self.w.put(x, e)
        s, x, e = dist_sym(d) if dsym is None else (dsym, 0, 0)
        self.w.code(*self.dc[s])
        self.w.put(x, e)

    def end(self):
        self.sym(256)


def fixed(w, final):
    w.put(final, 1)
    w.put(1, 2)
    return Block(w, FIXED_L, FIXED_D)


def stored(w, final, data, nlen=None, ln=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    ln = len(data) if ln is None else ln
    w.out += struct.pack("<HH", ln, (~ln & 0xFFFF) if nlen is None else nlen)
    w.out += data


def dynamic(w, final, llens, dlens, ops=None, hlit=None, hdist=None):
    """Header of a dynamic block.  ops: the code-length symbols to send, an int 0..15 or (16 | 17 | 18, extra); default: the
    lengths one by one."""
    w.put(final, 1)
    w.put(2, 2)
    w.put((len(llens) if hlit is None else hlit) - 257, 5)
    w.put((len(dlens) if hdist is None else hdist) - 1, 5)
    w.put(19 - 4, 4)
    for s in ORDER:
        w.put(CL_LENS[s], 3)
    for op in (list(llens) + list(dlens) if ops is None else ops):
        s, x = op if isinstance(op, tuple) else (op, 0)
        w.code(*CL[s])
        w.put(x, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return Block(w, canonical(llens), canonical(dlens))


def lens_of(pairs, n):
    l = [0] * n
    for s, v in pairs.items():
        l[s] = v
    return l


def one(payload_bits, text, **kw):
    return member(payload_bits.bytes() if isinstance(payload_bits, Bits) else payload_bits, text, **kw)


# ---------------------------------------------------------------- the cases
def golden_text(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def synth_var():
    return golden_text("synth_var.fastq")


WRITERS = {
    "stored": dict(level=0), "l1": dict(level=1), "l9": dict(level=9), "fixed": dict(level=6, strategy=zlib.Z_FIXED),
    "rle": dict(level=6, strategy=zlib.Z_RLE), "huff": dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY), "flush": dict(level=6, flush_at=1000),
}


def matrix():
    """name -> BGZF bytes: texts x chunks x writers"""
    out = {}
    texts = {"example": golden_text("example.fastq"), "synth": synth_var()}
    for tn, text in texts.items():
        for chunk in (65280, 4096, 700, 1):
            t = text[:3000] if chunk == 1 else text
            for wn, kw in WRITERS.items():
                out["%s-c%d-%s" % (tn, chunk, wn)] = bgzf(t, chunk, **kw)
    return out


def extremes():
    rng = random.Random(7)
    out = {"eof-only": EOF}
    t = bytes(rng.choice(b"ACGT") for _ in range(65536))
    out["isize-65536"] = bgzf(t, 65536)
    t = bytes(rng.getrandbits(8) for _ in range(65280))
    out["random-65280"] = bgzf(t, 65280)
    out["A-65536"] = bgzf(b"A" * 65536, 65536)
    out["no-eof"] = bgzf(golden_text("example.fastq"), 5000, eof=False)
    return out


def big():
    rng = random.Random(11)
    t = bytes(rng.choices(b"ACGT", k=20_000_000))
    return bgzf(t, 65280, level=1)


def crafted():
    out = {}
    w = Bits()
    b = fixed(w, 0); b.lit(b"AB"); b.end()
    stored(w, 0, b"")
    b = fixed(w, 1); b.lit(b"CD"); b.end()
    out["stored-len0-between"] = one(w, b"ABCD")

    w = Bits()
    b = dynamic(w, 1, lens_of({65: 1, 256: 2, 257: 2}, 258), [1])
    b.lit(b"A"); b.match(3, 1); b.end()
    out["single-dist-code"] = one(w, b"AAAA")

    w = Bits()
    b = dynamic(w, 1, [8] * 226 + [9] * 60, [4, 4] + [5] * 28)
    b.lit(b"hello, "); b.match(7, 7); b.lit(b"\xff\x00"); b.match(258, 1); b.end()
    out["hlit286-hdist30"] = one(w, b"hello, hello, \xff" + b"\x00" * 259)

    # 17 (zero run) across the boundary: literal lengths 258, 259 and distance lengths 0, 1 are one run of four
    w = Bits()
    ll, dl = lens_of({65: 1, 256: 2, 257: 2}, 260), [0, 0, 1, 1]
    ops = [0] * 65 + [1] + [0] * 190 + [2, 2, (17, 1), 1, 1]
    b = dynamic(w, 1, ll, dl, ops)
    b.lit(b"AAA"); b.match(3, 3); b.end()
    out["rep17-straddles"] = one(w, b"AAAAAA")
    # 16 (copy run): the length of 257 is copied over 258 and the eight distance lengths
    w = Bits()
    ll, dl = lens_of({65: 1, 256: 2, 257: 3, 258: 3}, 259), [3] * 8
    ops = [0] * 65 + [1] + [0] * 190 + [2, 3, (16, 3), (16, 0)]
    b = dynamic(w, 1, ll, dl, ops)
    b.lit(b"AAAAA"); b.match(4, 5); b.end()
    out["rep16-straddles"] = one(w, b"AAAAAAAAA")

    rng = random.Random(3)
    head = bytes(rng.getrandbits(8) for _ in range(32768))
    w = Bits()
    stored(w, 0, head)
    b = fixed(w, 1); b.match(258, 32768); b.end()
    out["len258-dist32768"] = one(w, head + head[:258])

    w = Bits()
    b = fixed(w, 1); b.lit(b"A"); b.match(3, 1); b.end()
    out["dist1-at-byte1"] = one(w, b"AAAA")

    w = Bits()
    b = fixed(w, 1); b.lit(b"\xc8" * 6); b.end()
    assert w.n == 0 and len(w.out) == 8                     # 3 + 6 * 9 + 7 bits: the end-of-block code fills the last byte
    out["ends-on-bit7"] = one(w, b"\xc8" * 6)
    return out


def refusals():
    """name -> (bytes, reason, member index, byte offset of that member).  A good member stands in front of most of them, so
    that index and offset are not zero."""
    good = member(deflate_raw(b"@r\nACGT\n+\nIIII\n"), b"@r\nACGT\n+\nIIII\n")
    G = len(good)
    out, bare = {}, {}

    def add(name, bad, reason, alone=False):
        bare[name] = bad
        out[name] = (bad if alone else good + bad + EOF, R[reason], 0 if alone else 1, 0 if alone else G)

    ok = deflate_raw(b"0123456789")
    out["short-header"] = (good + good[:10], R["SHORT"], 1, G)
    out["not-gzip"] = (good + b"@r\nACGT\n+\nIIII\n", R["NOT_GZIP"], 1, G)
    add("flg", member(ok, b"0123456789", flg=0), "FLG")
    add("subfield", member(ok, b"0123456789", extra=b"BC\x02\x00\x00\x00XY\x09\x00ab"), "SUBFIELD")
    add("no-bc", member(ok, b"0123456789", extra=b"XY\x02\x00ab"), "NO_BC")
    add("total-small", member(ok, b"0123456789", bsize=20), "TOTAL")
    out["truncated-mid-member"] = (good + member(ok, b"0123456789")[:-9], R["TOTAL"], 1, G)
    add("isize", member(ok, b"0123456789", isize=65537), "ISIZE")

    w = Bits(); b = fixed(w, 1); b.lit(b"A")
    add("payload-end", one(w, b"A"), "PAYLOAD_END")
    add("out-over", member(ok, b"01234", isize=5), "OUT_OVER")
    w = Bits(); b = fixed(w, 1); b.lit(b"A"); b.match(3, 2); b.end()
    add("dist-far", one(w, b"AAAA"), "DIST_FAR")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 66: 1, 256: 1}, 257), [1, 1]); w.put(0, 16)
    add("oversub", one(w, b""), "OVERSUB")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 2, 256: 2}, 257), [1, 1]); w.put(0, 16)
    add("incomplete", one(w, b""), "INCOMPLETE")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 1}, 257), [2, 2]); w.put(0, 16)
    add("incomplete-dist", one(w, b""), "INCOMPLETE")
    w = Bits(); b = fixed(w, 1); b.lit(b"A"); b.sym(286); b.end()
    add("litsym-286", one(w, b"A"), "LITSYM")
    w = Bits(); b = fixed(w, 1); b.lit(b"A"); b.sym(287); b.end()
    add("litsym-287", one(w, b"A"), "LITSYM")
    w = Bits(); b = fixed(w, 1); b.lit(b"A"); b.match(3, 1, dsym=30); b.end()
    add("distsym-30", one(w, b"AAAA"), "DISTSYM")
    w = Bits(); b = fixed(w, 1); b.lit(b"A"); b.match(3, 1, dsym=31); b.end()
    add("distsym-31", one(w, b"AAAA"), "DISTSYM")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 66: 1}, 257), [1, 1]); w.put(0, 16)
    add("no-eob", one(w, b""), "NO_EOB")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 1}, 257), [1, 1], ops=[(16, 0)] + [0] * 300); w.put(0, 16)
    add("rep-first", one(w, b""), "REP_FIRST")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 1}, 257), [1, 1], ops=[0] * 65 + [1] + [0] * 190 + [1, 1, (18, 0)]); w.put(0, 16)
    add("rep-over", one(w, b""), "REP_OVER")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 1}, 257), [1, 1], hlit=287); w.put(0, 16)
    add("hlit-287", one(w, b""), "HLIT_HDIST")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 1}, 257), [1, 1], hdist=31); w.put(0, 16)
    add("hdist-31", one(w, b""), "HLIT_HDIST")
    w = Bits(); stored(w, 1, b"abcd", nlen=0x1234)
    add("stored-len", one(w, b"abcd"), "STORED_LEN")
    w = Bits(); stored(w, 1, b"0123456789", ln=100)
    add("stored-run", one(w, b"0123456789"), "STORED_RUN")
    w = Bits(); w.put(1, 1); w.put(3, 2); w.put(0, 13)
    add("btype-3", one(w, b""), "BTYPE")
    w = Bits(); b = dynamic(w, 1, lens_of({65: 1, 256: 2, 257: 2}, 258), [1]); b.lit(b"A"); b.sym(257); w.put(1, 1); b.end(); w.put(0, 32)
    add("badcode", one(w, b"AAAA"), "BADCODE")
    add("wrong-isize", member(ok, b"0123456789", isize=15), "LENGTH")
    text = b"The quick brown fox jumps over the lazy dog.\n" * 8
    st = bytearray(deflate_raw(text, 0))
    st[40] ^= 0x10                                           # a stored byte: nothing but the CRC sees it
    add("crc-only", member(bytes(st), text), "CRC")
    add("trailing", member(ok + b"\0", b"0123456789"), "TRAILING")
    out["plain-gzip"] = (gzip.compress(b"@r\nACGT\n+\nIIII\n"), R["FLG"], 0, 0)
    return out, good, bare


def expected(blob):
    return gzip.decompress(blob) if blob else b""
