"""The BFQEDIT1 container (include/bfqzip_hip.h) stated in Python: the edit list of two FASTQ texts, encode, decode with
the first offending edit, apply, `shape` and `target_sum`.  Plain integers and bytes: no numpy arithmetic that could wrap
differently from the definition."""
import struct

M64 = (1 << 64) - 1
S = 1024
HDR = 64
NOPOS = M64
TMAX = 1 << 56


def fmix64(x):
    x &= M64
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M64
    x ^= x >> 33
    return x


def pad8(n):
    return (n + 7) & ~7


def records(text):
    """[(sequence start, sequence length)] of a FASTQ text; CR before LF dropped; a missing final newline is supplied"""
    text = bytes(text)
    lines, at = [], 0
    while at < len(text):
        e = text.find(b"\n", at)
        if e < 0:
            e = len(text)
        lines.append((at, e))
        at = e + 1
    assert len(lines) % 4 == 0, "FASTQ: number of lines is not a multiple of 4"
    out = []
    for i in range(0, len(lines), 4):
        s, e = lines[i + 1]
        if e > s and text[e - 1] == 13:
            e -= 1
        out.append((s, e - s))
    return out


def shape_of(lens):
    return sum(fmix64(r * 65536 + l) for r, l in enumerate(lens)) & M64


def edit_list(a, b):
    """(pos[], byte[], N, T, shape, target_sum, reads touched) of the run that made text b out of text a"""
    a, b = bytes(a), bytes(b)
    ra, rb = records(a), records(b)
    assert len(ra) == len(rb), "record counts differ"
    pos, byt, g0, tsum, touched = [], [], 0, 0, 0
    for r, ((sa, la), (sb, lb)) in enumerate(zip(ra, rb)):
        assert la == lb, "read %d differs in length" % r
        any_ = False
        for j in range(la):
            if a[sa + j] != b[sb + j]:
                pos.append(g0 + j); byt.append(a[sa + j])
                tsum += fmix64((g0 + j) * 256 + b[sb + j])
                any_ = True
        touched += any_
        g0 += la
    return pos, byt, len(ra), g0, shape_of([l for _, l in ra]), tsum & M64, touched


def seg_words(c, w):
    return ((c - 1) * w + 63) >> 6


def encode(pos, byt, N, T, shape, target_sum, widths=None):
    """One member.  widths: per segment, a width to write instead of the canonical one (to build malformed members)."""
    E = len(pos)
    assert len(byt) == E
    nseg = (E + S - 1) // S
    first, wt, gaps = b"", b"", b""
    for s in range(nseg):
        seg = pos[s * S:(s + 1) * S]
        g = [seg[j + 1] - seg[j] - 1 for j in range(len(seg) - 1)]
        w = max(g).bit_length() if g else 0
        if widths is not None and widths.get(s) is not None:
            w = widths[s]
        bits = 0
        for j, v in enumerate(g):
            bits |= (v & ((1 << w) - 1)) << (j * w)
        first += struct.pack("<Q", seg[0])
        wt += bytes([w])
        gaps += bits.to_bytes(8 * seg_words(len(seg), w), "little")
    wt += bytes(pad8(nseg) - nseg)
    payload = first + wt + gaps + bytes(byt) + bytes(pad8(E) - E)
    return b"BFQEDIT1" + struct.pack("<QQQIIQQQ", N, T, E, S, 0, shape, target_sum, len(payload)) + payload


def container(a, b):
    pos, byt, N, T, shape, tsum, _ = edit_list(a, b)
    return encode(pos, byt, N, T, shape, tsum)


class Malformed(Exception):
    def __init__(self, first_bad, why):
        super().__init__("%s (first_bad %s)" % (why, "none" if first_bad == NOPOS else first_bad))
        self.first_bad = first_bad


def member_len(z):
    return HDR + struct.unpack_from("<Q", z, 56)[0]


def decode(z):
    """ONE member of exactly len(z) bytes -> dict(pos, byte, N, T, E, shape, target_sum); Malformed with .first_bad"""
    z = bytes(z)
    if len(z) < HDR or z[:8] != b"BFQEDIT1":
        raise Malformed(NOPOS, "magic")
    N, T, E, s_, flags, shape, tsum, payload = struct.unpack_from("<QQQIIQQQ", z, 8)
    if s_ != S or flags or T > TMAX or E > T:
        raise Malformed(NOPOS, "header")
    if payload > len(z) - HDR:
        raise Malformed(NOPOS, "short")
    nseg = (E + S - 1) // S
    off_w = HDR + 8 * nseg
    off_g = off_w + pad8(nseg)
    if off_g - HDR + pad8(E) > payload:
        raise Malformed(NOPOS, "length")
    counts = [min(S, E - s * S) for s in range(nseg)]
    words = 0
    for s in range(nseg):
        if z[off_w + s] > 56:
            raise Malformed(s * S, "width above 56")
        words += seg_words(counts[s], z[off_w + s])
        if words > payload // 8:
            raise Malformed(NOPOS, "length")
    off_b = off_g + 8 * words
    if off_b - HDR + pad8(E) != payload or HDR + payload != len(z):
        raise Malformed(NOPOS, "length")
    if any(z[off_w + nseg:off_g]) or any(z[off_b + E:off_b + pad8(E)]):
        raise Malformed(NOPOS, "padding")
    pos, at, prev = [], off_g, None
    for s in range(nseg):
        w, c = z[off_w + s], counts[s]
        nw = seg_words(c, w)
        bits = int.from_bytes(z[at:at + 8 * nw], "little")
        at += 8 * nw
        g = [(bits >> (j * w)) & ((1 << w) - 1) for j in range(c - 1)]
        cur = struct.unpack_from("<Q", z, HDR + 8 * s)[0]
        if (prev is not None and cur <= prev) or (max(g).bit_length() if g else 0) != w or bits >> ((c - 1) * w):
            raise Malformed(s * S, "segment")
        for j in range(c):
            if j:
                cur += g[j - 1] + 1
            if cur >= T or not 33 <= z[off_b + s * S + j] <= 126:
                raise Malformed(s * S + j, "edit")
            pos.append(cur)
        prev = cur
    return dict(pos=pos, byte=list(z[off_b:off_b + E]), N=N, T=T, E=E, shape=shape, target_sum=tsum)


def members(z):
    z, out, at = bytes(z), [], 0
    while at < len(z):
        n = member_len(z[at:])
        out.append(z[at:at + n])
        at += n
    return out


def apply(text, z):
    """text with the members' bytes written back at the edit positions (the checks of bfq_fastq_unedit as assertions)"""
    text = bytearray(text)
    recs = records(text)
    r0 = g_base = 0
    for m in members(z):
        d = decode(m)
        part = recs[r0:r0 + d["N"]]
        assert len(part) == d["N"] and sum(l for _, l in part) == d["T"] and shape_of([l for _, l in part]) == d["shape"]
        where, g0 = [], 0
        for s, l in part:
            where.append((g0, s, l)); g0 += l
        tsum, k = 0, 0
        for g, b in zip(d["pos"], d["byte"]):
            while not where[k][0] <= g < where[k][0] + where[k][2]:
                k += 1
            a = where[k][1] + g - where[k][0]
            tsum += fmix64(g * 256 + text[a])
            text[a] = b
        assert tsum & M64 == d["target_sum"], "the text is not the output these edits were made from"
        r0 += d["N"]
    assert r0 == len(recs)
    return bytes(text)
