"""The BFQQUAL1 container (include/bfqzip_hip.h, bfqzip_amd/csrc/k_quals.hip) as Python: the statement the kernels are compared
with, byte for byte.  Quality lines in read order, every value coded against a context made of the value before it, a coarse
view of the two before that, its place in the read and how noisy the read has been so far; a static model counted on a
sample, stored rows, rANS with one stream per segment of reads.  The `lens` member is made by the CPU statement of the
general codec (oracle.orc.codec_encode), which is what bfq_stream_compress is held to; the checksum is restated here."""
import struct
from bisect import bisect_right
import numpy as np
from oracle import orc

S = 1024
SCALE = 12
M12 = 1 << SCALE
RANS_L = 1 << 23
MAX_LINE = 65535
MAX_TABLE = 1 << 22
HDR = 72
RUNGS = ((1, 1, 1, 1), (4, 4, 2, 1), (8, 8, 4, 1), (8, 16, 4, 2))          # (M, P, D, E)


class Damaged(Exception):
    pass


def _bytes(data):
    return data.tobytes() if isinstance(data, np.ndarray) else bytes(data)


def _log2(v):
    return v.bit_length() - 1


# ---- the codec's checksum (oracle/bfq_codec_ref.c states it) -------------------------------------------------------------
def _mix64(z):
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def checksum(data):
    data = _bytes(data)
    n = len(data)
    w = np.frombuffer(data + b"\0" * (-n % 8), "<u8")
    with np.errstate(over="ignore"):
        j = np.arange(1, len(w) + 1, dtype=np.uint64)
        total = int(_mix64(w + j * np.uint64(0x9E3779B97F4A7C15)).sum(dtype=np.uint64)) if len(w) else 0
        return int(_mix64(np.array([n ^ total], np.uint64))[0])


# ---- the stream as lines ------------------------------------------------------------------------------------------------
def split(data):
    """(lens, vals) of a stream that ends with a newline."""
    a = np.frombuffer(_bytes(data), np.uint8)
    ends = np.flatnonzero(a == 10)
    lens = np.diff(np.concatenate([[-1], ends])) - 1
    return lens.astype(np.int64), a[a != 10]


def eligible(data):
    data = _bytes(data)
    if not data.endswith(b"\n"):
        return False
    lens, vals = split(data)
    return len(vals) >= 1 and int(lens.max()) <= MAX_LINE and len(np.unique(vals)) <= 64


def sample_step(nvals):
    return min(64, max(1, nvals >> 24))


def rung_rows(r, A):
    M, P, D, E = RUNGS[r]
    return P * D * E * M * A


def rung_max(A, nvals):
    limit = min(MAX_TABLE, max(4096, (nvals // sample_step(nvals)) // 16))
    return max(r for r in range(4) if r == 0 or rung_rows(r, A) * A <= limit)


def features(ranks, lens, A, maxlen):
    """q1, m8, e, p16, d4 of every value (arrays over vals)."""
    n = len(ranks)
    boff = np.concatenate([[0], np.cumsum(lens)])
    start = np.repeat(boff[:-1], lens)
    j = np.arange(n) - start
    s = ranks.astype(np.int64)

    def back(k):
        q = np.zeros(n, np.int64)
        q[k:] = s[:-k] if k else s
        q[j < k] = 0
        return q
    q1, q2, q3 = back(1), back(2), back(3)
    m8 = np.maximum(q2, q3) * 8 // A
    e = (q2 == q3).astype(np.int64)
    W = max(1, -(-maxlen // 16))
    p16 = np.minimum(15, j // W)
    ad = np.abs(s - q1)
    ad[j == 0] = 0
    G = np.cumsum(ad)
    delta = np.zeros(n, np.int64)
    if n > 1:
        delta[1:] = G[:-1] - G[start[1:]]
    delta[j == 0] = 0
    d4 = (delta >= 8).astype(np.int64) + (delta >= 32) + (delta >= 128)
    return q1, m8, e, p16, d4


def context(r, A, q1, m8, e, p16, d4):
    M, P, D, E = RUNGS[r]
    m = m8 >> (3 - _log2(M))
    p = p16 >> (4 - _log2(P))
    d = d4 >> (2 - _log2(D))
    ee = e if E == 2 else 0
    return (((p * D + d) * E + ee) * M + m) * A + q1


def collapse(cnt, rhi, rlo, A):
    """counts at rung rhi (rows x A) summed into the rows of rung rlo <= rhi"""
    if rhi == rlo:
        return cnt
    M, P, D, E = RUNGS[rhi]
    c = np.arange(rung_rows(rhi, A))
    q1 = c % A; c //= A
    m = c % M; c //= M
    e = c % E; c //= E
    d = c % D; p = c // D
    m8, p16, d4 = m << (3 - _log2(M)), p << (4 - _log2(P)), d << (2 - _log2(D))
    to = context(rlo, A, q1, m8, e, p16, d4)
    out = np.zeros((rung_rows(rlo, A), A), np.int64)
    np.add.at(out, to, cnt)
    return out


def normalise_rows(cnt):
    """normalise() of oracle/bfq_codec_ref.c on every row of cnt (rows x A)"""
    cnt = cnt.astype(np.int64)
    T = cnt.sum(1, keepdims=True)
    v = np.maximum(1, np.where(T > 0, cnt * M12 // np.maximum(T, 1), 0))
    tot = v.sum(1)
    while True:
        rows = np.flatnonzero(tot > M12)
        if not len(rows):
            break
        best = v[rows].argmax(1)
        d = np.minimum(tot[rows] - M12, v[rows, best] - 1)
        v[rows, best] -= d
        tot[rows] -= d
    rows = np.flatnonzero(tot < M12)
    best = v[rows].argmax(1)
    v[rows, best] += M12 - tot[rows]
    return v


def _bit_cost(f):
    e = f.bit_length() - 1
    m = f << (31 - e)
    frac = 0
    for _ in range(8):
        m = (m * m) >> 31
        frac <<= 1
        if m >> 32:
            frac |= 1
            m >>= 1
    return SCALE * 256 - (e * 256 + frac)


BIT_COST = np.array([0] + [_bit_cost(f) for f in range(1, M12 + 1)], np.int64)


def estimate(cnt, A, St):
    """estimated bits of the container made with these counts (choose_order() of oracle/bfq_codec_ref.c)"""
    used = cnt.sum(1) > 0
    f = normalise_rows(cnt[used])
    bits = int((cnt[used] * BIT_COST[f]).sum())
    return bits // 256 * St + int(used.sum()) * A * 16 + len(cnt)


def rans_encode(fs, cs):
    """one segment: the values' (freq, cum) in order, coded last to first; the stream as the decoder reads it"""
    x = RANS_L
    out = bytearray()
    for f, c in zip(reversed(fs), reversed(cs)):
        xmax = ((RANS_L >> SCALE) << 8) * f
        while x >= xmax:
            out.append(x & 255)
            x >>= 8
        x = ((x // f) << SCALE) + (x % f) + c
    out += bytes([(x >> 24) & 255, (x >> 16) & 255, (x >> 8) & 255, x & 255])
    return bytes(reversed(out))


def seg_first(boff, nreads, nseg):
    """first read of segment g = 0..nseg: the first read whose first value has an index >= g S"""
    return np.searchsorted(boff[:nreads], np.arange(nseg + 1) * S, side="left")


class Parts:
    """The pieces of a container; bytes() puts them together (tests change pieces to make lying containers)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def lens_member(self):
        return orc.codec_encode(np.frombuffer(np.asarray(self.lens, "<u4").tobytes(), np.uint8)).tobytes()

    def bytes(self):
        lm = self.lens_z if getattr(self, "lens_z", None) is not None else self.lens_member()
        alpha = bytes(self.alphabet) + b"\0" * (64 - len(self.alphabet))
        h = b"BFQQUAL1" + struct.pack("<3Q6IQQ", self.raw_len, self.nreads, self.nvals, self.S, self.nseg, self.A, self.rung, self.scale,
                                      self.maxlen, self.checksum, len(lm))
        return (h + lm + alpha + np.asarray(self.dflt, "<u2").tobytes() + bytes(self.used) + np.asarray(self.freq, "<u2").tobytes() +
                np.asarray(self.seg_bytes, "<u4").tobytes() + b"".join(self.streams))


def parts(data, rung=None):
    """The container of an eligible stream, in pieces.  rung: forced (the counts are then taken at that rung)."""
    data = _bytes(data)
    assert eligible(data)
    lens, vals = split(data)
    nreads, nvals, maxlen = len(lens), len(vals), int(lens.max())
    alphabet = np.unique(vals)
    A = len(alphabet)
    rank = np.zeros(256, np.int64)
    rank[alphabet] = np.arange(A)
    s = rank[vals]
    boff = np.concatenate([[0], np.cumsum(lens)])
    nseg = -(-nvals // S)
    St = sample_step(nvals)
    feats = features(s, lens, A, maxlen)
    rmax = rung_max(A, nvals) if rung is None else rung
    sampled = (np.repeat(boff[:-1] // S, lens) % St) == 0
    key = context(rmax, A, *feats) * A + s
    cnt = np.bincount(key[sampled], minlength=rung_rows(rmax, A) * A).reshape(-1, A)
    best, best_bits = rmax, None
    if rung is None:
        for r in range(rmax + 1):                                   # the lowest rung among equals
            bits = estimate(collapse(cnt, rmax, r, A), A, St)
            if best_bits is None or bits < best_bits:
                best, best_bits = r, bits
    cnt = collapse(cnt, rmax, best, A)
    rows = rung_rows(best, A)
    dflt = normalise_rows(cnt.sum(0, keepdims=True))[0]
    usedrow = cnt.sum(1) > 0
    freq = np.tile(dflt, (rows, 1))
    freq[usedrow] = normalise_rows(cnt[usedrow])
    cum = np.cumsum(freq, 1) - freq
    used = np.packbits(usedrow, bitorder="little").tobytes()
    ctx = context(best, A, *feats)
    fs, cs = freq[ctx, s].tolist(), cum[ctx, s].tolist()
    first = seg_first(boff, nreads, nseg)
    streams, seg_bytes = [], []
    for g in range(nseg):
        a, b = int(boff[first[g]]), int(boff[first[g + 1]])
        z = rans_encode(fs[a:b], cs[a:b]) if b > a else b""
        streams.append(z)
        seg_bytes.append(len(z))
    return Parts(raw_len=len(data), nreads=nreads, nvals=nvals, S=S, nseg=nseg, A=A, rung=best, scale=SCALE, maxlen=maxlen,
                 checksum=checksum(data), lens=lens, lens_z=None, alphabet=alphabet.tolist(), dflt=dflt, used=used, freq=freq[usedrow],
                 seg_bytes=seg_bytes, streams=streams)


def container(data, rung=None):
    return parts(data, rung).bytes()


def general(data):
    """What bfq_stream_compress writes for these bytes."""
    return orc.codec_encode(np.frombuffer(_bytes(data), np.uint8)).tobytes()


def choose(data, always=False, rung=None):
    """What bfq_quals_compress gives: flags 0 keeps the shorter (BFQQUAL1 only when strictly shorter); ineligible streams take
    the general container with any flags."""
    data = _bytes(data)
    if not eligible(data):
        return general(data)
    c = container(data, rung)
    if always:
        return c
    g = general(data)
    return c if len(c) < len(g) else g


# ---- the decoder ----------------------------------------------------------------------------------------------------------
def decode(blob):
    """The raw bytes of one BFQQUAL1 container; Damaged for everything the decoder has to refuse."""
    blob = _bytes(blob)
    if len(blob) < HDR or blob[:8] != b"BFQQUAL1":
        raise Damaged("magic")
    raw_len, nreads, nvals, S_, nseg, A, rung, scale, maxlen, csum, Lb = struct.unpack_from("<3Q6IQQ", blob, 8)
    if S_ != S or scale != SCALE or not 1 <= A <= 64 or rung > 3 or maxlen > MAX_LINE:
        raise Damaged("header")
    if nvals < 1 or nreads < 1 or nseg != -(-nvals // S) or nvals + nreads != raw_len:
        raise Damaged("counts")
    rows = rung_rows(rung, A)
    if HDR + Lb + 64 + 2 * A + (rows + 7) // 8 > len(blob):
        raise Damaged("cut")
    lm = np.frombuffer(blob[HDR:HDR + Lb], np.uint8)
    if Lb < 16 or blob[HDR:HDR + 8] != b"BFQRANS2" or struct.unpack_from("<Q", blob, HDR + 8)[0] != 4 * nreads:
        raise Damaged("lens member")
    try:
        lens = np.frombuffer(orc.codec_decode(lm).tobytes(), "<u4").astype(np.int64)
    except Exception:
        raise Damaged("lens member")
    if len(lens) != nreads or int(lens.sum()) != nvals or int(lens.max()) != maxlen:
        raise Damaged("lens")
    pos = HDR + Lb
    alphabet = list(blob[pos:pos + A]); pos += 64
    if any(b <= a for a, b in zip(alphabet, alphabet[1:])) or 10 in alphabet:
        raise Damaged("alphabet")
    dflt = np.frombuffer(blob[pos:pos + 2 * A], "<u2").astype(np.int64); pos += 2 * A
    usedrow = np.unpackbits(np.frombuffer(blob[pos:pos + (rows + 7) // 8], np.uint8), bitorder="little")[:rows].astype(bool)
    pos += (rows + 7) // 8
    nused = int(usedrow.sum())
    if pos + 2 * A * nused + 4 * nseg > len(blob):
        raise Damaged("cut")
    freq = np.tile(dflt, (rows, 1))
    freq[usedrow] = np.frombuffer(blob[pos:pos + 2 * A * nused], "<u2").reshape(nused, A)
    pos += 2 * A * nused
    if (freq.sum(1) != M12).any():
        raise Damaged("row sum")
    seg_bytes = np.frombuffer(blob[pos:pos + 4 * nseg], "<u4").astype(np.int64); pos += 4 * nseg
    if pos + int(seg_bytes.sum()) != len(blob):
        raise Damaged("seg_bytes")
    cum = (np.cumsum(freq, 1) - freq).tolist()
    freq = freq.tolist()
    M, P, D, E = RUNGS[rung]
    lM, lP, lD = 3 - _log2(M), 4 - _log2(P), 2 - _log2(D)
    W = max(1, -(-maxlen // 16))
    boff = np.concatenate([[0], np.cumsum(lens)])
    first = seg_first(boff, nreads, nseg)
    ranks = np.zeros(nvals, np.int64)
    for g in range(nseg):
        ra, rb = int(first[g]), int(first[g + 1])
        nb = int(seg_bytes[g])
        if boff[rb] == boff[ra]:
            if nb:
                raise Damaged("bytes of an empty segment")
            continue
        if nb < 4:
            raise Damaged("segment")
        z = blob[pos:pos + nb]; pos += nb
        x = z[0] | z[1] << 8 | z[2] << 16 | z[3] << 24
        if x < RANS_L:
            raise Damaged("initial state")
        used = 4
        for r in range(ra, rb):
            o, l = int(boff[r]), int(lens[r])
            q1 = q2 = q3 = delta = 0
            for j in range(l):
                m = (max(q2, q3) * 8 // A) >> lM
                p = min(15, j // W) >> lP
                d = ((delta >= 8) + (delta >= 32) + (delta >= 128)) >> lD
                e = int(q2 == q3) if E == 2 else 0
                c = (((p * D + d) * E + e) * M + m) * A + q1
                slot = x & (M12 - 1)
                cu, fr = cum[c], freq[c]
                sy = bisect_right(cu, slot) - 1
                x = fr[sy] * (x >> SCALE) + slot - cu[sy]
                while x < RANS_L:
                    if used >= nb:
                        raise Damaged("refill past the segment")
                    x = (x << 8) | z[used]; used += 1
                ranks[o + j] = sy
                if j >= 1:
                    delta += abs(sy - q1)
                q3, q2, q1 = q2, q1, sy
        if used != nb:
            raise Damaged("segment not consumed")
    vals = np.asarray(alphabet, np.uint8)[ranks]
    out = np.full(raw_len, 10, np.uint8)
    out[np.arange(nvals) + np.repeat(np.arange(nreads), lens)] = vals
    out = out.tobytes()
    if checksum(out) != csum:
        raise Damaged("checksum")
    return out


# ---- streams ----------------------------------------------------------------------------------------------------------------
def lines_of(arrs):
    return b"".join(bytes(np.asarray(a, np.uint8)) + b"\n" for a in arrs)


def shaped(nreads, length, seed):
    """The seeded generator of the issue: reads of three classes whose values decay along the read, with drop-outs."""
    rng = np.random.default_rng(seed)
    cls = rng.choice(3, size=nreads, p=[.6, .3, .1])
    top = np.array([40., 36., 30.])[cls]
    decay = np.array([.03, .10, .25])[cls]
    u = rng.random((nreads, length))
    step = rng.integers(-3, 4, size=(nreads, length))
    cur = top - 6
    out = np.empty((nreads, length), np.uint8)
    for j in range(length):
        mean = top - decay * j - (6 * (1 - j / 5) if j < 5 else 0)
        uj = u[:, j]
        towards = cur + np.sign(mean - cur)
        cur = np.where(uj < .70, towards, np.where(uj < .78, 2., np.where(uj < .90, np.rint(mean), cur + step[:, j])))
        cur = np.clip(cur, 2, 41)
        out[:, j] = cur.astype(np.uint8) + 33
    return b"".join(row.tobytes() + b"\n" for row in out)


def cases():
    """The streams the kernels are compared on (tests/test_gpu_quals.py), small enough for the Python coder."""
    rng = np.random.default_rng(20261018)
    c = {"shaped_2000x100": shaped(2000, 100, 7)}
    lens = rng.integers(1, 151, 400)
    lens[[0, 17, 18, 399]] = 0
    c["variable_with_empty_lines"] = lines_of(rng.integers(35, 74, int(l)) for l in lens)
    c["one_read"] = lines_of([rng.integers(40, 50, 37)])
    c["long_read_then_empty_segments"] = lines_of([rng.integers(60, 70, 20), rng.integers(35, 75, 5000), rng.integers(40, 44, 30)] + [[]] * 5)
    c["one_line_of_65535"] = lines_of([np.clip(np.cumsum(rng.integers(-1, 2, 65535)) + 60, 35, 90)])
    c["maxlen_below_16"] = lines_of(rng.integers(50, 58, int(l)) for l in rng.integers(0, 16, 300))
    saw = np.concatenate([np.full(4, 40), [40, 47], np.full(6, 47), [40, 60, 40, 60], np.full(5, 50), np.tile([35, 74], 20), np.full(8, 60)])
    c["delta_crosses_8_32_128"] = lines_of([saw, saw[::-1], np.full(40, 50)] * 20)
    c["alphabet_of_1"] = b"IIIIIIII\nIII\n\nI\n" * 50
    c["alphabet_of_64"] = lines_of(rng.integers(33, 97, 90) for _ in range(60))
    bins = np.array([35, 39, 48, 55, 60, 66, 70, 73])
    c["binned_8_levels"] = lines_of(bins[np.clip(np.cumsum(rng.integers(-1, 2, 120)) + 4, 0, 7)] for _ in range(150))
    return c


def ineligible_cases():
    rng = np.random.default_rng(5)
    return {"alphabet_of_65": lines_of(rng.integers(33, 98, 200) for _ in range(40)),
            "no_final_newline": b"IIII\nIII",
            "only_empty_lines": b"\n" * 300}


def refusal_cases():
    """(good stream, {name: container that must be refused}); every one parses as far as its lie."""
    rng = np.random.default_rng(11)
    good = lines_of(rng.integers(40, 52, int(l)) for l in rng.integers(0, 120, 60))
    c = {}

    def vary(**kw):
        p = parts(good, rung=1)
        p.__dict__.update(kw)
        return p.bytes()
    base = parts(good, rung=1)
    c["S"] = vary(S=2048)
    c["scale"] = vary(scale=11)
    c["A_0"] = vary(A=0)
    c["A_65"] = vary(A=65)
    c["rung_4"] = vary(rung=4)
    c["nseg"] = vary(nseg=base.nseg + 1)
    c["nreads"] = vary(nreads=base.nreads + 1)
    c["nvals"] = vary(nvals=base.nvals + 1)
    c["raw_len"] = vary(raw_len=base.raw_len + 1)
    c["maxlen"] = vary(maxlen=base.maxlen + 1)
    c["alphabet_not_ascending"] = vary(alphabet=base.alphabet[:1] + base.alphabet[:1] + base.alphabet[2:])
    c["alphabet_with_newline"] = vary(alphabet=[10] + base.alphabet[1:])
    c["lens_member_of_another_length"] = vary(lens=np.concatenate([base.lens, [0]]))
    moved = base.lens.copy(); moved[0] += 1
    c["lens_sum"] = vary(lens=moved)
    nz = np.flatnonzero((base.lens > 0) & (base.lens < base.maxlen))
    moved = base.lens.copy(); moved[nz[0]] -= 1; moved[nz[1]] += 1
    c["lens_that_move_a_value"] = vary(lens=moved)                  # sums and maximum hold: the checksum (or the coder) must notice
    f = base.freq.copy(); f[0, 0] += 1
    c["row_sum"] = vary(freq=f)
    d = base.dflt.copy(); d[0] -= 1
    c["default_row_sum"] = vary(dflt=d)
    sb = list(base.seg_bytes); sb[0] += 1
    c["seg_bytes"] = vary(seg_bytes=sb)
    c["zeroed_segment"] = vary(streams=[bytes(len(base.streams[0]))] + base.streams[1:])
    ok = base.bytes()
    pay = len(ok) - sum(base.seg_bytes)
    for k in range(20):
        b = bytearray(ok)
        at = pay + int(rng.integers(0, sum(base.seg_bytes)))
        b[at] ^= 1 << int(rng.integers(0, 8))
        c["payload_flip_%d" % k] = bytes(b)
    c["cut"] = ok[:-3]
    c["cut_in_the_table"] = ok[:pay - 10]
    return good, c
