"""Segment geometry by construction for the suffix sorts behind the 16-symbol key (k_refine.hip: k_refine_big / block_sort,
k_refine_listed / big_sort; k_bigseg.hip: huge_batch, bfq_refine_huge): the collections of tests/test_segment_host.py and
tests/test_gpu_segments.py, and the functions that read a collection's segments back out of the oracle's LCP array.

Plain numpy; neither the GPU nor the package is touched (the oracle's output, where a function needs it, is passed in).

Rows that share their 16-symbol sort key form a segment.  The oracle's LCP counts bases only and terminators never match, so
row i continues the segment of row i - 1 exactly when lcp[i] >= 16: segments(lcp).  In the same way the rows still tied
after the text up to depth d has been looked at are the runs of lcp >= d: runs(lcp, d, first, rows).  Which rows are the
whole reads a builder designed comes from the oracle's suffix array (read_rows).  Nothing here says where a segment lies
without the host test asserting it from those.

The builders (every one is seeded, and shuffles its reads so that the final order differs from the slot order):
  class_case   part A: one designed segment of exactly g rows in one of four tail forms
  placed       part B: a T x 16 (the collection's last rows) or G x 16 segment with its head a chosen number of rows
               before a chunk border
  grids_case   part C: more segments in every size class than its launch has workgroups
  copies_case, compaction_case, border_case, passes_case, cap_case, two_case   part D: the radix rounds of k_bigseg.hip
"""
import numpy as np

# the kernels' constants, mirrored (tests/test_segment_host.py holds them to the sources)
RF_CHUNK = 2048       # k_refine.hip: rows per wavefront chunk
LOOK = 128            # k_refine.hip: the chunk kernel reads keys of RF_CHUNK + 128 rows
RB_SMALL = 512        # k_refine.hip: largest segment of the one-wavefront classes
HUGE = 2048           # BFQ_HUGE_SEG: above it a segment goes to the radix rounds
KEY = 16              # BFQ_KEY_SYMS: symbols of the sorted key, and of one radix round of k_bigseg.hip
WORD = 21             # BFQ_SYMS_PER_WORD: a round of k_refine.hip looks at two words
SCAN_TILE = 4096      # k_scan.hip: SC_THREADS * SC_ITEMS
PASS_SWITCH = 65536   # k_bigseg.hip: the second sort of a round takes 2 passes while nsub <= 1 << 16
CLASSES = ((65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048))     # PMIN + 1 .. PMAX of the five launches
GRIDS = (8192, 8192, 4096, 2048, 1024)                                       # their workgroups
THREADS = (64, 64, 64, 128, 256)
G_ALL = (65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
G_BORDER = (128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
G_FULL = (128, 256, 512, 1024, 2048)                                         # one per class, compared in full
DS = (20, 21, 22, 41, 42, 43, 84, 85)                                        # form 3: common bases behind the key

ACGT = np.frombuffer(b"ACGT", np.uint8)
ACG = np.frombuffer(b"ACG", np.uint8)


class Case:
    """A collection (b, q, r), the tag of every read (0: filler, > 0: what the builder says) and what it is meant to hold."""

    def __init__(self, name, reads, tags, rng, shuffle=True, **meta):
        tags = np.asarray(tags, np.int64)
        assert len(reads) == len(tags)
        if shuffle:
            perm = rng.permutation(len(reads))
            reads = [reads[i] for i in perm]
            tags = tags[perm]
        self.name = name
        self.b = np.frombuffer(b"".join(reads), np.uint8)
        self.q = rng.integers(35, 75, len(self.b)).astype(np.uint8)
        self.r = np.zeros(len(reads) + 1, np.uint64)
        self.r[1:] = np.cumsum(np.fromiter((len(x) for x in reads), np.int64, len(reads)))
        self.tags = tags
        self.n = len(self.b) + len(reads)
        self.meta = meta

    def __repr__(self):
        return self.name

    def __getattr__(self, k):
        try:
            return self.__dict__["meta"][k]
        except KeyError:
            raise AttributeError(k)

    @property
    def bqr(self):
        return self.b, self.q, self.r


# ------------------------------------------------------------------------------------------ geometry from the oracle
def segments(lcp):
    """(first row, rows) of every segment of >= 2 rows, as an array of shape (k, 2): row i joins row i - 1 iff lcp[i] >= 16."""
    return runs(lcp, KEY, 0, len(lcp))


def runs(lcp, depth, first, rows):
    """(first row, rows) of every run of >= 2 rows inside [first, first + rows) whose neighbours share >= depth bases."""
    j = (np.asarray(lcp[first:first + rows]) >= depth).astype(np.int8)
    if len(j):
        j[0] = 0                                                      # the first row joins nothing inside the range
    d = np.diff(np.concatenate([[0], j, [0]]))
    a = np.flatnonzero(d == 1) - 1
    e = np.flatnonzero(d == -1)
    return np.stack([a + first, e - a], 1).astype(np.int64).reshape(-1, 2)


def class_of(rows):
    """Index of the k_refine_big launch that sorts a segment of that many rows; None below 65, 5 for the radix rounds."""
    if rows <= 64:
        return None
    for k, (lo, hi) in enumerate(CLASSES):
        if lo <= rows <= hi:
            return k
    return 5


def padded(rows):
    """block_sort's P: the power of two from 128 up that holds the segment."""
    P = 128
    while P < rows:
        P <<= 1
    return P


def read_rows(sa, case, tag):
    """eBWT rows of the designed suffixes of the reads with that tag: the suffix behind the read's lead base, or the whole
    read where the case has none (the suffix array holds text positions, one terminator behind every read)."""
    idx = np.flatnonzero(case.tags == tag)
    inv = np.empty(len(sa), np.int64)
    inv[np.asarray(sa, np.int64)] = np.arange(len(sa))
    return np.sort(inv[case.r[idx].astype(np.int64) + idx + case.meta.get("lead", 0)])


def segment_of(segs, rows):
    """The one segment (first, rows) that holds all the given rows."""
    k = int(np.searchsorted(segs[:, 0], rows[0], "right")) - 1
    assert k >= 0, "no segment there"
    st, sz = int(segs[k, 0]), int(segs[k, 1])
    assert st <= rows[0] and rows[-1] < st + sz, (st, sz, int(rows[0]), int(rows[-1]))
    return st, sz


def rounds_left(lcp, huge):
    """[(slots, sub-segments)] left after every 16-symbol round of huge_batch over the segments `huge` ([(first, rows)]):
    after round k the rows still tied are the runs of lcp >= 16 * (k + 1).  Ends with the first (0, 0)."""
    out = []
    depth = 2 * KEY
    while True:
        slots = subs = 0
        for st, sz in huge:
            rr = runs(lcp, depth, st, sz)
            slots += int(rr[:, 1].sum())
            subs += len(rr)
        out.append((slots, subs))
        if not slots:
            return out
        depth += KEY


# ------------------------------------------------------------------------------------------ pieces
def _rand(rng, L, alphabet=ACGT):
    return alphabet[rng.integers(0, len(alphabet), int(L))].tobytes()


def _other(rng, c):
    return bytes([int(rng.choice([x for x in b"ACGT" if x != c]))])


def _lead(reads, bases=b"ACGT", k0=0):
    """One more base in front of every read, each of `bases` about equally often.  The rows of whole-read suffixes all show
    the terminator in the BWT and '#' in QS, and no walk of the inversion goes on from them: no output depends on the order
    of equal ones.  Behind a lead base the designed suffixes show that base and its (random) quality, so a wrong order among
    equal suffixes is seen in the eBWT."""
    return [bases[(k0 + i) % len(bases):(k0 + i) % len(bases) + 1] + x for i, x in enumerate(reads)]


def _lens_for_rows(rows, L=100):
    """Read lengths (L, the last one shorter) whose bases + reads make exactly `rows` rows."""
    k = rows // (L + 1)
    rest = rows - k * (L + 1)
    lens = [L] * k
    if rest:
        lens.append(rest - 1)                                         # (rest = 1: an empty read)
    assert sum(lens) + len(lens) == rows
    return lens


def _filler(rng, rows, alphabet=ACG):
    """Reads of exactly `rows` rows drawn from a short genome over `alphabet` (equal keys among them)."""
    genome = alphabet[rng.integers(0, len(alphabet), 700)]
    out = []
    for L in _lens_for_rows(rows):
        st = int(rng.integers(0, 700))
        out.append(np.tile(genome, L // 700 + 2)[st:st + L].tobytes())
    return out


def _some_reads(rng, k=30):
    return [_rand(rng, rng.integers(20, 61)) for _ in range(k)]


# ------------------------------------------------------------------------------------------ part A
def _tails(rng, g, form, D):
    if form == 1:                                                     # tied to the terminator: by read index
        return [b""] * g
    if form == 2:                                                     # 0 .. 100 bases, the start copied from an earlier tail: LCPs of every value
        t = []
        for L in rng.integers(0, 101, g):
            src = t[int(rng.integers(0, len(t)))] if t else b""
            keep = int(rng.integers(0, min(len(src), int(L)) + 1))
            t.append(src[:keep] + _rand(rng, int(L) - keep))
        return [b"ACGT"[i % 4:i % 4 + 1] + x[1:] if x else x for i, x in enumerate(t)]   # (one offset on, g / 4 rows share a key)
    if form == 3:                                                     # the deciding symbol is symbol 16 + D of the suffix
        C = _rand(rng, D)
        return [C + _rand(rng, L) for L in rng.integers(0, 31, g)]
    assert form == 4 and g >= 128
    base = _rand(rng, 50)
    near = base[:44] + _other(rng, base[44]) + base[45:]              # differs behind round 0's 42 symbols
    pair = _rand(rng, 60)
    short = _rand(rng, 10)                                            # the terminator in round 0's first word
    t = [base] * 70 + [near] * 5 + [pair] * 2 + [short] * 3
    if g >= 512:
        b2 = _rand(rng, 48)
        t += [b2] * 65 + [b2 + b"A"] * 33 + [b2 + b"C"] * 32
    while len(t) < g:
        t.append(_rand(rng, 42 + int(rng.integers(0, 20))))           # on its own after round 0 (all but never two alike)
    return t


def class_case(g, form, D=0, seed=None):
    """g reads (tag 1) of a lead base, a common random 16-base head and a tail, among 30 other reads: the head's segment has
    exactly g rows."""
    rng = np.random.default_rng(1000 * form + 100_000 * D + g if seed is None else seed)
    H = _rand(rng, KEY)
    reads = _lead([H + t for t in _tails(rng, g, form, D)])
    other = _some_reads(rng)
    return Case("A%d_g%d%s" % (form, g, "_D%d" % D if form == 3 else ""), reads + other, [1] * g + [0] * len(other), rng,
                g=g, form=form, D=D, lead=1)


# ------------------------------------------------------------------------------------------ part B
def placed(name, kind, g, d, behind=0, fill_extra=0, seed=0):
    """g reads of a smaller lead base and 16 T (kind "T": the largest key there is, so the segment is the collection's last
    rows) or 16 G with `behind` reads "T" + 20 bases of ACG sorting behind it, the head d rows before a chunk border
    (d = RF_CHUNK: on a chunk's row 0).  Rows before the head: every suffix of the filler (ACG only), 17 other suffixes per
    designed read (the whole read, and 16 with a terminator inside the key), 21 per read behind."""
    rng = np.random.default_rng(7000 + seed)
    fixed = (KEY + 1) * g + (WORD * behind if kind == "G" else 0)
    assert kind in "TG" and (kind == "G" or not behind) and 1 <= d <= RF_CHUNK
    j = (fixed + d + 101) // RF_CHUNK + 1 + fill_extra
    head = j * RF_CHUNK - d
    fill = _filler(rng, head - fixed)
    des = _lead([kind.encode() * KEY] * g, b"ACG" if kind == "T" else b"AC")
    back = [b"T" + _rand(rng, 20, ACG) for _ in range(behind)]
    return Case(name, des + back + fill, [1] * g + [2] * behind + [0] * len(fill), rng,
                kind=kind, g=g, d=d, behind=behind, head=head, border=j * RF_CHUNK, lead=1)


def _end_cases():
    out = []
    for res in (0, 1, 2047):
        d = 30
        g = d + (RF_CHUNK + res if res < 2 else res)                  # the end is on res modulo the chunk, beyond the look-ahead
        out.append(("end_T_n%d" % res, "T", g, d, 0))
        out.append(("end_G_n%d" % res, "G", g, d, RF_CHUNK))          # the same segment, 2048 rows behind it: n keeps its residue
    out.append(("end_T_n2047_g2048", "T", RF_CHUNK, 1, 0))
    return out


# name, kind, g, d, reads behind
PART_B = [
    ("end_127", "T", 137, 10, 0),              # the next head on the last row the look-ahead has a head bit for
    ("end_128", "T", 138, 10, 0),
    ("end_129", "T", 139, 10, 0),
    ("last_row", "T", 200, 1, 0),                # nothing left of the head's chunk to scan
    ("row0_513", "T", 513, RF_CHUNK, 0),
    ("row0_1025", "T", 1025, RF_CHUNK, 0),
    ("row0_2047", "T", 2047, RF_CHUNK, 0),
    ("row0_2177", "T", RF_CHUNK + LOOK + 1, RF_CHUNK, 0),   # searched from a chunk's row 0: the 512-row scan runs 4 steps
    ("end_on_border", "G", RF_CHUNK + 5, 5, 7),  # the next head is row 0 of the next chunk
    ("no_head_chunk", "T", RF_CHUNK + 300, 100, 0),
] + _end_cases()
PART_B_PILES = ("end_128", "end_129") + tuple(x[0] for x in _end_cases())
LONG = ("long_140000", "T", 140_000, 777, 0)


def part_b(name):
    for k, x in enumerate(PART_B + [LONG]):
        if x[0] == name:
            nm, kind, g, d, behind = x
            return placed(nm, kind, g, d, behind, fill_extra=24 if nm == LONG[0] else 0, seed=k)
    raise KeyError(name)


def length_known(st, end):
    """The chunk kernel finds the next head itself while it lies on a row it has a head bit for: up to the chunk's end + 127."""
    return end <= (st // RF_CHUNK + 1) * RF_CHUNK + LOOK - 1


# ------------------------------------------------------------------------------------------ part C
C_DISTINCT = (170, 170, 90, 45, 22)
C_COPIES = (65, 200, 300, 600, 1100)


def grids_case():
    """Reads of 80 bases, the last 10 of every copy random: every distinct read gives about 55 segments of `copies` rows."""
    rng = np.random.default_rng(31)
    blocks = []
    for distinct, copies in zip(C_DISTINCT, C_COPIES):
        for _ in range(distinct):
            blk = np.tile(ACGT[rng.integers(0, 4, 80)], (copies, 1))
            blk[:, 70:] = ACGT[rng.integers(0, 4, (copies, 10))]
            blocks.append(blk)
    rows = np.concatenate(blocks)
    reads = [x.tobytes() for x in rows]
    return Case("C_grids", reads, [0] * len(reads), rng)


# ------------------------------------------------------------------------------------------ part D
def copies_case():
    """2049 copies of one 300-base read: 285 segments of 2049 rows, tied to the terminator."""
    rng = np.random.default_rng(41)
    return Case("D_2049x300", [_rand(rng, 300)] * 2049, [1] * 2049, rng, copies=2049, L=300)


def _mer(i, L=KEY):
    """The 16-mer whose order among such is that of i."""
    return ACGT[(int(i) >> (2 * np.arange(L - 1, -1, -1))) & 3].tobytes()


def compaction_case():
    """Three huge segments and no other (whatever shares 32 symbols also shares the key one offset further on, so the rows
    that stay tied are kept to 1025 per common continuation, and the tails of every segment start with each base about
    equally often: the segments of the offset-1 suffixes stay below BFQ_HUGE_SEG).
      X  4095 reads, head + 21 random bases: done after round 1.
      Y  4096 reads, head + m_i (sorted as i) + a second 16-mer: for even i two reads alike and a third one base longer, for
         odd i one read: 1024 tied sub-segments of 3 slots after round 1 with single slots between them; one triple's third
         read differs inside the second 16-mer, so round 2 leaves one slot less; done after round 3.
      Z  4097 reads: 1024 with 50 common bases behind the head and one that leaves them at symbol 16 + 40 (1025 slots after
         rounds 1 and 2, 1024 after round 3, done after round 4); the others differ at once.
    Slots left: 3072 + 1025 = 4097 after round 1, 4096 after round 2, 1024 after round 3, 0 after round 4."""
    rng = np.random.default_rng(43)
    hx, hy, hz = (b"A" + _rand(rng, 15), b"C" + _rand(rng, 15), b"G" + _rand(rng, 15))
    X = _lead([hx + b"ACGT"[i % 4:i % 4 + 1] + _rand(rng, 20) for i in range(4095)], k0=1)
    Y = []
    for i in range(2048):
        m, m2 = _mer(i << 21), _rand(rng, KEY)
        if i % 2:
            Y.append(hy + m + m2)
        elif i == 100:
            Y += [hy + m + m2, hy + m + m2, hy + m + m2[:15] + _other(rng, m2[15])]
        else:
            Y += [hy + m + m2, hy + m + m2, hy + m + m2 + b"A"]
    Y = _lead(Y)
    C = _rand(rng, 50)
    Z = [hz + C + _rand(rng, L) for L in rng.integers(0, 12, 1024)]
    Z.append(hz + C[:40] + _other(rng, C[40]) + _rand(rng, 9))
    rest = [x for x in b"ACGT" if x != C[0]]
    Z += [hz + bytes([rest[i % 3]]) + _rand(rng, 20) for i in range(4097 - 1025)]
    Z = _lead(Z)
    other = _some_reads(rng)
    return Case("D_compaction", X + Y + Z + other, [1] * 4095 + [2] * 4096 + [3] * 4097 + [0] * len(other), rng,
                left=[(4097, 1025), (4096, 1025), (1024, 1), (0, 0)], lead=1)


def border_case():
    """2049 reads H1 + C and 2049 reads H2 + C, H1 and H2 alike but for their last base: after the first round the last
    sub-segment of the first segment and the first of the second have the same key."""
    rng = np.random.default_rng(47)
    R, C = _rand(rng, 15), _rand(rng, 40)
    reads = _lead([R + b"A" + C] * 2049 + [R + b"C" + C] * 2049)
    other = _some_reads(rng)
    return Case("D_border", reads + other, [1] * 2049 + [2] * 2049 + [0] * len(other), rng, lead=1)


def passes_case(K):
    """A + P + X_i and C + P + X_i for K distinct 16-mers X_i: the segment of P, 2K rows, leaves K tied pairs after its first
    round, each of an A and a C row in the order of their reads.  The X_i differ within their first 15 symbols, so the two
    segments of the whole reads (K rows each) leave nothing tied."""
    rng = np.random.default_rng(53)
    P = ACGT[rng.integers(0, 4, KEY)]
    i = np.arange(K)
    X = ACGT[(i[:, None] >> (2 * np.arange(KEY))[None, :]) & 3]
    assert K < 1 << 30                                                # the last symbol of every X_i is A
    rows = np.repeat(np.concatenate([np.zeros((K, 1), np.uint8), np.tile(P, (K, 1)), X], 1), 2, 0)
    rows[0::2, 0] = ord("A")
    rows[1::2, 0] = ord("C")
    reads = [x.tobytes() for x in rows]
    return Case("D_passes_%d" % K, reads, [1] * len(reads), rng, K=K, lead=1)


def _designed(rng, g, form, first):
    H = first + _rand(rng, 15)
    return _lead([H + t for t in _tails(rng, g, form, 0)])


def cap_case():
    """Segments of 3000 (random tails), 4096 (tails from a small set) and 4097 rows (tied to the terminator)."""
    rng = np.random.default_rng(59)
    reads = _designed(rng, 3000, 2, b"A") + _designed(rng, 4096, 4, b"C") + _designed(rng, 4097, 1, b"G")
    other = _some_reads(rng)
    return Case("D_cap3", reads + other, [1] * 3000 + [2] * 4096 + [3] * 4097 + [0] * len(other), rng, sizes=(3000, 4096, 4097), lead=1)


def two_case():
    rng = np.random.default_rng(61)
    reads = _designed(rng, 2500, 2, b"A") + _designed(rng, 3500, 4, b"C")
    other = _some_reads(rng)
    return Case("D_cap2", reads + other, [1] * 2500 + [2] * 3500 + [0] * len(other), rng, sizes=(2500, 3500), lead=1)


def g2049_case(form=1):
    c = class_case(2049, form)
    c.name = "D_g2049_f%d" % form
    return c
