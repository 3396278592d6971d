"""Cluster geometry by construction: a numpy model of the flag rule of k_cluster.hip, LCP arrays that put clusters exactly
where a test wants them, and the collections and cases of tests/test_cluster_host.py and tests/test_gpu_clusters.py.

Plain numpy; neither the GPU nor the package is touched (the oracle, where a helper needs it, is passed in).

Two ways to place a cluster:
  A  bfq_ext's job takes the LCP as given (it comes from a file and is not validated).  So the eBWT and QS of any real
     collection (the inversion closes) with an LCP array written here: every cluster lies where lcp_for() puts it.
  B  the fused paths compute their own LCP.  designed() is a collection with one cluster of a chosen size (the rows of the
     suffix U) whose first row moves down by one per empty read added (one more terminator row in front of it).
"""
import functools
import numpy as np

# the kernels' constants, mirrored (k_cluster.hip unless said otherwise)
FLAG_GROUP = 8        # k_lcp_flags: "8 rows per thread", r0 = g * 8
LANE_ROWS = 16        # k_cluster: "16 rows per lane", CL_WROWS / 64
CL_WROWS = 1024       # #define CL_WROWS (CL_CHUNK / 4): rows per wave, the pieces of firstOut[]
CL_CHUNK = 4096       # #define CL_CHUNK 4096: rows per workgroup
CL_BIG = 2048         # #define CL_BIG 2048: j0 + 8 - start >= CL_BIG hands the cluster to k_big_*
CB_TILE = 65536       # #define CB_TILE 65536
RANK_BLOCK = 64       # prec_sym: load_blk(a.rankBlk, j >> 6)
WINDOWS = (1000, 1024)  # the BFQ_COMPACT_WIN values the GPU module sets (k_compact.hip: lcp_window)
LCP_TOP = 65000       # the device clamps entries at 0xFFFE, the oracle does not; a real eBWT stays far below

K2 = 16               # K of the 2- and 4-byte LCP arrays
K1 = 200              # K of the 1-byte ones: near the type's top


def flags(lcp, K):
    """in() of every row: thr[r] = r>=1 && LCP[r]>=K; min[r] = 1<=r<=n-2 && LCP[r-1]>LCP[r] && LCP[r+1]>=LCP[r]."""
    l = np.asarray(lcp).astype(np.int64)
    n = len(l)
    thr = l >= K
    if n:
        thr[0] = False
    mn = np.zeros(n, bool)
    if n >= 3:
        mn[1:n - 1] = (l[0:n - 2] > l[1:n - 1]) & (l[2:n] >= l[1:n - 1])
    return (thr & ~mn).astype(np.uint8)


def clusters(in_flags):
    """[(first row, last row)]: every maximal run [b, e] of in() is the cluster [b-1, e]."""
    f = np.asarray(in_flags).astype(np.int8)
    d = np.diff(np.concatenate([[0], f, [0]]))
    return [(int(b) - 1, int(e) - 1) for b, e in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1))]


def lcp_for(n, K, wanted, dips=(), seed=0):
    """An LCP array of n rows whose clusters are exactly `wanted` ([(first, last)], ascending).  K inside a run; values in
    [0, K-1] between runs, K-1 beside every other run (decides >= against >).  A row in `dips` is the first row of a cluster
    that follows the last row of the one before, and gets its in() = 0 from the minimum rule instead of the threshold:
    .., K+2, K+2, K, K+1, ..; the run behind a dip stays at K+1."""
    assert 1 <= K and K + 2 <= LCP_TOP
    wanted = [(int(a), int(b)) for a, b in wanted]
    rng = np.random.default_rng(seed)
    lcp = rng.integers(0, K, n).astype(np.uint32)
    firsts = {a for a, _ in wanted}
    assert set(dips) <= firsts, sorted(set(dips) - firsts)
    for i, (a, b) in enumerate(wanted):
        assert 0 <= a < b < n, (a, b, n)
        assert i == 0 or wanted[i - 1][1] < a, "clusters overlap"
        lcp[a + 1:b + 1] = K + 1 if a in dips else K
        if a in dips:
            assert i > 0 and wanted[i - 1][1] + 1 == a, "a dip joins two clusters"
            lcp[a] = K
            lcp[max(a - 2, wanted[i - 1][0] + 1):a] = K + 2
        elif i % 2 == 0:
            lcp[a] = K - 1
        if b + 1 < n and (b + 1) not in dips and i % 2 == 1:
            lcp[b + 1] = K - 1
    assert int(lcp.max(initial=0)) <= LCP_TOP
    assert clusters(flags(lcp, K)) == wanted
    return lcp


def window_hits(cl):
    """How the window borders of WINDOWS lie to the cluster [first, last]: 'first' a border on its first in() row, 'after' on
    the row after its last, 'inside' elsewhere in the run."""
    b, e = cl[0] + 1, cl[1]
    out = set()
    for W in WINDOWS:
        if b % W == 0:
            out.add("first")
        if (e + 1) % W == 0:
            out.add("after")
        if e // W > b // W:
            out.add("inside")
    return out


# ---------------------------------------------------------------------------------------------------- collections
def pack(reads, quals):
    r = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    cat = lambda xs: np.concatenate([np.asarray(x, np.uint8) for x in xs] + [np.zeros(0, np.uint8)])
    return cat(reads), cat(quals), r


def skewed(lens, seed, t=20):
    """Part A's collection: bases drawn A .55, C .33, G .06, T .05, N .01; the rare bases' qualities below t + 33, those of
    A and C over the whole range.  Any row range then has a base above -f 40, and the rare ones in it get replaced."""
    rng = np.random.default_rng(seed)
    tot = int(sum(lens))
    idx = rng.choice(5, tot, p=[.55, .33, .06, .05, .01])
    b = np.frombuffer(b"ACGTN", np.uint8)[idx]
    q = np.where(idx < 2, rng.integers(33, 74, tot), rng.integers(33, t + 33, tot)).astype(np.uint8)
    r = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return b, q, r


def lens_for_rows(n, L=70):
    """Read lengths of a collection with exactly n rows (bases + one terminator per read), reads of L bases but the last."""
    assert n >= 1
    N = max(1, n // (L + 1))
    lens = [L] * (N - 1)
    lens.append(n - N - L * (N - 1))
    assert sum(lens) + len(lens) == n and lens[-1] >= 0
    return lens


def designed(c0, c1, odd, n_empty, U, seed=1):
    """Part B's collection: c0 copies of "AC"+U, c1 of "TG"+U, `odd` of "AT"+U, n_empty empty reads, shuffled.  With
    k = len(U) the rows of the suffix U are one cluster of c0 + c1 + odd rows with two frequent symbols C and G, each with its
    own preceding base.  The odd reads' second base has quality 35 ('#' + 2: not trusted), so it is replaced."""
    rng = np.random.default_rng(seed)
    U = np.frombuffer(U, np.uint8)
    kinds = np.concatenate([np.zeros(c0, np.int8), np.ones(c1, np.int8), np.full(odd, 2, np.int8), np.full(n_empty, 3, np.int8)])
    kinds = kinds[rng.permutation(len(kinds))]
    heads = [b"AC", b"TG", b"AT"]
    reads, quals = [], []
    for kd in kinds:
        if kd == 3:
            reads.append(np.zeros(0, np.uint8)); quals.append(np.zeros(0, np.uint8))
            continue
        reads.append(np.concatenate([np.frombuffer(heads[kd], np.uint8), U]))
        q = rng.integers(53, 74, len(U) + 2).astype(np.uint8)
        if kd == 2:
            q[1] = 35
        quals.append(q)
    return pack(reads, quals)


def find_cluster(lcp, K, size):
    """The one cluster of `size` rows under the oracle's LCP."""
    got = [c for c in clusters(flags(lcp, K)) if c[1] - c[0] + 1 == size]
    assert len(got) == 1, (size, got)
    return got[0]


def place(orc, c0, c1, odd, U, modulus, residue):
    """The designed collection with as many empty reads as put the cluster's first row at `residue` modulo `modulus`; returns
    (bases, quals, roff, (first, last)).  Asserted on the oracle's LCP of the finished collection."""
    size, K = c0 + c1 + odd, len(U)
    b, q, r = designed(c0, c1, odd, 0, U)
    s0 = find_cluster(orc.build_ebwt(b, q, r)[2], K, size)[0]
    n_empty = (residue - s0) % modulus
    b, q, r = designed(c0, c1, odd, n_empty, U)
    cl = find_cluster(orc.build_ebwt(b, q, r)[2], K, size)
    assert cl[0] % modulus == residue and cl[1] - cl[0] + 1 == size, (cl, s0, n_empty)
    return b, q, r, cl


# ---------------------------------------------------------------------------------------------------- part A: the cases
# the smoothing parameters, spread over the cases (never multiplied out): M 0..3, ext 0/1 for M = 1 and 3, B 0/1, m 2/5
PARAMS = (dict(M=0, B=0, m=2), dict(M=1, ext=0, B=1, m=5), dict(M=1, ext=1, B=0, m=2), dict(M=2, B=1, m=5),
          dict(M=3, ext=0, B=0, m=2), dict(M=3, ext=1, B=1, m=5), dict(M=0, B=1, m=5), dict(M=2, B=0, m=2))


class Case:
    """One eBWT (`lens`, `seed`) with one set of wanted clusters.  lcp(K) is the crafted array, par the smoothing parameters
    (without k), wide the extra entry width of the table path (1, 4 or None: the rotating third)."""

    def __init__(self, name, lens, wanted, par, wide=None, seed=0, raw=None, dips=()):
        self.name, self.lens, self.wanted, self.par, self.wide, self.seed, self.raw = name, lens, wanted, dict(par), wide, seed, raw
        self.dips = tuple(dips)
        self.n = int(sum(lens)) + len(lens)

    def collection(self):
        return skewed(self.lens, 1000 + self.seed)

    def lcp(self, K):
        return self.raw(K) if self.raw else lcp_for(self.n, K, self.wanted, dips=self.dips, seed=self.seed)

    def __repr__(self):
        return self.name


def _wide(i):
    return (1, None, 4)[i % 3]


def _tiny_plain(n, K):
    l = np.full(n, K, np.uint32); l[0] = 0
    return l


def _tiny_last_min(n, K):
    l = _tiny_plain(n, K); l[n - 2] = K + 1
    return l


def _tiny_dip(n, K):
    l = np.full(n, K + 1, np.uint32); l[0] = 0; l[n - 3] = K + 2; l[n - 2] = K
    return l


def tiny_cases():
    """Every n from 1 to 34, one read of n - 1 bases (two reads for a few n), one cluster [0, n-1]; then LCP[n-2] = K + 1
    (the last row would be a minimum if the rule held for it) and a dip at row n - 2 (the last row the rule does hold for)."""
    out = []
    for n in range(1, 35):
        lens = [n - 1] if n % 5 or n < 4 else [n // 2, n - 2 - n // 2]
        plain, last_min, dip = (functools.partial(f, n) for f in (_tiny_plain, _tiny_last_min, _tiny_dip))
        kinds = [("plain", plain)] + ([("lastmin", last_min)] if n >= 3 else []) + ([("dip", dip)] if n >= 4 else [])
        for j, (kind, raw) in enumerate(kinds):
            want = clusters(flags(raw(K2), K2))
            assert want == clusters(flags(raw(K1), K1))
            par = dict(PARAMS[(n + 3 * j) % len(PARAMS)], m=2)
            out.append(Case("tiny_n%d_%s" % (n, kind), lens, want, par, wide=_wide(n + j), seed=n, raw=raw))
    return out


START_ROWS = {-1: (15, 1023, 4095, 8191), 0: (1, 16, 1024, 4096, 8192), 1: (17, 1025, 4097)}
ACROSS = (32, 2048, 12288)                 # a run lies across these rows: found once, not twice
DIPS = (48, 3072, 16384)                   # two clusters touch through a dip here (3072 and 16384: first row of a 1024-row window)
WIN_DIPS = (5000, 6999, 10239)             # more dips on window borders: first row of a 1000-row window, last row of a 1000- / 1024-row one
STEADY = (2999, 7167)                      # a run whose last row is the last row of a 1000- / 1024-row window


def start_cases():
    """Clusters of 2 to 9 rows whose first in() row sits on the lane, wave and chunk borders of k_cluster's start detection."""
    out = []
    n = 40000
    for v, rows in START_ROWS.items():
        want = []
        for i, b in enumerate(rows):
            want.append((b - 1, b - 1 + 1 + (i + v + 1) % 8))            # sizes 2 .. 9
        for x in ACROSS:
            want.append((x - 4 + v, x + 3 + v))
        for d in DIPS + WIN_DIPS:
            want += [(d - 5 - (v + 1), d - 1), (d, d + 2 + (v + 1))]
        for e in STEADY:
            want.append((e - 6, e))
        want.sort()
        out.append(Case("start_%+d" % v, lens_for_rows(n), want, PARAMS[v + 1] if v else dict(PARAMS[1], f=30), wide=_wide(v + 1), seed=40 + v, dips=DIPS + WIN_DIPS))
    return out


def dense_cases():
    """Chunk 1 (rows 4096..8191) full of two-row clusters: 512 starts per wave, eight rounds of the take loop; chunk 2 in
    three-row clusters."""
    want = [(r, r + 1) for r in range(4096, 8192, 2)] + [(r, r + 2) for r in range(8192, 12288 - 2, 3)]
    lens = lens_for_rows(14001)
    return [Case("dense_m2", lens, want, PARAMS[0], wide=1, seed=50), Case("dense_m5", lens, want, PARAMS[1], wide=None, seed=50)]


EMPTY_FRONT = 8                            # empty reads in the "eight-byte steps" collection: rows 0..7 hold terminators only


def step_cases():
    """Every size from 2 to 26 at start rows 0, 1 and 7 modulo 8; m = 5, so sizes below and at m occur.  The cluster [1, 6]
    in front lies on the terminator rows of the empty reads: no base in it at all."""
    want, at = [(1, 6)], 8
    for size in range(2, 27):
        for res in (0, 1, 7):
            at = (at + 7) // 8 * 8 + res
            want.append((at, at + size - 1))
            at += size + 3
    lens = [0] * EMPTY_FRONT + lens_for_rows(at + 100 - EMPTY_FRONT, L=50)
    return [Case("steps8_M3", lens, want, PARAMS[5], wide=4, seed=60), Case("steps8_M1", lens, want, PARAMS[1], wide=1, seed=61)]


BIG_SIZES = (2040, 2041, 2047, 2048, 2049, 2050, 2056, 2057)


def threshold_cases():
    """Both sides of CL_BIG: a cluster is big if and only if it has more than 2048 rows."""
    want, at = [], 64
    for res in (0, 5):
        for size in BIG_SIZES:
            at = (at + 7) // 8 * 8 + res
            want.append((at, at + size - 1))
            at += size + 2
    lens = lens_for_rows(at + 500)
    return [Case("bigthr_M2", lens, want, PARAMS[3], wide=None, seed=70), Case("bigthr_M1_f30", lens, want, dict(PARAMS[2], f=30), wide=4, seed=71)]


def extent_cases():
    """k_big_extent: big clusters whose last row is the last / first row of a 1024-row piece, three whole pieces further on,
    and n - 1 with n = 0, 1 and 1023 modulo 1024; a first in() row that is the last row of a piece and one at 15 modulo 16;
    two big clusters that start in the same chunk."""
    out = []
    P = CL_WROWS
    for i, rem in enumerate((0, 1, 1023)):
        n = 35 * P + rem if rem else 36 * P
        want = [(10, 2049 + 10 - 1), (10 + 2049 + 1, 4 * P + 200),       # two that start in chunk 0
                (7 * P - 2100, 7 * P - 1),                                 # last row = last row of a piece
                (7 * P + 300, 10 * P),                                     # last row = first row of a piece
                (11 * P - 400, 14 * P + 77),                               # 3 whole pieces (11, 12, 13) after its start's piece
                (15 * P - 2, 18 * P - 5),                                  # first in() row = last row of a piece
                (19 * P + 14, 22 * P + 500),                               # first in() row = 15 modulo 16
                (23 * P - 1, 31 * P - 1),                                  # first in() row opens a piece; whole pieces up to its last row
                (n - 2600, n - 1)]                                         # to the end of the arrays
        out.append(Case("extent_n%%1024=%d" % rem, lens_for_rows(n), want, dict(PARAMS[(2 * i + 3) % len(PARAMS)], f=(40, 30, 40)[i]), wide=_wide(i), seed=80 + i))
    return out


def tile_cases():
    """CB_FOR_TILES / CB_FOR_ROWS: one tile exactly, one row more, two tiles and a row from a start at 5 modulo 16; M = 1
    (k_big_decide sums sequentially in row order) and M = 3."""
    a = 1024 + 16
    b = a + CB_TILE + 7
    c = (b + CB_TILE + 1 + 40) // 16 * 16 + 5
    want = [(a, a + CB_TILE - 1), (b, b + CB_TILE), (c, c + 2 * CB_TILE)]
    lens = lens_for_rows(c + 2 * CB_TILE + 1 + 3000)
    return [Case("tiles_M1", lens, want, PARAMS[1], wide=None, seed=90), Case("tiles_M3_f30", lens, want, dict(PARAMS[4], f=30), wide=4, seed=90)]


@functools.lru_cache(maxsize=None)
def part_a():
    return {"tiny": tiny_cases(), "start": start_cases(), "dense": dense_cases(), "steps8": step_cases(),
            "bigthr": threshold_cases(), "extent": extent_cases(), "tiles": tile_cases()}


_ORACLE = {}


def oracle_ext(orc, case, K, **over):
    """(bwt, qs, lcp, parameters with k, (bases, quals, roff, statistics) of the oracle) of a part A case under its crafted
    LCP for K; computed once.  `over` replaces smoothing parameters."""
    key = (case.name, K, tuple(sorted(over.items())))
    if key not in _ORACLE:
        b, q, r = case.collection()
        bwt, qs, _ = orc.build_ebwt(b, q, r)
        lcp = case.lcp(K)
        full = dict(k=K, m=2, v=ord(">"), f=40, t=20, M=2, B=0, ext=0)
        full.update(case.par); full.update(over)
        p = orc.params(K=K, m=full["m"], v=full["v"], f=full["f"], t=full["t"], M=full["M"], B=full["B"], ext=full["ext"])
        want = orc.smooth_invert(bwt, qs, lcp, p) if len(bwt) else None
        for a in (bwt, qs, lcp) + tuple(x for x in (want or ())[:3]):
            a.setflags(write=False)
        _ORACLE[key] = (bwt, qs, lcp, full, want)
    return _ORACLE[key]


def end_cases():
    """The shapes whose last cluster ends at n - 1: "tiny n" above 16 rows and the three of "big extent"."""
    return [c for c in part_a()["tiny"] if c.n > 16] + part_a()["extent"]


# ---------------------------------------------------------------------------------------------------- part B: the cases
U12 = b"GATTACAGCTCA"
# (name, c0, c1, odd, modulus, residue of the cluster's first row)
PART_B = (("b2047_chunk0", 1024, 1019, 4, 4096, 0), ("b2047_chunk4095", 1024, 1019, 4, 4096, 4095),
          ("b2048_chunk0", 1024, 1020, 4, 4096, 0), ("b2048_chunk4095", 1024, 1020, 4, 4096, 4095),
          ("b2049_chunk0", 1024, 1021, 4, 4096, 0), ("b2049_chunk4095", 1024, 1021, 4, 4096, 4095),
          ("b4097_piece1023", 2050, 2043, 4, 1024, 1023), ("b4097_lane5", 2050, 2043, 4, 16, 5),
          ("b65537_piece1023", 33000, 32533, 4, 1024, 1023), ("b65537_lane5", 33000, 32533, 4, 16, 5))
PART_B_PAR = (dict(M=2, B=0, m=5), dict(M=1, B=1, m=5), dict(M=3, B=0, m=2), dict(M=0, B=1, m=5), dict(M=1, B=0, m=2))


def part_b_par(i):
    return dict(PART_B_PAR[i % len(PART_B_PAR)], k=len(U12))
