"""Designed inputs for the LCP deduction from the eBWT (k_bfs.hip) and a numpy model of its geometry: which of the kernel's
special cases a given eBWT reaches.  tests/bfs_model.py's bfs() is the specification of the algorithm; geometry() below is the
same refinement vectorised per level (held to bfs() in tests/test_bfs_cases_host.py) that also records what the kernel does
with every interval: the inner-boundary route of every leaf block, side-list entries, one or two rank blocks per interval,
the LDS stage's flushes inside the loop, and -- for a ring size -- the route of bfq_lcp_from_bwt's launch loop.
Test infrastructure (tests/test_gpu_lcp_deduce.py on the GPU, tests/test_bfs_cases_host.py without one).

Family U (unary): M copies of the read A^L.  n = M (L + 1), bwt = 'A' * (M L) + '#' * M, and with j = row // M the LCP is j
inside a block of M rows, max(j, 1) - 1 at a block's first row, 0 at row 0: a closed form, no sort needed.  Every level j has
one leaf block with M - 1 inner boundaries, starting at row j M.
Family T (siblings): a 12-mer u without repeated 3-mers in a copies of A+u, c of C+u, g of G+u.  The leaf block u# then has
three children Au#, Cu#, Gu# with a - 1, c - 1, g - 1 inner boundaries, extended by ONE thread in that order.
Family R (wide levels): random reads of a random genome, both strands: levels of tens of thousands of intervals with four
children each."""
import numpy as np

TERM = ord("#")
SYMS = np.frombuffer(b"ACGNT", np.uint8)
LEN_MAX = (1 << 25) - 1                 # BQ_LEN_MAX: rb - lb values up to here fit the packed queue entry
FILL_INLINE = 64                        # BQ_FILL_INLINE
STAGE = 4096                            # BQ_STAGE
PER_GROUP = 2048                        # parents per workgroup of k_bfs_level<false>: bfq_grid(cnt, 256 * 8)
MAX_GRID = 1 << 19                      # BFQ_MAX_GRID
MAX_READ_LEN = 65000                    # BFQ_MAX_READ_LEN
ROUTES = ("direct", "inline", "serial", "fill")
UNSET = 0xFFFF

U12 = b"CATGGTCAGTTA"                   # no 3-mer twice (asserted in the host test)

# ---------------------------------------------------------------------------------------------------- the cases
FILL_BORDERS = [(M, 70) for M in (1, 2, 3, 4, 64, 65, 66, 67)]
ARRAY_ENDS = [(1, L) for L in (62, 63, 64, 254, 255, 256)] + [(M, 0) for M in (1, 64, 256)] + [(64, 3)]
DEPTH = (2, MAX_READ_LEN)
SIDE_LISTS = [(1 << 25, 1), ((1 << 25) + 1, 1)]
# the last two are this file's own: no listed case puts a fill-list block (more than 64 inner boundaries) behind a sibling
SIBLINGS = [(3, 4, 0), (4, 3, 0), (4, 4, 0), (65, 4, 0), (4, 65, 0), (65, 65, 0), (65, 65, 65), (66, 2, 1), (4, 66, 0), (66, 66, 0)]
# rings for family R (n = 404 000): levels in several launches with the queue on the device / moved to host memory after such
# launches; tests/test_bfs_cases_host.py holds ring_route() to these names 10 % either side
WIDE_RINGS = {"chunks": 200_000, "host": 75_000}
POISON_ENDS =[(1, 63), (1, 255), (1, 256), (1, 0)]     # n = 64, 256, 257, and one empty read
POISON_SIBLINGS = (65, 65, 65)


def unary(M, L):
    """(bwt, lcp) of M copies of A^L: the closed form."""
    n = M * (L + 1)
    bwt = np.full(n, ord("A"), np.uint8)
    bwt[M * L:] = TERM
    row = np.arange(n, dtype=np.int64)
    j = row // M
    lcp = np.where(row % M == 0, np.maximum(j, 1) - 1, j)
    lcp[0] = 0
    return bwt, lcp.astype(np.uint32)


def quals_for(bwt, seed):
    """qualities for a closed-form eBWT: anything on the base rows, '#' on the terminator rows (as the oracle's builder)"""
    q = np.random.default_rng(seed).integers(33, 74, len(bwt)).astype(np.uint8)
    q[np.asarray(bwt) == TERM] = ord("#")
    return q


def unary_ks(M, L):
    """k values for the output comparison of U(M, L): every level 1 .. L is >= 1 and < L + 1, and the middle splits them"""
    return sorted({1, max(L // 2, 1), max(L, 1), L + 1})


def siblings(a, c, g, seed=0):
    """(bases, quals, roff) of family T, the reads shuffled"""
    rng = np.random.default_rng(1000 + 97 * a + 11 * c + g + seed)
    reads = [b"A" + U12] * a + [b"C" + U12] * c + [b"G" + U12] * g
    reads = [reads[i] for i in rng.permutation(len(reads))]
    b = np.frombuffer(b"".join(reads), np.uint8).copy()
    q = rng.integers(33, 74, len(b)).astype(np.uint8)
    r = np.arange(len(reads) + 1, dtype=np.uint64) * (len(U12) + 1)
    return b, q, r


SIBLING_KS = (len(U12), len(U12) + 1, len(U12) + 2)     # the children's level is 13, their parent's 12


def wide(seed=20251021, nreads=4000, L=100, glen=100_000):
    """(bases, quals, roff) of family R: reads of both strands of a random genome, a few N, 5 % duplicates"""
    rng = np.random.default_rng(seed)
    g = SYMS[[0, 1, 2, 4]][rng.integers(0, 4, glen)]
    comp = np.zeros(256, np.uint8)
    for x, y in zip(b"ACGTN", b"TGCAN"):
        comp[x] = y
    reads = []
    for _ in range(nreads):
        if reads and rng.random() < 0.05:
            reads.append(reads[int(rng.integers(0, len(reads)))])
            continue
        s = int(rng.integers(0, glen - L + 1))
        x = g[s:s + L].copy()
        if rng.random() < 0.5:
            x = comp[x[::-1]]
        x[rng.random(L) < 0.002] = ord("N")
        reads.append(x)
    b = np.concatenate(reads)
    q = rng.integers(33, 74, len(b)).astype(np.uint8)
    r = np.arange(nreads + 1, dtype=np.uint64) * L
    return b, q, r


def shuffle_ties(bwt, qs, lcp, sa, roff, rng):
    """tests/util.py's shuffle_ties without decoding the rows (for 4 * 10^5 of them): rows r - 1 and r hold identical suffixes
    when LCP[r] equals both their lengths; sa and lcp as oracle.orc.build_ebwt(..., want_sa=True) returns them."""
    roff = np.asarray(roff, np.int64)
    ends = roff[1:] + np.arange(len(roff) - 1)                  # text position of every read's terminator
    sa = np.asarray(sa, np.int64)
    slen = ends[np.searchsorted(ends, sa, "left")] - sa
    same = np.zeros(len(sa), bool)
    same[1:] = (np.asarray(lcp, np.int64)[1:] == slen[1:]) & (slen[1:] == slen[:-1])
    block = np.cumsum(~same)
    order = np.lexsort((rng.random(len(sa)), block))
    return np.asarray(bwt)[order].copy(), np.asarray(qs)[order].copy()


# ---------------------------------------------------------------------------------------------------- the model
class Geometry:
    """lcp: int64[n] (UNSET where nothing was written); level_sizes[l]: queue entries read at level l + 1 (packed ones; the
    side list's are side_sizes[l]); kids[l]: packed children of every such entry, in queue order; routes[(route, position)]:
    leaf blocks with inner boundaries by their route and their place among their parent's children; side: intervals that went
    to a side list (the level-0 ones included); one_block / two_blocks: lb & 63 of the intervals whose two rank ends lay in
    one 64-row block / in two; flushes[l]: stage flushes inside the loop, summed over the workgroups of that level's one
    launch; kids_per_group[l]: the most children any workgroup of that launch stages."""


def _grid(items, per):
    return int(min(max(-(-items // per), 1), MAX_GRID))


def _stage(kids):
    """(flushes inside the loop, most children of one workgroup) of k_bfs_level<false> over parents with these children"""
    cnt = len(kids)
    if not cnt:
        return 0, 0
    grid = _grid(cnt, PER_GROUP)
    stride = grid * 256
    rounds = -(-cnt // stride)
    pad = np.zeros(rounds * stride, np.int64)
    pad[:cnt] = kids
    tot = pad.reshape(rounds, grid, 256).sum(axis=2)            # thread t of group b takes parent it * stride + 256 b + t
    used = np.zeros(grid, np.int64)
    flushes = 0
    for it in range(rounds):
        fl = used + tot[it] > STAGE
        flushes += int(fl.sum())
        used[fl] = 0
        used += tot[it]
    return flushes, int(tot.sum(axis=0).max())


def geometry(bwt, term=TERM):
    bwt = np.asarray(bwt, np.uint8)
    n = len(bwt)
    N = int(np.count_nonzero(bwt == term))
    pre = np.zeros((5, n + 1), np.int64)
    for ci, s in enumerate(SYMS):
        np.cumsum(bwt == s, out=pre[ci, 1:])
    tot = pre[:, n]
    assert N + int(tot.sum()) == n
    F = N + np.concatenate([[0], np.cumsum(tot)[:-1]])
    g = Geometry()
    lcp = np.full(n + 1, UNSET, np.int64)
    lcp[0] = 0
    lcp[n] = 0
    g.routes = {}
    g.side = 0
    g.one_block, g.two_blocks = set(), set()
    g.level_sizes, g.side_sizes, g.kids, g.flushes, g.kids_per_group = [], [], [], [], []
    q, sq = [], []                                              # (lb, rb, leaf): the packed queue, the side list
    if N:
        lcp[:N + 1] = 0
        (q if N - 1 <= LEN_MAX else sq).append((0, N - 1, 1))
    for ci in range(5):
        if tot[ci]:
            lcp[F[ci] + tot[ci]] = 0
            (q if tot[ci] - 1 <= LEN_MAX else sq).append((F[ci], F[ci] + tot[ci] - 1, 0))
    g.side += len(sq)
    q = np.array(q, np.int64).reshape(-1, 3)
    sq = np.array(sq, np.int64).reshape(-1, 3)
    level = 1
    while len(q) or len(sq):
        assert level <= MAX_READ_LEN + 2
        nq, nsq, kids_here = [], [], None
        for part, is_side in ((q, False), (sq, True)):
            lb, rb, leaf = part[:, 0], part[:, 1], part[:, 2].astype(bool)
            one = (lb >> 6) == ((rb + 1) >> 6)
            g.one_block |= set((lb[one] & 63).tolist())
            g.two_blocks |= set((lb[~one] & 63).tolist())
            P = len(part)
            pending = np.zeros(P, bool)                         # the thread's one inline fill is taken
            place = np.zeros(P, np.int64)                       # children so far
            enq = np.zeros((P, 5), bool)
            long_ = np.zeros((P, 5), bool)
            klb = np.zeros((P, 5), np.int64)
            krb = np.zeros((P, 5), np.int64)
            for ci in range(5):
                a, b = pre[ci][lb], pre[ci][rb + 1]
                ok = b > a
                nlb, nrb = F[ci] + a, F[ci] + b - 1
                claim = ok.copy()
                claim[ok] = lcp[nrb[ok] + 1] == UNSET
                lcp[nrb[claim] + 1] = level                     # (children of one level are disjoint: no slot twice)
                inner = nrb - nlb
                wide_ = ok & leaf & (inner > 0)
                if wide_.any():
                    w = np.flatnonzero(wide_)
                    cnts = inner[w]
                    starts = np.repeat(nlb[w] + 1 - (np.cumsum(cnts) - cnts), cnts) + np.arange(int(cnts.sum()))
                    assert (lcp[starts] == UNSET).all(), "inner boundary already set"
                    lcp[starts] = level
                    route = np.where(inner <= 2, 0, np.where(inner <= FILL_INLINE, np.where(pending, 2, 1), 3))
                    for r_ in range(4):
                        for pl in np.unique(place[wide_ & (route == r_)]).tolist():
                            key = (ROUTES[r_], pl)
                            g.routes[key] = g.routes.get(key, 0) + int(np.count_nonzero(wide_ & (route == r_) & (place == pl)))
                    pending |= wide_ & (route == 1)
                place += ok
                e = claim | wide_
                enq[:, ci] = e
                long_[:, ci] = e & (inner > LEN_MAX)
                klb[:, ci], krb[:, ci] = nlb, nrb
            packed = enq & ~long_
            kl = np.broadcast_to(leaf[:, None], (P, 5))
            nq.append(np.stack([klb[packed], krb[packed], kl[packed]], axis=1))     # parent by parent, symbols in order
            nsq.append(np.stack([klb[long_], krb[long_], kl[long_]], axis=1))
            if not is_side:
                kids_here = packed.sum(axis=1)
        g.level_sizes.append(len(q))
        g.side_sizes.append(len(sq))
        g.kids.append(kids_here)
        fl, most = _stage(kids_here)
        g.flushes.append(fl)
        g.kids_per_group.append(most)
        q = np.concatenate(nq).astype(np.int64).reshape(-1, 3)
        sq = np.concatenate(nsq).astype(np.int64).reshape(-1, 3)
        g.side += len(sq)
        level += 1
    g.lcp = lcp[:n]
    g.levels = level - 1
    g.n = n
    return g


def side_list_arithmetic(M):
    """family U with L = 1 and M reads, by arithmetic alone (2^25 rows are not modelled row by row): the two level-0 intervals
    ('#' block and the A interval) hold M rows each, rb - lb = M - 1; level 1 makes of the '#' block the leaf block A# of M
    rows (M - 1 inner boundaries) and of the A interval nothing new (its A rows are none: the A suffixes are preceded by #).
    Returns (rb - lb of the level-0 intervals, side-list entries of level 0, of level 1, inner boundaries of the one block)."""
    d = M - 1
    return d, (2 if d > LEN_MAX else 0), (1 if d > LEN_MAX else 0), M - 1


def ring_route(g, ring):
    """bfq_lcp_from_bwt's launch loop for a ring of `ring` entries, restated on the model's queue (parents in the model's
    order): ('log' | 'one' | 'chunks' | 'host', most launches per level).  'log': as large as the log, no ring at all;
    'one': every level in one launch; 'chunks': some level in two launches or more, the queue stays on the device; 'host':
    the queue moved to pinned host memory."""
    n = g.n
    if ring and ring < 64:
        ring = 64
    if not ring or ring >= n + 64:
        return "log", 1
    qsize = ring
    tail = g.level_sizes[0]
    qbeg, qend = 0, tail
    chunks_max, host = 1, False
    for l in range(g.levels):
        kids = g.kids[l]
        nside = g.side_sizes[l]
        assert qend - qbeg == len(kids)
        pb = qbeg
        if qsize:
            side_room = 5 * nside
            if qsize - (tail - pb) < side_room:
                host, qsize = True, 0
            chunks = 0
            while qsize and pb < qend:
                rem, room = qend - pb, qsize - (tail - pb) - side_room
                chunk = room // 5
                if chunk < rem and chunk < max(rem // 64, 4096):
                    host, qsize = True, 0
                    break
                chunk = min(chunk, rem)
                tail += int(kids[pb - qbeg:pb - qbeg + chunk].sum())
                pb += chunk
                chunks += 1
            chunks_max = max(chunks_max, chunks)
        nxt = g.level_sizes[l + 1] if l + 1 < g.levels else 0
        tail = qend + nxt                                       # the rest of the level and the side list's intervals done
        qbeg, qend = qend, tail
    return ("host" if host else "chunks" if chunks_max >= 2 else "one"), chunks_max
