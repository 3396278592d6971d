"""The LCP deduction from the eBWT (k_bfs.hip: k_rankblocks, k_bfs_init, k_bfs_level<SIDE>, k_bfs_fill and the launch loop of
bfq_lcp_from_bwt) on inputs that put its special cases there by construction (tests/bfs_cases.py), the deduced array itself
held to the CPU reference value for value.  Never one GPU path against another.

Table path: after smooth_invert(bwt, qs) without an LCP the context keeps the given eBWT and the 16-bit LCP array that
bfq_lcp_from_bwt wrote (nothing allocated later lies below it in the arena and its one reader, k_lcp_flags, takes it const), so
fetch_ebwt returns it: compared with oracle.orc.lcp_from_bwt -- or family U's closed form -- over all n entries, and the reads,
offsets and eight statistics with oracle.orc.smooth_invert(bwt, qs, None, p).
Compact path (BFQ_COMPACT=1; the ring unset = the plain log, and BFQ_COMPACT_RING): the 16-bit array is released once the flags
exist, so reads, offsets and statistics are compared, at several k per case such that the levels the case is about lie on both
sides of some k.
tests/test_bfs_cases_host.py asserts without a GPU that the geometries named here are really in these inputs."""
import re
import numpy as np
import pytest
from bfqzip_amd import api
from tests import bfs_cases as bc
from tests import util

pytestmark = pytest.mark.gpu
ENV = ("BFQ_COMPACT", "BFQ_COMPACT_RING", "BFQ_TRACE")
RING_LINE = re.compile(r"interval refinement: ring of (\d+) entries for (\d+) rows, at most (\d+) launches per level(, finished in host memory)?")


def _par(i):
    """smoothing mode and binning rotate over the cases"""
    return dict(M=i % 4, B=(i // 4) % 2, m=2)


def _same(got, want, what):
    gb, gq, groff, gst = got
    eb, eq, eroff, est = want
    assert np.array_equal(gb, eb), ("bases",) + what
    assert np.array_equal(gq, eq), ("quals",) + what
    assert np.array_equal(groff, eroff), ("roff",) + what
    assert len(est) == 8
    for k in est:
        assert est[k] == gst[k], (k, est[k], gst[k]) + what


def _lcp_same(e, n, want, what):
    got = np.empty(n, np.uint16)
    e.fetch_ebwt(n, out=(None, None, got))
    got = got.astype(np.uint32)
    d = np.flatnonzero(got != want)
    assert len(want) == n and not len(d), what + ("%d rows differ, the first: row %d holds %d, the reference %d" % (
        len(d), int(d[0]), int(got[d[0]]), int(want[d[0]])),)


def _wants(orc, bwt, qs, ks, par):
    """the oracle's reads, offsets and statistics per k: computed once, shared by every path"""
    return {k: orc.smooth_invert(bwt, qs, None, orc.params(K=k, m=par["m"], M=par["M"], B=par["B"])) for k in ks}


def _clear(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def _paths(e, orc, monkeypatch, bwt, qs, lcp, ks, par, what, rings=(None, "64"), compact_ks=None):
    """One eBWT through the table path (LCP value for value, outputs) and the compact path (outputs) of `e`."""
    wants = _wants(orc, bwt, qs, ks, par)
    n = len(bwt)
    try:
        _clear(monkeypatch)
        for k in ks:
            e.set_params(k=k, **par)                                      # (the environment is read here)
            got = e.smooth_invert(bwt, qs)
            _lcp_same(e, n, lcp, what + ("table", k))
            _same(got, wants[k], what + ("table", k))
        monkeypatch.setenv("BFQ_COMPACT", "1")
        for ring in rings:
            if ring is None:
                monkeypatch.delenv("BFQ_COMPACT_RING", raising=False)
            else:
                monkeypatch.setenv("BFQ_COMPACT_RING", ring)
            for k in (ks if compact_ks is None else compact_ks):
                e.set_params(k=k, **par)
                _same(e.smooth_invert(bwt, qs), wants[k], what + ("compact", ring, k))
    finally:
        _clear(monkeypatch)
        e.set_params()


def _unary_case(e, orc, monkeypatch, M, L, i):
    bwt, lcp = bc.unary(M, L)
    qs = bc.quals_for(bwt, 7 * M + L)
    assert np.array_equal(orc.lcp_from_bwt(bwt), lcp)                    # the closed form is the reference's
    _paths(e, orc, monkeypatch, bwt, qs, lcp, bc.unary_ks(M, L), _par(i), ("U", M, L))


def _sibling_case(e, orc, monkeypatch, acg, i):
    bwt, qs, lcp = orc.build_ebwt(*bc.siblings(*acg))
    for shuffled in (False, True):
        sb, sq = bwt, qs
        for seed in range(20 if shuffled else 0):                       # (a permutation may leave an 8-row block's symbols in place)
            sb, sq = util.shuffle_ties(bwt, qs, np.random.default_rng(seed))
            if not np.array_equal(sb, bwt):
                break
        assert shuffled == (not np.array_equal(sb, bwt))
        _paths(e, orc, monkeypatch, sb, sq, orc.lcp_from_bwt(sb), bc.SIBLING_KS, _par(i + shuffled), ("T", acg, shuffled))


@pytest.mark.parametrize("i", range(len(bc.FILL_BORDERS)), ids=["M%d_L%d" % ml for ml in bc.FILL_BORDERS])
def test_fill_borders(engine, orc, monkeypatch, i):
    """M copies of A^70: a leaf block with M - 1 = 0, 1, 2, 3, 63, 64, 65, 66 inner boundaries at every level -- none, the two
    direct stores, the wave-wide fill up to its last lane, k_bfs_fill from its first size on.  With M = 65 the blocks start at
    every residue modulo 64; with M = 64 both rank ends sit on a block's first row (occ5 at p & 63 == 0)."""
    M, L = bc.FILL_BORDERS[i]
    _unary_case(engine, orc, monkeypatch, M, L, i)


@pytest.mark.parametrize("i", range(len(bc.ARRAY_ENDS)), ids=["M%d_L%d" % ml for ml in bc.ARRAY_ENDS])
def test_array_ends(engine, orc, monkeypatch, i):
    """n = 63 .. 65 and 255 .. 257 with one row per level, terminators only (n = 1, 64, 256: nothing to extend) and n = 256 in
    blocks of 64: the rank block at index n / 64 and the group n / 256 when n is a multiple of them, lcp[n] beside the last row."""
    M, L = bc.ARRAY_ENDS[i]
    _unary_case(engine, orc, monkeypatch, M, L, i + 1)


@pytest.mark.parametrize("i", range(len(bc.SIBLINGS)), ids=["a%d_c%d_g%d" % acg for acg in bc.SIBLINGS])
def test_sibling_blocks(engine, orc, monkeypatch, i):
    """a, c, g copies of A+u, C+u, G+u: ONE thread extends the block u# into two or three sibling blocks that take the direct
    stores, the pending wave-wide fill, the serial loop behind it and the fill list, in first, second and third place; as built
    and with the ties shuffled (the A, C and G rows interleaved in the parent block)."""
    _sibling_case(engine, orc, monkeypatch, bc.SIBLINGS[i], i)


def test_depth_limit(engine, orc, monkeypatch):
    """Two copies of A^65000 (BFQ_MAX_READ_LEN): 65 001 levels of one interval, each a launch and a synchronisation (1.3 s per
    call on the MI355X), the last LCP values 64 999 and 65 000 next to LCP_UNSET (0xFFFF).  k = 65 000: only the last row is
    inside.  Table path with the LCP values, and the compact path with a ring of 64 entries, which the 65 001 entries go round
    a thousand times (the ring unset is the log of the table path again)."""
    M, L = bc.DEPTH
    bwt, lcp = bc.unary(M, L)
    qs = bc.quals_for(bwt, 3)
    par = dict(M=2, B=0, m=2)
    want = _wants(orc, bwt, qs, (L,), par)[L]
    assert int(lcp.max()) == L and want[3]["num_clust"] == 1
    try:
        _clear(monkeypatch)
        engine.set_params(k=L, **par)
        got = engine.smooth_invert(bwt, qs)
        _lcp_same(engine, len(bwt), lcp, ("U", M, L, "table"))
        _same(got, want, ("U", M, L, "table"))
        monkeypatch.setenv("BFQ_COMPACT", "1")
        monkeypatch.setenv("BFQ_COMPACT_RING", "64")
        engine.set_params(k=L, **par)
        _same(engine.smooth_invert(bwt, qs), want, ("U", M, L, "compact", "64"))
    finally:
        _clear(monkeypatch)
        engine.set_params()


@pytest.mark.parametrize("M", [m for m, _l in bc.SIDE_LISTS], ids=["2p25", "2p25_plus_1"])
def test_side_lists(engine, monkeypatch, M):
    """M reads 'A' (n = 2 M rows).  M = 2^25: rb - lb == BQ_LEN_MAX, still packed.  M = 2^25 + 1: both level-0 intervals go to
    the side list in k_bfs_init, k_bfs_level<true> extends them, hands a block of 2^25 inner boundaries to k_bfs_fill and puts
    the child on the next side list.  k = 2: no LCP value reaches it, so the reads come back as given and every statistic is 0
    (no oracle run at this size); the LCP is the closed form.  Table path only."""
    bwt, lcp = bc.unary(M, 1)
    qs = np.full(2 * M, ord("#"), np.uint8)
    qs[:M] = (np.arange(M) % 41 + 33).astype(np.uint8)
    try:
        _clear(monkeypatch)
        engine.set_params(k=2, M=2, B=0, m=2)
        gb, gq, groff, gst = engine.smooth_invert(bwt, qs)
        _lcp_same(engine, 2 * M, lcp, ("U", M, 1))
        assert int(lcp.max()) == 1
        assert len(gb) == M and (gb == ord("A")).all()
        assert np.array_equal(gq, qs[:M])                               # read i ends on terminator-suffix row i
        assert np.array_equal(groff, np.arange(M + 1, dtype=np.uint64))
        for key in util.STAT_KEYS:
            assert gst[key] == 0, key
    finally:
        engine.set_params()


@pytest.fixture(scope="module")
def wide(orc):
    """family R as built and tie-shuffled with the reference's LCP, and what the oracle makes of both: once for the module"""
    b, q, r = bc.wide()
    bwt, qs, lcp, sa = orc.build_ebwt(b, q, r, want_sa=True)
    sb, sq = bc.shuffle_ties(bwt, qs, lcp, sa, r, np.random.default_rng(3))
    out = []
    for x, y in ((bwt, qs), (sb, sq)):
        ref = orc.lcp_from_bwt(x)
        assert np.array_equal(ref, lcp)
        for a in (x, y, ref):
            a.setflags(write=False)
        out.append((x, y, ref))
    return out


WIDE_KS = (5, 8, 11, 16)       # levels 5 .. 10 hold the tens of thousands of intervals


@pytest.mark.parametrize("shuffled", [0, 1], ids=["built", "ties"])
def test_stage_and_ring(engine, orc, monkeypatch, capfd, wide, shuffled):
    """4000 reads of 100 bases from both strands of a 100 kb genome (n = 404 000): levels of tens of thousands of intervals with
    four children each, so every workgroup flushes its 4096-entry stage inside the loop and a level is many grid strides of a
    ring's chunks.  Table path with the LCP values; compact path with the plain log and three rings, the route each ring took
    read from the library's own trace line: a 64-entry ring ends in host memory at once, one size takes a level in two
    launches or more and stays on the device, one does so and then moves to host memory."""
    bwt, qs, lcp = wide[shuffled]
    par = dict(M=1 + shuffled, B=shuffled, m=3)
    n = len(bwt)
    wants = _wants(orc, bwt, qs, WIDE_KS, par)
    assert all(w[3]["num_clust"] > 0 for w in wants.values())
    seen = []
    try:
        _clear(monkeypatch)
        for k in WIDE_KS:
            engine.set_params(k=k, **par)
            got = engine.smooth_invert(bwt, qs)
            _lcp_same(engine, n, lcp, ("R", shuffled, "table", k))
            _same(got, wants[k], ("R", shuffled, "table", k))
        monkeypatch.setenv("BFQ_COMPACT", "1")
        monkeypatch.setenv("BFQ_TRACE", "1")
        for ring, route in ((None, "log"), (64, "host"), (bc.WIDE_RINGS["chunks"], "chunks"), (bc.WIDE_RINGS["host"], "host")):
            if ring is None:
                monkeypatch.delenv("BFQ_COMPACT_RING", raising=False)
            else:
                monkeypatch.setenv("BFQ_COMPACT_RING", str(ring))
            for k in WIDE_KS:
                engine.set_params(k=k, **par)
                capfd.readouterr()
                got = engine.smooth_invert(bwt, qs)
                lines = [m for m in map(RING_LINE.search, capfd.readouterr().err.splitlines()) if m]
                seen.append("ring %s, k %d: %s" % (ring, k, [m.group(0) for m in lines]))
                _same(got, wants[k], ("R", shuffled, "compact", ring, k))
                if route == "log":
                    assert not lines                                    # no ring: the log of n entries
                    continue
                assert len(lines) == 1 and int(lines[0].group(1)) == ring and int(lines[0].group(2)) == n
                launches, host = int(lines[0].group(3)), lines[0].group(4) is not None
                assert host == (route == "host"), (ring, lines[0].group(0))
                if ring != 64:
                    assert launches >= 2, (ring, lines[0].group(0))
        print("\n".join(seen))                                          # (capfd.readouterr() above drops what was printed before it)
    finally:
        _clear(monkeypatch)
        engine.set_params()


@pytest.mark.parametrize("byte", [0xFF, 0x00], ids=["0xFF", "0x00"])
def test_poisoned_workspace(orc, monkeypatch, byte):
    """On an engine whose workspace holds `byte` before every call: n = 64, 256, 257 with one row per level, one empty read
    (n = 1) and the three sibling blocks of 65 rows.  0x00: an LCP entry that the explicit 0xFF fill missed reads as claimed
    with level 0.  0xFF: a rank block, queue slot or list entry read beyond what was built is all ones."""
    from tests.test_gpu_poison import poisoned
    with poisoned(byte):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 16)
            assert e.workspace_bytes() > 0 and (e.workspace_read(0, 1 << 16) == byte).all()     # the switch is on for this engine
            for i, (M, L) in enumerate(bc.POISON_ENDS):
                _unary_case(e, orc, monkeypatch, M, L, i)
            _sibling_case(e, orc, monkeypatch, bc.POISON_SIBLINGS, 2)
        finally:
            e.close()
