"""What tests/test_gpu_lcp_deduce.py rests on, checked without a GPU: the reference (oracle.orc.lcp_from_bwt) agrees with the
LCP of the oracle's own builder and with family U's closed form, tests/bfs_cases.py's geometry() computes what
tests/bfs_model.py's bfs() specifies, and every geometry of k_bfs.hip that the GPU module names is really in its inputs."""
import numpy as np
import pytest
from tests import bfs_cases as bc
from tests import bfs_model as bm
from tests import util

SMALL_U = bc.FILL_BORDERS + bc.ARRAY_ENDS + [(2, 7), (3, 1), (4, 9), (66, 3), (64, 64)]


@pytest.fixture(scope="module")
def fam_u():
    return {ml: bc.geometry(bc.unary(*ml)[0]) for ml in bc.FILL_BORDERS + bc.ARRAY_ENDS}


@pytest.fixture(scope="module")
def fam_t(orc):
    out = {}
    for acg in bc.SIBLINGS:
        bwt, qs, lcp = orc.build_ebwt(*bc.siblings(*acg))
        out[acg] = (bwt, qs, lcp, bc.geometry(bwt))
    return out


@pytest.fixture(scope="module")
def fam_r(orc):
    b, q, r = bc.wide()
    bwt, qs, lcp, sa = orc.build_ebwt(b, q, r, want_sa=True)
    sb, sq = bc.shuffle_ties(bwt, qs, lcp, sa, r, np.random.default_rng(3))
    return bwt, qs, lcp, sb, sq, bc.geometry(bwt), bc.geometry(sb)


# ---------------------------------------------------------------------------------------------------- the reference
def test_reference_equals_the_builders_lcp(orc):
    """50 random collections with duplicates, N and empty reads: the LCP located by LF walks is the LCP of the sorted suffixes,
    as built and with the ties shuffled"""
    rng = np.random.default_rng(2025)
    shuffled = 0
    for it in range(50):
        b, q, r = util.random_reads(rng, int(rng.integers(1, 120)), 0 if it % 5 == 0 else 1, int(rng.integers(1, 40)), dup=0.4)
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        if not len(bwt):
            continue
        assert np.array_equal(orc.lcp_from_bwt(bwt), lcp), it
        sb, _sq = util.shuffle_ties(bwt, qs, rng)
        shuffled += int(not np.array_equal(sb, bwt))
        assert np.array_equal(orc.lcp_from_bwt(sb), lcp), it
    assert shuffled >= 25


@pytest.mark.parametrize("ml", SMALL_U, ids=lambda ml: "M%d_L%d" % ml)
def test_closed_form_of_family_u(orc, ml):
    bwt, lcp = bc.unary(*ml)
    assert len(bwt) == ml[0] * (ml[1] + 1) and lcp.dtype == np.uint32
    assert np.array_equal(orc.lcp_from_bwt(bwt), lcp)
    assert np.array_equal(bc.geometry(bwt).lcp, lcp)


# ---------------------------------------------------------------------------------------------------- the model
def test_geometry_is_the_specified_refinement():
    """geometry() against bfs_model.bfs(): the same LCP and the same number of intervals, on small collections as built and
    with ties in inconsistent order"""
    rng = np.random.default_rng(5)
    tested = 0
    for it in range(300):
        glen = int(rng.integers(2, 12))
        g = "".join(rng.choice(list("ACGT"), glen))
        reads = []
        for _ in range(int(rng.integers(1, 14))):
            if reads and rng.random() < 0.35:
                reads.append(reads[int(rng.integers(0, len(reads)))])
                continue
            L = int(rng.integers(0, glen + 1)); s = int(rng.integers(0, glen - L + 1))
            x = list(g[s:s + L])
            for k in range(len(x)):
                if rng.random() < 0.08:
                    x[k] = str(rng.choice(list("ACGTN")))
            reads.append("".join(x))
        for shuffle in (False, True):
            bwt = bm.ebwt(reads, rng, shuffle)
            if bm.decode(bwt)[0] is None:
                continue
            want, work = bm.bfs(bwt)
            geo = bc.geometry(np.frombuffer("".join(bwt).encode(), np.uint8))
            assert geo.lcp.tolist() == want, (reads, shuffle)
            assert sum(geo.level_sizes) + sum(geo.side_sizes) == work
            tested += 1
    assert tested >= 500


def test_geometry_on_the_designed_families(orc, fam_t, fam_r):
    for acg, (bwt, qs, lcp, geo) in fam_t.items():
        assert len(bwt) <= 3000
        assert np.array_equal(geo.lcp, lcp) and np.array_equal(orc.lcp_from_bwt(bwt), lcp), acg
        sb, _sq = util.shuffle_ties(bwt, qs, np.random.default_rng(1))
        assert not np.array_equal(sb, bwt) and np.array_equal(orc.lcp_from_bwt(sb), lcp), acg
    bwt, qs, lcp, sb, sq, geo, geo_s = fam_r
    assert 350_000 <= len(bwt) <= 450_000
    assert np.array_equal(geo.lcp, lcp) and np.array_equal(geo_s.lcp, lcp)
    assert np.array_equal(orc.lcp_from_bwt(bwt), lcp) and np.array_equal(orc.lcp_from_bwt(sb), lcp)
    assert int((sb != bwt).sum()) > 1000                       # the A, C, G, T rows of the duplicates' blocks are interleaved
    assert np.array_equal(np.sort(sq), np.sort(qs))


# ---------------------------------------------------------------------------------------------------- the geometries
def test_u12_has_no_repeated_3mer():
    u = bc.U12
    assert len(u) == 12 and len({u[i:i + 3] for i in range(10)}) == 10


def test_sibling_routes_in_every_place(fam_t):
    """One thread extends the block u# by A, C and G in that order.  Direct stores, the pending fill and the fill list occur in
    first and in second place; the serial loop needs the pending fill taken, so its places are second and third."""
    seen = {}
    for acg, (_bwt, _qs, _lcp, geo) in fam_t.items():
        for key, cnt in geo.routes.items():
            seen.setdefault(key, []).append(acg)
    for key in (("direct", 0), ("direct", 1), ("inline", 0), ("inline", 1), ("serial", 1), ("serial", 2), ("fill", 0), ("fill", 1)):
        assert key in seen, key
    assert ("serial", 0) not in seen
    assert seen[("direct", 0)] == [(3, 4, 0)] and seen[("inline", 1)] == [(3, 4, 0)]
    assert set(seen[("direct", 1)]) == {(4, 3, 0), (66, 2, 1)}
    assert set(seen[("serial", 1)]) == {(4, 4, 0), (65, 4, 0), (4, 65, 0), (65, 65, 0), (65, 65, 65)} and seen[("serial", 2)] == [(65, 65, 65)]
    assert set(seen[("fill", 1)]) == {(4, 66, 0), (66, 66, 0)}
    # 64 inner boundaries through the pending fill and through the serial loop
    assert fam_t[(65, 4, 0)][3].routes[("inline", 0)] == 1 and fam_t[(4, 65, 0)][3].routes[("serial", 1)] == 1


def test_inner_boundaries_of_family_u(fam_u):
    """M - 1 inner boundaries at every one of the 70 levels: 0, 1, 2 (none / direct), 3, 63, 64 (the wave-wide fill), 65, 66
    (the fill list)"""
    want = {1: None, 2: "direct", 3: "direct", 4: "inline", 64: "inline", 65: "inline", 66: "fill", 67: "fill"}
    assert [M - 1 for M, _L in bc.FILL_BORDERS] == [0, 1, 2, 3, 63, 64, 65, 66]
    for M, route in want.items():
        geo = fam_u[(M, 70)]
        assert geo.routes == ({(route, 0): 70} if route else {}), (M, geo.routes)
        assert geo.levels in (70, 71) and geo.side == 0


def test_rank_ends_in_one_block_and_in_two(fam_u):
    """U(65, 70): blocks of 65 rows start at every residue modulo 64, their two ends always in two rank blocks (65 rows never
    fit one).  Both ends in one block: every residue but 63 (rb + 1 > lb: from lb & 63 == 63 the far end is always in the next
    block), in the family's members with one row per level.  occ5 at p & 63 == 0: a far end on a block's first row."""
    geo = fam_u[(65, 70)]
    assert geo.two_blocks == set(range(64)) and geo.one_block == set()
    one = set()
    for (M, L), g in fam_u.items():
        one |= g.one_block
    assert one == set(range(63))
    assert 63 in fam_u[(1, 70)].two_blocks                      # [63, 63]: the far end is row 64, p & 63 == 0
    assert 0 in fam_u[(64, 70)].two_blocks                      # [64 j, 64 j + 63]: both ends at p & 63 == 0


def test_array_ends():
    ns = sorted(M * (L + 1) for M, L in bc.ARRAY_ENDS)
    assert ns == [1, 63, 64, 64, 65, 255, 256, 256, 256, 257]
    assert {n // 256 + 1 for n in ns} == {1, 2} and {n % 64 for n in ns} >= {0, 1, 63}
    assert sorted(M * (L + 1) for M, L in bc.POISON_ENDS) == [1, 64, 256, 257]
    assert bc.DEPTH[0] * (bc.DEPTH[1] + 1) == 130_002 and bc.DEPTH[1] == bc.MAX_READ_LEN < bc.UNSET


def test_wide_levels_flush_the_stage_inside_the_loop(fam_r):
    bwt, qs, lcp, sb, sq, geo, geo_s = fam_r
    for g in (geo, geo_s):
        assert max(g.kids_per_group) > bc.STAGE and sum(g.flushes) >= 8
        assert sum(1 for s in g.level_sizes if s > 10_000) >= 4
        assert max(g.level_sizes) > 16 * bc.PER_GROUP          # many workgroups
        for key in (("direct", 0), ("inline", 0), ("serial", 1), ("fill", 0), ("fill", 1)):
            assert g.routes.get(key, 0) > 0, key


def test_ring_sizes_select_the_three_routes(fam_r, fam_u, fam_t):
    """The rings of test_stage_and_ring.  The kernel appends children in the order its workgroups reserve, not the model's, so
    a size counts only when the model names the same route 10 % either side of it."""
    bwt, qs, lcp, sb, sq, geo, geo_s = fam_r
    n = len(bwt)
    for g in (geo, geo_s):
        assert bc.ring_route(g, 0)[0] == "log" and bc.ring_route(g, n + 64)[0] == "log"
        assert bc.ring_route(g, 64) == ("host", 1)
        for f in (0.9, 1.0, 1.1):
            route, k = bc.ring_route(g, int(bc.WIDE_RINGS["chunks"] * f))
            assert route == "chunks" and k >= 2, (f, route, k)
            route, k = bc.ring_route(g, int(bc.WIDE_RINGS["host"] * f))
            assert route == "host" and k >= 2, (f, route, k)
    # the small families under a ring of 64 entries: one row per level never leaves it, 65-row blocks do
    assert bc.ring_route(fam_u[(1, 70)], 64)[0] == "one"
    assert bc.ring_route(fam_t[(65, 65, 65)][3], 64)[0] in ("one", "chunks", "host")


def test_side_list_arithmetic():
    d, s0, s1, inner = bc.side_list_arithmetic(1 << 25)
    assert d == bc.LEN_MAX == 2 ** 25 - 1 and (s0, s1) == (0, 0) and inner > bc.FILL_INLINE
    d, s0, s1, inner = bc.side_list_arithmetic((1 << 25) + 1)
    assert d == bc.LEN_MAX + 1 and (s0, s1) == (2, 1) and inner == 1 << 25
    assert all(M * (L + 1) <= 1 << 27 for M, L in bc.SIDE_LISTS)
    # the same arithmetic row by row at a size that can be modelled: LEN_MAX lowered is not possible, so the shape only
    bwt, lcp = bc.unary(1000, 1)
    geo = bc.geometry(bwt)
    assert geo.level_sizes == [2, 1] and geo.routes == {("fill", 0): 1} and np.array_equal(geo.lcp, lcp)
