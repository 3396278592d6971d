"""What tests/test_gpu_clusters.py rests on, checked without a GPU: tests/cluster_model.py's flag rule agrees with the oracle,
every geometry the GPU module is written for is really present in its inputs (sizes, first and last rows, their residues
modulo 8, 16, 64, 1024, 4096 and 65536), and every branch of the cluster analysis is really reached (the oracle's statistics)."""
import itertools
import numpy as np
import pytest
from tests import cluster_model as cm

A = cm.part_a()
ALL_A = [c for fam in A.values() for c in fam]
TERM = ord("#")


def _size(c):
    return c[1] - c[0] + 1


def _counted(wanted, m):
    return sum(1 for c in wanted if _size(c) >= m)


# ---------------------------------------------------------------------------------------------------- model == oracle
@pytest.mark.parametrize("fam", list(A))
def test_model_agrees_with_the_oracle_part_a(orc, fam):
    for c in A[fam]:
        for K in (cm.K2,) + ((cm.K1,) if c.wide == 1 else ()):
            bwt, qs, lcp, full, want = cm.oracle_ext(orc, c, K)
            assert len(bwt) == c.n <= 1_000_000
            assert int(lcp.max(initial=0)) <= (255 if K == cm.K1 else cm.LCP_TOP)
            assert cm.clusters(cm.flags(lcp, K)) == c.wanted, c
            assert want[3]["num_clust"] == _counted(c.wanted, full["m"]), (c, K)


@pytest.fixture(scope="module")
def part_b(orc):
    out = []
    for i, (name, c0, c1, odd, mod, res) in enumerate(cm.PART_B):
        b, q, r, cl = cm.place(orc, c0, c1, odd, cm.U12, mod, res)
        par = cm.part_b_par(i)
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        st = orc.run_reads(b, q, r, orc.params(K=par["k"], m=par["m"], M=par["M"], B=par["B"]))[2]
        out.append((name, c0 + c1 + odd, mod, res, cl, par, bwt, lcp, st))
    return out


def test_model_agrees_with_the_oracle_part_b(part_b):
    for name, size, mod, res, cl, par, bwt, lcp, st in part_b:
        assert len(bwt) <= 1_000_000
        assert st["num_clust"] == _counted(cm.clusters(cm.flags(lcp, par["k"])), par["m"]), name


# ---------------------------------------------------------------------------------------------------- the geometries
def test_tiny_n():
    by = {c.name: c for c in A["tiny"]}
    assert sorted({c.n for c in A["tiny"]}) == list(range(1, 35))
    assert any(len(c.lens) == 2 for c in A["tiny"]) and by["tiny_n1_plain"].wanted == []
    for n in range(2, 35):
        assert by["tiny_n%d_plain" % n].wanted == [(0, n - 1)]
        if n >= 3:
            c = by["tiny_n%d_lastmin" % n]
            l = c.lcp(cm.K2)
            assert l[n - 2] > l[n - 1] >= cm.K2 and c.wanted == [(0, n - 1)]          # a minimum, were the rule applied to the last row
        if n >= 4:
            c = by["tiny_n%d_dip" % n]
            l = c.lcp(cm.K2)
            assert l[n - 3] > l[n - 2] >= cm.K2 and l[n - 1] >= l[n - 2] and c.wanted == [(0, n - 3), (n - 2, n - 1)]
    # the flag kernel's fast path needs r0 >= 1 && r0 + 9 <= n: groups on both sides of it, byte tails of every length
    assert {n % cm.FLAG_GROUP for n in range(1, 35)} == set(range(8)) and 8 + 9 <= 34


def test_start_detection():
    firsts = set()
    for c in A["start"]:
        assert 39000 <= c.n <= 41000
        l = c.lcp(cm.K2)
        f = cm.flags(l, cm.K2)
        v = int(c.name.split("_")[1])
        for b in cm.START_ROWS[v]:
            cl = [x for x in c.wanted if x[0] + 1 == b]
            assert len(cl) == 1 and 2 <= _size(cl[0]) <= 9 and f[b] and not f[b - 1]
            firsts.add(b)
        for x in cm.ACROSS:
            assert sum(1 for a, e in c.wanted if a + 1 <= x - 1 and e >= x) == 1 and f[x - 1] and f[x]
        for d in cm.DIPS + cm.WIN_DIPS:
            assert l[d] >= cm.K2 and not f[d] and f[d - 1] and f[d + 1]                # in() = 0 by the minimum rule alone
            assert sum(1 for a, e in c.wanted if e == d - 1) == 1 and sum(1 for a, e in c.wanted if a == d) == 1
        assert all(2 <= _size(x) <= 9 for x in c.wanted)
    assert firsts == {1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192}
    assert {b % cm.LANE_ROWS for b in firsts} >= {0, 1, 15} and {b % cm.CL_WROWS for b in firsts} >= {0, 1, 1023}
    assert {b % cm.CL_CHUNK for b in firsts} >= {0, 1, 4095}
    assert [x % cm.LANE_ROWS for x in cm.ACROSS] == [0, 0, 0] and 2048 % cm.CL_WROWS == 0 and 12288 % cm.CL_CHUNK == 0
    assert [d % cm.LANE_ROWS for d in cm.DIPS] == [0, 0, 0] and 3072 % cm.CL_WROWS == 0 and 16384 % cm.CL_CHUNK == 0


def test_dense():
    for c in A["dense"]:
        ch1 = [x for x in c.wanted if cm.CL_CHUNK <= x[0] + 1 < 2 * cm.CL_CHUNK]
        assert len(ch1) == 2048 and all(_size(x) == 2 for x in ch1)
        per_wave = np.bincount([(x[0] + 1 - cm.CL_CHUNK) // cm.CL_WROWS for x in ch1])
        assert list(per_wave) == [512] * 4                                              # the starts[] list full in every wave
        assert 2048 // 256 == 8                                                         # rounds of the take loop
        ch2 = [x for x in c.wanted if 2 * cm.CL_CHUNK <= x[0] + 1 < 3 * cm.CL_CHUNK]
        assert len(ch2) >= 1360 and all(_size(x) == 3 for x in ch2)
    assert {c.par["m"] for c in A["dense"]} == {2, 5}


def test_eight_byte_steps():
    for c in A["steps8"]:
        got = {(_size(x), x[0] % 8) for x in c.wanted[1:]}
        assert got == set(itertools.product(range(2, 27), (0, 1, 7)))
        assert c.par["m"] == 5 and c.wanted[0] == (1, 6) and c.lens[:cm.EMPTY_FRONT] == [0] * cm.EMPTY_FRONT


def test_big_threshold():
    for c in A["bigthr"]:
        assert {(_size(x), x[0] % 8) for x in c.wanted} == set(itertools.product(cm.BIG_SIZES, (0, 5)))
    assert {s > cm.CL_BIG for s in cm.BIG_SIZES} == {False, True} and cm.CL_BIG in cm.BIG_SIZES and cm.CL_BIG + 1 in cm.BIG_SIZES


def test_big_extent():
    P = cm.CL_WROWS
    assert [c.n % P for c in A["extent"]] == [0, 1, 1023]
    for c in A["extent"]:
        w = c.wanted
        assert all(_size(x) > cm.CL_BIG for x in w)
        assert any(e % P == P - 1 and e != c.n - 1 for a, e in w)                        # last row = a piece's last row
        assert any(e % P == 0 for a, e in w)                                             # ... = a piece's first row
        assert any(e // P - (a + 2) // P == 4 and e % P not in (0, P - 1) for a, e in w)  # three whole pieces skipped by firstOut[]
        assert w[-1][1] == c.n - 1
        assert any((a + 1) % P == P - 1 for a, e in w)                                   # r + 1 opens a piece
        assert any((a + 1) % cm.LANE_ROWS == 15 and (a + 1) % P != P - 1 for a, e in w)
        same = [(x, y) for x, y in zip(w, w[1:]) if (x[0] + 1) // cm.CL_CHUNK == (y[0] + 1) // cm.CL_CHUNK]
        assert same and _size(same[0][0]) == cm.CL_BIG + 1 and same[0][1][0] == same[0][0][1] + 2   # 2049 rows, a gap row, the next


def test_tiles():
    for c in A["tiles"]:
        assert 250_000 <= c.n <= 350_000
        assert [_size(x) for x in c.wanted] == [cm.CB_TILE, cm.CB_TILE + 1, 2 * cm.CB_TILE + 1]
        assert c.wanted[2][0] % 16 == 5 and c.wanted[0][0] % 16 == 0 and c.wanted[1][0] % 16 not in (0, 5)
    assert [c.par["M"] for c in A["tiles"]] == [1, 3]


def test_window_borders():
    """The compact path's windows (BFQ_COMPACT_WIN unset, 1000, 1024): in every family with a border case a window border
    falls on a first in() row, on the row after a last one and inside a run; the start detection cases have a dip on the
    first row of a window of either size and on the last row of one (the neighbours the minimum rule reads lie in the
    window before / behind)."""
    for fam in ("start", "extent"):
        for c in A[fam]:
            hits = set().union(*(cm.window_hits(x) for x in c.wanted))
            assert hits == {"first", "after", "inside"}, (c, hits)
    for fam in ("bigthr", "tiles", "dense", "steps8"):
        for c in A[fam]:
            assert "inside" in set().union(*(cm.window_hits(x) for x in c.wanted)) or c.n < 2000, c
    dips = cm.DIPS + cm.WIN_DIPS
    for W in cm.WINDOWS:
        assert any(d % W == 0 for d in dips) and any((d + 1) % W == 0 for d in dips), W


def test_end_of_the_arrays():
    ends = cm.end_cases()
    assert {c.n for c in ends if c.name.startswith("tiny")} == set(range(17, 35))
    assert sorted(c.n % cm.CL_WROWS for c in ends if c.name.startswith("extent")) == [0, 1, 1023]
    assert all(c.wanted[-1][1] == c.n - 1 for c in ends)


def test_part_b_geometry(part_b):
    sizes = set()
    for name, size, mod, res, cl, par, bwt, lcp, st in part_b:
        assert _size(cl) == size and cl[0] % mod == res, name
        assert cl[0] // cm.RANK_BLOCK < cl[1] // cm.RANK_BLOCK                          # straddles a rank block border
        syms = {chr(s): int(n) for s, n in zip(*np.unique(bwt[cl[0]:cl[1] + 1], return_counts=True))}
        assert set(syms) == {"C", "G", "T"} and 100 * syms["C"] // size >= 40 and 100 * syms["G"] // size >= 40, (name, syms)
        assert st["num_clust_mod"] > 0 and st["modified"] > 0, name
        sizes.add((size, mod, res))
    assert sizes == {(s, 4096, r) for s in (2047, 2048, 2049) for r in (0, 4095)} | \
        {(s, m, r) for s in (4097, 65537) for m, r in ((1024, 1023), (16, 5))}


# ---------------------------------------------------------------------------------------------------- the branches
def test_every_branch_is_reached(orc):
    tot = {}
    no_base = below_m = 0
    for c in ALL_A:
        bwt, qs, lcp, full, want = cm.oracle_ext(orc, c, cm.K2)
        for k, v in want[3].items():
            tot[k] = tot.get(k, 0) + v
        for a, e in c.wanted:
            below_m += _size((a, e)) < full["m"]
            no_base += _size((a, e)) >= full["m"] and bool((bwt[a:e + 1] == TERM).all())
    assert tot["modified"] > 0 and tot["qs_smoothed"] > 0 and tot["num_clust_amb_discarded"] > 0
    assert tot["num_clust_discarded"] > 0 and tot["num_clust_mod"] > 0 and tot["num_clust_alleq"] > 0
    assert no_base > 0 and below_m > 0
    assert any(c.par.get("f") == 30 for c in ALL_A)
    # the big kernels' two-frequent-bases branch (k_big_prec) under a crafted LCP: -f 30 lets A and C both through
    for c in ALL_A:
        if c.par.get("f") == 30 and all(_size(x) > cm.CL_BIG for x in c.wanted):
            assert cm.oracle_ext(orc, c, cm.K2)[4][3]["num_clust_amb_discarded"] > 0, c
    assert {(c.par["M"], c.par.get("ext", 0)) for c in ALL_A} == {(0, 0), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1)}
    assert {c.par["B"] for c in ALL_A} == {0, 1} and {c.par["m"] for c in ALL_A} == {2, 5}


def test_m1_differs_from_m0(orc):
    for c in ALL_A:
        if c.par["M"] == 1 and c.n > 1000 and cm.oracle_ext(orc, c, cm.K2)[4][3]["qs_smoothed"]:
            q1 = cm.oracle_ext(orc, c, cm.K2)[4][1]
            q0 = cm.oracle_ext(orc, c, cm.K2, M=0, ext=0)[4][1]
            assert not np.array_equal(q0, q1), c
