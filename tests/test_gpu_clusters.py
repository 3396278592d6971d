"""The cluster kernels (k_cluster.hip: k_lcp_flags, k_cluster, process_cluster_body, the five k_big_*; k_compact.hip:
k_lcp_flags_win) with clusters placed on their chunk, lane, piece, tile and window borders by construction, every path held
to the CPU oracle bit for bit: bases, qualities, read offsets and all eight statistics.  Never one GPU path against another.

Part A: the eBWT and QS of a real collection with an LCP array written by tests/cluster_model.py (bfq_ext's job takes the LCP
as given), through the table path (2-byte entries always; 1-byte with K = 200 or 4-byte entries on a rotating third) and the
compact path (BFQ_COMPACT=1 with BFQ_COMPACT_WIN unset, 1000 and 1024).  Part B: designed collections whose one cluster of
chosen size is moved row by row with empty reads, through every path that computes its own LCP.  tests/test_cluster_host.py
asserts without a GPU that the geometries named here are really in these inputs."""
import numpy as np
import pytest
from bfqzip_amd import api
from tests import cluster_model as cm
from tests.test_gpu_parity import _check_against_oracle
from tests.test_gpu_poison import poisoned
from tests.test_gpu_posbins import _device_run

pytestmark = pytest.mark.gpu
A = cm.part_a()
ENV = ("BFQ_COMPACT", "BFQ_COMPACT_WIN", "BFQ_POSMODE")


def _same(got, want, what):
    gb, gq, groff, gst = got
    eb, eq, eroff, est = want
    assert np.array_equal(gb, eb), ("bases",) + what
    assert np.array_equal(gq, eq), ("quals",) + what
    assert np.array_equal(groff, eroff), ("roff",) + what
    assert len(est) == 8
    for k in est:
        assert est[k] == gst[k], (k, est[k], gst[k]) + what


def _widths(case):
    return [(cm.K2, np.uint16)] + {1: [(cm.K1, np.uint8)], 4: [(cm.K2, np.uint32)], None: []}[case.wide]


def _ext_paths(e, orc, monkeypatch, case, windows=(None, "1000", "1024")):
    """One part A case through the table path and the compact path of `e`."""
    try:
        for K, dt in _widths(case):
            bwt, qs, lcp, full, want = cm.oracle_ext(orc, case, K)
            for name in ENV:
                monkeypatch.delenv(name, raising=False)
            e.set_params(**full)                                          # (the environment is read here)
            _same(e.smooth_invert(bwt, qs, lcp.astype(dt)), want, (case.name, "table", dt.__name__))
        bwt, qs, lcp, full, want = cm.oracle_ext(orc, case, cm.K2)
        monkeypatch.setenv("BFQ_COMPACT", "1")
        for win in windows:
            if win is None:
                monkeypatch.delenv("BFQ_COMPACT_WIN", raising=False)
            else:
                monkeypatch.setenv("BFQ_COMPACT_WIN", win)
            e.set_params(**full)
            _same(e.smooth_invert(bwt, qs, lcp.astype(np.uint16)), want, (case.name, "compact", win))
    finally:
        for name in ENV:
            monkeypatch.delenv(name, raising=False)
        e.set_params()


# ---------------------------------------------------------------------------------------------------- part A
@pytest.mark.parametrize("kind", ["plain", "lastmin", "dip"])
def test_tiny_n(engine, orc, monkeypatch, kind):
    """k_lcp_flags: n = 1 .. 34 rows (fast path r0 >= 1 && r0 + 9 <= n, the byte-wise tail, no minimum on the last row).
    A window of 1000 or 1024 rows is cut to n (k_compact.hip: lcp_window), so the compact path runs with the default only."""
    for case in A["tiny"]:
        if case.name.endswith(kind):
            _ext_paths(engine, orc, monkeypatch, case, windows=(None,))


@pytest.mark.parametrize("case", A["start"], ids=repr)
def test_start_detection(engine, orc, monkeypatch, case):
    """k_cluster's start bits: first in() rows around the lane (16), wave (1024) and chunk (4096) borders, prev from the row
    before the lane's first, runs across a border found once, clusters that touch through a dip (on window borders too)."""
    _ext_paths(engine, orc, monkeypatch, case)


@pytest.mark.parametrize("case", A["dense"], ids=repr)
def test_dense(engine, orc, monkeypatch, case):
    """u16 starts[4][CL_WROWS]: 512 starts in every wave of a chunk, taken in eight rounds of 256."""
    _ext_paths(engine, orc, monkeypatch, case)


@pytest.mark.parametrize("case", A["steps8"], ids=repr)
def test_eight_byte_steps(engine, orc, monkeypatch, case):
    """process_cluster_body's 8-byte loads and first-zero-byte run length: sizes 2 .. 26 at starts 0, 1, 7 modulo 8."""
    _ext_paths(engine, orc, monkeypatch, case)


@pytest.mark.parametrize("case", A["bigthr"], ids=repr)
def test_big_threshold(engine, orc, monkeypatch, case):
    """j0 + 8 - start >= CL_BIG: sizes on both sides of 2048 rows, equal to the oracle whichever kernels take them."""
    engine.prof_reset()
    _ext_paths(engine, orc, monkeypatch, case)
    prof = engine.prof()
    assert prof["k_cluster"]["launches"] >= 4 and prof["k_cluster_big"]["launches"] >= 5 * prof["k_cluster"]["launches"]


@pytest.mark.parametrize("case", A["extent"], ids=repr)
def test_big_extent(engine, orc, monkeypatch, case):
    """k_big_extent: the flag-by-flag rest of the start row's piece, whole pieces by firstOut[], the fall-back to n."""
    _ext_paths(engine, orc, monkeypatch, case)


@pytest.mark.parametrize("case", A["tiles"], ids=repr)
def test_tiles(engine, orc, monkeypatch, case):
    """CB_FOR_TILES / CB_FOR_ROWS: 65536, 65537 and 131073 rows, 16-byte loads from ts & ~15 with the guard j < ts || j > te,
    tiles of three clusters rotated over the grid; M = 1 sums the errors of 131073 rows in row order."""
    _ext_paths(engine, orc, monkeypatch, case)


def test_end_of_the_arrays(orc, monkeypatch):
    """The guards at n of k_cluster, process_cluster_body and k_big_extent on an engine whose workspace holds 0xFF before every
    call: the table path never clears the 64 pad bytes behind in[n - 1], so they read as set flags."""
    with poisoned(0xFF):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 16)
            assert e.workspace_bytes() > 0 and (e.workspace_read(0, 1 << 16) == 0xFF).all()     # the switch is on for this engine
            for case in cm.end_cases():
                _ext_paths(e, orc, monkeypatch, case, windows=(None,) if case.n < 1000 else (None, "1024"))
        finally:
            e.close()


# ---------------------------------------------------------------------------------------------------- part B
@pytest.mark.parametrize("i", range(len(cm.PART_B)), ids=[x[0] for x in cm.PART_B])
def test_designed_collections(engine, orc, monkeypatch, i):
    """One cluster of 2047 .. 65537 rows with two frequent bases and a base to replace, its first row at 0 / 4095 modulo 4096
    (the per-chunk walk) or 1023 modulo 1024 / 5 modulo 16 (the big kernels), through every path with an LCP of its own:
    build + fused + inversion of a given eBWT, the device-resident call by position bins and with BFQ_POSMODE=1, pile by
    pile, capped, and the compact path on the oracle's eBWT (prec_sym from rank blocks)."""
    name, c0, c1, odd, mod, res = cm.PART_B[i]
    b, q, r, cl = cm.place(orc, c0, c1, odd, cm.U12, mod, res)
    par = cm.part_b_par(i)
    full = dict(k=16, m=2, v=ord(">"), f=40, t=20, M=2, B=0); full.update(par)
    p = orc.params(K=full["k"], m=full["m"], v=full["v"], f=full["f"], t=full["t"], M=full["M"], B=full["B"])
    eb, eq, est = orc.run_reads(b, q, r, p)
    assert est["num_clust_mod"] > 0 and est["modified"] > 0
    want = (eb, eq, r, est)
    try:
        _check_against_oracle(engine, orc, b, q, r, **par)
        engine.set_params(**full)
        gb, gq, gst = _device_run(engine, b, q, r)
        _same((gb, gq, r, gst), want, (name, "posbins"))
        monkeypatch.setenv("BFQ_POSMODE", "1")
        engine.set_params(**full)
        gb, gq, gst = _device_run(engine, b, q, r)
        _same((gb, gq, r, gst), want, (name, "posmode"))
        monkeypatch.delenv("BFQ_POSMODE")
        for piles in (1, 2):
            engine.set_params(piles=piles, **full)
            gb, gq, gst = engine.run_reads(b, q, r)
            _same((gb, gq, r, gst), want, (name, "piles", piles))
        bwt, qs, lcp = orc.build_ebwt(b, q, r)
        assert cm.find_cluster(lcp, full["k"], c0 + c1 + odd) == cl
        monkeypatch.setenv("BFQ_COMPACT", "1")
        engine.set_params(**full)
        _same(engine.smooth_invert(bwt, qs, lcp.astype(np.uint16)), orc.smooth_invert(bwt, qs, lcp, p), (name, "compact"))
    finally:
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        engine.set_params()
