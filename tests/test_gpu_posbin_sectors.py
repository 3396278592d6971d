"""The position bins' first partition level writes whole 64-byte chunks (k_posbin_l1_wc: a workgroup carries every bin's
incomplete tail from tile to tile; the tails go to the bins' ends through a second, downward cursor).  Every case runs
bfq_run_reads_device three ways on the same parameters -- the default, BFQ_POSBIN_WC=0 (per-tile runs at the cursor) and
BFQ_POSBINS=0 (LF walks) -- and compares bases, qualities and every counter byte for byte; cases of at most about 10 k rows
are compared with the CPU oracle as well.

The shapes are the smallest at which the new code can go wrong; the geometry comes from bfq_posbin_geometry(), a chunk is 8
records of 8 bytes (16 of the second level's 4-byte records, which the microbenchmark left as runs): fewer rows than one
chunk (C - 1, C, C + 1 rows for both C), a last first-level bin cut off mid-chunk (capacities = 1, 7, 15 mod C; a last bin
of one record), tiles whose records all fall into one bin (identical reads: the rows of one suffix offset are adjacent and
lie four positions apart), a poly-G block, one collection above 512 windows (first-level bins of two windows: many bins
with whole chunks and tails, several tiles per workgroup), and reads of lengths 1, 17 and 300."""
import numpy as np
import pytest
from bfqzip_amd import api
from tests.test_gpu_posbins import A, BASE, _device_run, _geometry, _reads_with_rows

pytestmark = pytest.mark.gpu

WAYS = ((None, None), ("BFQ_POSBIN_WC", "0"), ("BFQ_POSBINS", "0"))


def _three(engine, monkeypatch, b, q, r, orc=None, **par):
    """Default against BFQ_POSBIN_WC=0 and BFQ_POSBINS=0, then (orc given) against the oracle; returns the statistics."""
    full = dict(BASE); full.update(par)
    got = []
    try:
        for name, val in WAYS:
            monkeypatch.delenv("BFQ_POSBIN_WC", raising=False)
            monkeypatch.delenv("BFQ_POSBINS", raising=False)
            if name:
                monkeypatch.setenv(name, val)
            engine.set_params(**full)                                 # (the environment is read here)
            got.append(_device_run(engine, b, q, r))
    finally:
        monkeypatch.delenv("BFQ_POSBIN_WC", raising=False)
        monkeypatch.delenv("BFQ_POSBINS", raising=False)
        engine.set_params()
    nb, nq, nst = got[0]
    for (name, _), (ob, oq, ost) in zip(WAYS[1:], got[1:]):
        assert np.array_equal(nb, ob), ("bases", name, par)
        assert np.array_equal(nq, oq), ("quals", name, par)
        assert nst == ost, (nst, ost, name, par)
    if orc is not None:
        p = orc.params(K=full["k"], m=full["m"], v=full["v"], f=full["f"], t=full["t"], M=full["M"], B=full["B"])
        eb, eq, est = orc.run_reads(b, q, r, p)
        assert np.array_equal(nb, eb) and np.array_equal(nq, eq), ("oracle", par)
        for k in est:
            assert est[k] == nst[k], (k, par)
    return nst


@pytest.mark.parametrize("rows", [7, 8, 9, 15, 16, 17])
def test_fewer_rows_than_a_chunk(engine, orc, monkeypatch, rows):
    """C - 1, C and C + 1 rows for both chunk sizes: nothing or one chunk goes through the head cursor, the rest is tails."""
    rng = np.random.default_rng(rows)
    b, q, r = _reads_with_rows(rng, rows, [2])
    st = _three(engine, monkeypatch, b, q, r, orc, m=2, k=1, B=1)
    assert st["n_rows"] == rows


@pytest.mark.parametrize("extra", [1, 7, 15])
def test_last_window_cut_off_mid_chunk(engine, monkeypatch, extra):
    """W + 1, W + 7 and W + 15 rows: the last first-level bin (one window) holds 1, C - 1 records for both C."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(200 + extra)
    b, q, r = _reads_with_rows(rng, W + extra, [100] * 300)
    st = _three(engine, monkeypatch, b, q, r, None, m=3, k=8, B=1)
    assert st["n_rows"] == W + extra and st["qs_smoothed"] > 0


def test_last_first_level_bin_of_one_record(engine, monkeypatch):
    """Two first-level bins plus one row."""
    W, s1 = _geometry(100000)
    rows = 2 * (1 << s1) + 1
    assert _geometry(rows) == (W, s1)
    rng = np.random.default_rng(6)
    b, q, r = _reads_with_rows(rng, rows, [100] * 600)
    st = _three(engine, monkeypatch, b, q, r, None, m=3, k=8)
    assert st["n_rows"] == rows and st["qs_smoothed"] > 0


def test_tiles_that_fall_into_one_bin(engine, monkeypatch):
    """16384 identical reads of three bases: the rows of one suffix offset are adjacent, in read order, four positions apart, so
    4096 consecutive rows cover 16384 consecutive positions -- one window, one first-level bin, 512 whole chunks of one bin."""
    W, _ = _geometry(1)
    N = W // 2
    b = np.tile(A(b"ACG"), N)
    q = np.tile(np.array([40, 55, 70], np.uint8), N)
    r = np.arange(N + 1, dtype=np.uint64) * 3
    st = _three(engine, monkeypatch, b, q, r, None, m=2, k=2, B=1)
    assert st["n_rows"] == 2 * W


def test_poly_g_block(engine, monkeypatch):
    """The poly-G shape of tests/test_gpu_posbins.py at 1500 x 100 (clusters of the k_big_* kernels)."""
    rng = np.random.default_rng(77)
    N, L = 1500, 100
    b = np.full(N * L, ord("G"), np.uint8)
    hit = rng.random(N * L) < 0.01
    b[hit] = np.array(list(b"ACTN"), np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    q = rng.integers(35, 75, N * L).astype(np.uint8)
    r = np.arange(N + 1, dtype=np.uint64) * L
    st = _three(engine, monkeypatch, b, q, r, None, m=5, M=1, B=1)
    assert st["qs_smoothed"] > 2048


def test_bins_of_two_windows(engine, monkeypatch):
    """Just above 512 windows a first-level bin holds two windows: 258 bins, every workgroup takes several tiles and carries
    tails between them."""
    W, _ = _geometry(1)
    N = (512 * W) // 101 + 2000
    _, s1 = _geometry(N * 101)
    assert (1 << s1) > W
    b, q, r = api.synth_host(api.synth_spec(N, 100, seed=99, coverage=25))
    st = _three(engine, monkeypatch, b, q, r, None, m=5, B=1)
    assert st["n_rows"] == N * 101 and st["modified"] > 0


@pytest.mark.parametrize("B", [0, 1])
def test_mixed_read_lengths(engine, orc, monkeypatch, B):
    rng = np.random.default_rng(11 + B)
    b, q, r = _reads_with_rows(rng, 1 + 17 + 300 + 3, [1, 17])
    assert list(np.diff(r.astype(np.int64))) == [1, 17, 300]
    _three(engine, monkeypatch, b, q, r, orc, m=2, k=2, B=B)


def test_whole_chunk_kernels_run_by_default(engine, monkeypatch):
    """The default takes the write-combining path (it alone checks head + tail = capacity afterwards: k_posbin_check) and
    BFQ_POSBIN_WC=0 the per-tile runs: told by the profile names."""
    b, q, r = api.synth_host(api.synth_spec(500, 50, seed=3, coverage=25))
    seen = {}
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("BFQ_POSBIN_WC", raising=False)
        else:
            monkeypatch.setenv("BFQ_POSBIN_WC", env)
        engine.set_params(**BASE)
        engine.prof_reset()
        _device_run(engine, b, q, r)
        seen[env] = {k for k, v in engine.prof().items() if v["launches"]}
    monkeypatch.delenv("BFQ_POSBIN_WC", raising=False)
    engine.set_params()
    parts = {"k_posbin_l1", "k_posbin_l2", "k_posbin_apply"}
    assert parts | {"k_posbin_check"} <= seen[None] and "k_invert" not in seen[None]
    assert parts <= seen["0"] and "k_posbin_check" not in seen["0"] and "k_invert" not in seen["0"]
