"""The device-resident fused path brings the rows back to text order by position bins (k_posbin.hip: two partition levels on
the text position every row's sort record carries, one LDS placement per window) instead of an LF table and walks.  Every
case runs bfq_run_reads_device twice on the same parameters -- the default and BFQ_POSBINS=0 (LF walks) -- and compares
bases, qualities and every counter byte for byte; one case of each shape is compared with the CPU oracle as well.

The shapes sit on the new code's edges, which bfq_posbin_geometry() reports (nothing is hard-coded here): collections of
W - 1, W and W + 1 rows, two first-level bins plus one row, reads that straddle a window / a first-level bin, reads of
lengths 1, 17 and 300, one read of one base, no rows at all, a poly-G block (clusters of the k_big_* kernels, which write
row-local edits too), all four smoothing modes, and one collection above 512 windows, where a first-level bin holds more
than one window (compared with the walks only: the oracle would take a minute on it)."""
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import util

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = lambda s: np.frombuffer(s, np.uint8)
BASE = dict(k=16, m=2, v=ord(">"), f=40, t=20, M=2, B=0)


def _geometry(n):
    w, s = C.c_uint64(0), C.c_int(0)
    assert _lib.lib().bfq_posbin_geometry(n, C.byref(w), C.byref(s)) == 0
    return int(w.value), int(s.value)


def _device_run(engine, b, q, r):
    dev = torch.device("cuda:0")
    n = max(len(b), 1)
    db = torch.zeros(n, dtype=torch.uint8, device=dev); dq = torch.zeros_like(db)
    db[:len(b)] = torch.from_numpy(np.array(b, np.uint8)).to(dev); dq[:len(b)] = torch.from_numpy(np.array(q, np.uint8)).to(dev)
    dr = torch.from_numpy(np.asarray(r).astype(np.int64)).to(dev)
    ob = torch.full_like(db, 0xEE); oq = torch.full_like(db, 0xEE)
    st = engine.run_reads_device(db.data_ptr(), dq.data_ptr(), dr.data_ptr(), len(r) - 1, len(b), ob.data_ptr(), oq.data_ptr())
    torch.cuda.synchronize()
    return ob.cpu().numpy()[:len(b)], oq.cpu().numpy()[:len(b)], st


def _both(engine, monkeypatch, b, q, r, orc=None, **par):
    """New default against BFQ_POSBINS=0, then (orc given) against the oracle; returns the statistics."""
    full = dict(BASE); full.update(par)
    try:
        monkeypatch.delenv("BFQ_POSBINS", raising=False)
        engine.set_params(**full)                                     # (the environment is read here)
        nb, nq, nst = _device_run(engine, b, q, r)
        monkeypatch.setenv("BFQ_POSBINS", "0")
        engine.set_params(**full)
        wb, wq, wst = _device_run(engine, b, q, r)
    finally:
        monkeypatch.delenv("BFQ_POSBINS", raising=False)
        engine.set_params()
    assert np.array_equal(nb, wb), ("bases", par)
    assert np.array_equal(nq, wq), ("quals", par)
    assert nst == wst, (nst, wst, par)
    if orc is not None:
        p = orc.params(K=full["k"], m=full["m"], v=full["v"], f=full["f"], t=full["t"], M=full["M"], B=full["B"])
        eb, eq, est = orc.run_reads(b, q, r, p)
        assert np.array_equal(nb, eb) and np.array_equal(nq, eq), ("oracle", par)
        for k in est:
            assert est[k] == nst[k], (k, par)
    return nst


def _reads_with_rows(rng, rows, lens):
    """Reads of the given lengths, the last one sized so that bases + reads = rows; drawn from a short genome so that clusters
    form and get edited."""
    lens = list(lens)
    lens.append(rows - sum(lens) - len(lens) - 1)
    assert lens[-1] >= 1
    genome = np.array(list(b"ACGT"), np.uint8)[rng.integers(0, 4, 700)]
    bs = []
    for L in lens:
        reps = -(-(L + 700) // 700)
        st = int(rng.integers(0, 700))
        s = np.tile(genome, reps + 1)[st:st + L].copy()
        err = rng.random(L) < 0.02
        s[err] = np.array(list(b"ACGTN"), np.uint8)[rng.integers(0, 5, int(err.sum()))]
        bs.append(s)
    b = np.concatenate(bs)
    q = rng.integers(35, 75, len(b)).astype(np.uint8)
    r = np.zeros(len(lens) + 1, np.uint64); r[1:] = np.cumsum(lens)
    assert len(b) + len(lens) == rows
    return b, q, r


def test_smallest_collections(engine, orc, monkeypatch):
    _both(engine, monkeypatch, A(b"A"), A(b"I"), np.array([0, 1], np.uint64), orc, m=2, k=1)            # N = 1, L = 1
    _both(engine, monkeypatch, A(b""), A(b""), np.array([0], np.uint64))                                # no read at all
    _both(engine, monkeypatch, A(b""), A(b""), np.array([0, 0, 0], np.uint64), orc, m=2, k=1)           # only empty reads
    rng = np.random.default_rng(11)
    b, q, r = _reads_with_rows(rng, 1 + 17 + 300 + 3, [1, 17])                                          # lengths 1, 17, 300
    assert list(np.diff(r.astype(np.int64))) == [1, 17, 300]
    _both(engine, monkeypatch, b, q, r, orc, m=2, k=2, B=1)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_window_edges(engine, orc, monkeypatch, delta):
    """W - 1, W and W + 1 rows: one window that is just not full, exactly full, and a second window of one row."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(100 + delta)
    b, q, r = _reads_with_rows(rng, W + delta, [100] * 300)
    st = _both(engine, monkeypatch, b, q, r, orc if delta == 1 else None, m=3, k=8, B=1)
    assert st["n_rows"] == W + delta and st["qs_smoothed"] > 0


def test_two_bins_plus_one_row_and_straddling_reads(engine, orc, monkeypatch):
    """Exactly two first-level bins plus one row; a read of 300 bases lies across the first boundary (it starts 150 positions
    before it), and the last read (17 bases) ends at the second: its terminator is the one row of the third bin."""
    rows0 = 100000
    W, s1 = _geometry(rows0)
    bin1 = 1 << s1
    rows = 2 * bin1 + 1
    assert _geometry(rows) == (W, s1)
    rng = np.random.default_rng(5)
    # reads of 100 bases up to 150 positions before the boundary, then the straddling read
    k1 = (bin1 - 150) // 101
    lens = [100] * (k1 - 1) + [bin1 - 150 - 101 * (k1 - 1) - 1, 300]
    assert sum(lens[:-1]) + len(lens) - 1 == bin1 - 150
    pos = sum(lens) + len(lens)                                       # text position after the 300-base read's terminator
    k2 = (2 * bin1 - 17 - pos) // 101
    lens += [100] * (k2 - 1)
    pos = sum(lens) + len(lens)
    lens += [2 * bin1 - 17 - pos - 1]                                 # the last read starts 17 positions before the second boundary
    b, q, r = _reads_with_rows(rng, rows, lens)
    assert int(r[-1] - r[-2]) == 17 and int(r[-1]) + len(r) - 2 == 2 * bin1   # the last terminator alone in the third bin
    st = _both(engine, monkeypatch, b, q, r, orc, m=3, k=8)
    assert st["n_rows"] == rows and st["qs_smoothed"] > 0


@pytest.mark.parametrize("M,B", [(1, 0), (2, 0), (2, 1), (3, 0)])
def test_synthetic_all_edit_kinds(engine, orc, monkeypatch, M, B):
    b, q, r = api.synth_host(api.synth_spec(20000, 100, seed=4100 + 2 * M + B, coverage=25))
    st = _both(engine, monkeypatch, b, q, r, orc, M=M, B=B, m=5)
    assert st["qs_smoothed"] > 0 and st["modified"] > 0


def test_poly_g_block(engine, orc, monkeypatch):
    """Clusters far above CL_BIG rows (k_big_*): poly-G reads with a few other bases and N's."""
    rng = np.random.default_rng(77)
    N, L = 1500, 100
    b = np.full(N * L, ord("G"), np.uint8)
    hit = rng.random(N * L) < 0.01
    b[hit] = np.array(list(b"ACTN"), np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    q = rng.integers(35, 75, N * L).astype(np.uint8)
    r = np.arange(N + 1, dtype=np.uint64) * L
    st = _both(engine, monkeypatch, b, q, r, orc, m=5, M=1, B=1)
    assert st["qs_smoothed"] > 2048


def test_bins_of_several_windows(engine, monkeypatch):
    """Above 512 windows a first-level bin holds more than one window: the second partition level then really partitions."""
    W, _ = _geometry(1)
    N = (512 * W) // 101 + 2000
    _, s1 = _geometry(N * 101)
    assert (1 << s1) > W
    b, q, r = api.synth_host(api.synth_spec(N, 100, seed=99, coverage=25))
    st = _both(engine, monkeypatch, b, q, r, None, m=5, B=1)
    assert st["n_rows"] == N * 101 and st["modified"] > 0


def test_new_kernels_run_by_default(engine, monkeypatch):
    """The default really takes the new path (and BFQ_POSBINS=0 the walks): told by the profile names."""
    b, q, r = api.synth_host(api.synth_spec(500, 50, seed=3, coverage=25))
    seen = {}
    for env in (None, "0"):
        if env is None:
            monkeypatch.delenv("BFQ_POSBINS", raising=False)
        else:
            monkeypatch.setenv("BFQ_POSBINS", env)
        engine.set_params(**BASE)
        engine.prof_reset()
        _device_run(engine, b, q, r)
        seen[env] = {k for k, v in engine.prof().items() if v["launches"]}
    monkeypatch.delenv("BFQ_POSBINS", raising=False)
    engine.set_params()
    assert {"k_posbin_l1", "k_posbin_l2", "k_posbin_apply"} <= seen[None] and "k_invert" not in seen[None] and "k_lf_build" not in seen[None]
    assert "k_invert" in seen["0"] and "k_posbin_l1" not in seen["0"]
