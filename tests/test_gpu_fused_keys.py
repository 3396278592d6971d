"""The suffix sort's first pass makes its records itself from the text (k_radix_scatter<1, true>, counted by k_build_keys'
counting form) instead of reading the array k_build_keys wrote.  Every case builds the eBWT twice on the same input -- the
default and BFQ_FUSEKEYS=0 (records written, five streamed passes) -- and requires equal BWT, QS and LCP; most cases are
compared with the CPU oracle as well.

The shapes sit on the new code's edges, which bfq_radix_geometry() reports (nothing is hard-coded here): collections of 1, 2,
3 and 5 rows (the 16-byte text loads' tails; one row takes the fallback route), one scatter tile - 1, exactly, + 1 row (for
small collections a radix block is one tile), four tiles -1 / + 1, reads shorter than the 16-symbol key (every key holds a
terminator; empty reads put terminators side by side), N's, one read of 300 identical bases (one digit takes a whole tile's
run), terminators on the last row of a tile and on the first row of the next, and one collection of the smallest size at
which a workgroup runs through two tiles (the output cursors carry over), made and run on the device and compared with the
fallback route only: the oracle would take minutes on it."""
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

A = lambda s: np.frombuffer(s, np.uint8)


def _geometry(n):
    t, b = C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().bfq_radix_geometry(n, C.byref(t), C.byref(b)) == 0
    return int(t.value), int(b.value)


def _switch(engine, monkeypatch, value):
    if value is None:
        monkeypatch.delenv("BFQ_FUSEKEYS", raising=False)
    else:
        monkeypatch.setenv("BFQ_FUSEKEYS", value)
    engine.set_params()                                               # (the environment is read here)


def _both(engine, monkeypatch, b, q, r, orc=None):
    """eBWT by the new default against BFQ_FUSEKEYS=0, then (orc given) against the oracle."""
    r = np.asarray(r, np.uint64)
    try:
        _switch(engine, monkeypatch, None)
        nb, nq, nl = engine.build_ebwt(b, q, r)
        _switch(engine, monkeypatch, "0")
        wb, wq, wl = engine.build_ebwt(b, q, r)
    finally:
        _switch(engine, monkeypatch, None)
    assert len(nb) == int(r[-1]) + len(r) - 1
    assert np.array_equal(nb, wb), "bwt"
    assert np.array_equal(nq, wq), "qs"
    assert np.array_equal(nl, wl), "lcp"
    if orc is not None:
        eb, eq, el = orc.build_ebwt(b, q, r)
        assert np.array_equal(nb, eb) and np.array_equal(nq, eq) and np.array_equal(nl.astype(np.uint32), el), "oracle"


def _reads(rng, lens, alphabet=b"ACGT", err=0.02):
    """Reads of the given lengths drawn from a short genome (so that long common prefixes and equal keys occur), with a few
    substitutions (N's among them)."""
    lens = [int(x) for x in lens]
    genome = np.array(list(alphabet), np.uint8)[rng.integers(0, len(alphabet), 700)]
    bs = []
    for L in lens:
        st = int(rng.integers(0, 700))
        s = np.tile(genome, L // 700 + 2)[st:st + L].copy()
        hit = rng.random(L) < err
        s[hit] = np.array(list(b"ACGTN"), np.uint8)[rng.integers(0, 5, int(hit.sum()))]
        bs.append(s)
    b = np.concatenate(bs) if bs else np.zeros(0, np.uint8)
    q = rng.integers(35, 75, len(b)).astype(np.uint8)
    r = np.zeros(len(lens) + 1, np.uint64); r[1:] = np.cumsum(lens)
    return b, q, r


def _lens_for_rows(rows, L=100):
    """Read lengths (L, the last one shorter) whose bases + reads make exactly `rows` rows."""
    k = rows // (L + 1)
    rest = rows - k * (L + 1)
    lens = [L] * k
    if rest:
        lens.append(rest - 1)                                         # (rest = 1: an empty read)
    assert sum(lens) + len(lens) == rows
    return lens


def test_smallest_collections(engine, orc, monkeypatch):
    _both(engine, monkeypatch, A(b""), A(b""), [0, 0], orc)                                   # 1 row: one empty read
    _both(engine, monkeypatch, A(b"G"), A(b"I"), [0, 1], orc)                                 # 2 rows
    _both(engine, monkeypatch, A(b"TA"), A(b"I5"), [0, 2], orc)                               # 3 rows
    _both(engine, monkeypatch, A(b"CAT"), A(b"I5F"), [0, 1, 3], orc)                          # 5 rows


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_one_tile_edges(engine, orc, monkeypatch, delta):
    tile, blk = _geometry(1)
    assert blk == tile
    rng = np.random.default_rng(200 + delta)
    b, q, r = _reads(rng, _lens_for_rows(tile + delta))
    assert len(b) + len(r) - 1 == tile + delta
    _both(engine, monkeypatch, b, q, r, orc)


@pytest.mark.parametrize("delta", [-1, 1])
def test_four_tiles_edges(engine, orc, monkeypatch, delta):
    tile, _ = _geometry(1)
    rng = np.random.default_rng(300 + delta)
    b, q, r = _reads(rng, _lens_for_rows(4 * tile + delta))
    assert len(b) + len(r) - 1 == 4 * tile + delta and _geometry(4 * tile + delta) == (tile, tile)
    _both(engine, monkeypatch, b, q, r, orc if delta == 1 else None)


def test_reads_shorter_than_the_key(engine, orc, monkeypatch):
    rng = np.random.default_rng(41)
    lens = np.array([0, 1, 2, 15])[rng.integers(0, 4, 1500)]
    lens[:6] = [0, 0, 15, 0, 1, 0]                                    # terminators side by side, at the very start as well
    b, q, r = _reads(rng, lens)
    _both(engine, monkeypatch, b, q, r, orc)


def test_reads_with_ns(engine, orc, monkeypatch):
    rng = np.random.default_rng(42)
    b, q, r = _reads(rng, [100] * 80, alphabet=b"ACGTNN", err=0.1)
    assert (b == ord("N")).sum() > 1000
    _both(engine, monkeypatch, b, q, r, orc)


def test_one_read_of_identical_bases(engine, orc, monkeypatch):
    _both(engine, monkeypatch, np.full(300, ord("G"), np.uint8), np.arange(300, dtype=np.uint8) % 40 + 35, [0, 300], orc)


def test_terminators_on_tile_borders(engine, orc, monkeypatch):
    """A read whose terminator is the last row of the first tile, one whose terminator is the first row of the third."""
    tile, _ = _geometry(1)
    lens = _lens_for_rows(tile)                                       # the terminator of the last of them is row tile - 1
    k = len(lens)
    lens += _lens_for_rows(tile + 1)                                  # ... and of these, row 2 * tile
    lens += [100, 0, 37]
    ends = np.cumsum(lens) + np.arange(len(lens))                     # the row of every read's terminator
    assert ends[k - 1] == tile - 1 and 2 * tile in ends
    rng = np.random.default_rng(43)
    b, q, r = _reads(rng, lens)
    _both(engine, monkeypatch, b, q, r, orc)


def test_two_tiles_per_block_on_the_device(engine, monkeypatch):
    """The smallest collection of 100-base reads whose radix blocks hold two tiles: made on the device, the whole fused path both ways."""
    tile, _ = _geometry(1)
    lo, hi = tile, 1 << 40                                            # smallest n with two tiles per block
    while lo < hi:
        mid = (lo + hi) // 2
        if _geometry(mid)[1] >= 2 * tile:
            hi = mid
        else:
            lo = mid + 1
    L = 100
    N = -(-lo // (L + 1))
    assert _geometry(N * (L + 1))[1] == 2 * tile
    dev = torch.device("cuda:0")
    sp = api.synth_spec(N, L, seed=77)
    db = torch.empty(N * L, dtype=torch.uint8, device=dev); dq = torch.empty_like(db)
    dr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    engine.synth_device(sp, db.data_ptr(), dq.data_ptr(), dr.data_ptr())
    torch.cuda.synchronize()
    res = {}
    par = dict(k=16, m=5, v=ord(">"), f=40, t=20, M=2, B=1)
    try:
        for env in (None, "0"):
            if env is None:
                monkeypatch.delenv("BFQ_FUSEKEYS", raising=False)
            else:
                monkeypatch.setenv("BFQ_FUSEKEYS", env)
            engine.set_params(**par)
            ob = torch.full_like(db, 0xEE); oq = torch.full_like(db, 0xEE)
            st = engine.run_reads_device(db.data_ptr(), dq.data_ptr(), dr.data_ptr(), N, N * L, ob.data_ptr(), oq.data_ptr())
            torch.cuda.synchronize()
            res[env] = (ob, oq, st)
    finally:
        _switch(engine, monkeypatch, None)
    assert res[None][2] == res["0"][2], (res[None][2], res["0"][2])
    assert res[None][2]["n_rows"] == N * (L + 1) and res[None][2]["qs_smoothed"] > 0
    assert torch.equal(res[None][0], res["0"][0]) and torch.equal(res[None][1], res["0"][1])


def test_generating_pass_runs_by_default(engine, monkeypatch):
    """The default really takes the new route (and BFQ_FUSEKEYS=0 the old one): told by the bytes the profile books for the
    five scatter passes -- the generating pass moves 14.51 bytes per row, a streamed one 24."""
    b, q, r = api.synth_host(api.synth_spec(500, 50, seed=3, coverage=25))
    n = len(b) + len(r) - 1
    seen = {}
    try:
        for env in (None, "0"):
            _switch(engine, monkeypatch, env)
            engine.prof_reset()
            engine.build_ebwt(b, q, r)
            p = engine.prof()
            seen[env] = (p["k_radix_scatter"]["launches"], p["k_radix_scatter"]["alg_bytes"] / n, p["k_build_keys"]["alg_bytes"] / n)
    finally:
        _switch(engine, monkeypatch, None)
    assert seen[None][0] == seen["0"][0] >= 5                         # (sorts inside large segments would add the same to both)
    assert abs((seen["0"][1] - seen[None][1]) - (24.0 - 14.51)) < 1e-6
    assert abs(seen["0"][2] - 14.5) < 1e-6 and seen[None][2] < 1.0
