"""The position bins move only the rows whose final (base, quality) differs from a default the last kernel works out by itself
at that position (k_posbin.hip, bfq_posbin.h): the input ("keep"), or the input base with the constant quality of M = 2
("const"), chosen per call on the device.  The choice changes the traffic, never the result, so every case runs
bfq_run_reads_device on the same parameters the default way, with both polarities forced (const where M = 2),
with BFQ_POSBIN_SPARSE=0 (every row travels) and with BFQ_POSBINS=0 (LF walks), and compares bases, qualities and every
counter byte for byte; cases of at most about 10 k rows are compared with the CPU oracle as well.  After every sparse run
bfq_posbin_sparse_last() must report exactly as many rows sent as output positions differ from that run's default -- a count
taken from the inputs and outputs alone.

The shapes are the smallest at which the new code can go wrong (geometry from bfq_posbin_geometry()): nothing to send at all,
almost nothing under const, collections that make the device choose either polarity, windows of W - 1, W and W + 1 rows,
terminators on the first and the last position of a window, windows of terminators only, a window without a record between
two that get some, two first-level bins plus one row, first-level bins with head, gap and tail above 512 windows, big
clusters, all smoothing modes, and a workspace filled with 0xC3 / 0x41 before the call (the gaps of partially filled bins
and windows must never be read as records)."""
import functools
import os
import numpy as np
import pytest
from bfqzip_amd import api
from tests.test_gpu_posbins import A, BASE, _device_run, _geometry, _reads_with_rows

pytestmark = pytest.mark.gpu

KEEP, CONST = 0, 1
ENV = ("BFQ_POSBIN_SPARSE", "BFQ_POSBIN_POLARITY", "BFQ_POSBINS", "BFQ_POSBIN_WC")
STAGES = {"k_posbin_l1", "k_posbin_l2", "k_posbin_apply"}


def _bin8(q):
    s = np.asarray(q, np.uint8).astype(np.int8).astype(np.int64) - 33
    out = s.copy()
    for lo, val in ((2, 6), (10, 15), (20, 22), (25, 27), (30, 33), (35, 37), (40, 40)):
        out[s >= lo] = val
    return ((out + 33) & 0xFF).astype(np.uint8)


def _differ(b, q, ob, oq, pol, full):
    """Output positions whose (base, quality) is not the default of polarity pol: what a sparse run has to send."""
    dq = np.asarray(q, np.uint8) if pol == KEEP else np.full(len(q), full["v"] & 0xFF, np.uint8)
    if full["B"]:
        dq = _bin8(dq)
    return int(np.count_nonzero((ob != np.asarray(b, np.uint8)) | (oq != dq)))


def _ways(M):
    ways = [("default", {}), ("keep", {"BFQ_POSBIN_POLARITY": "keep"})]
    if M == 2:
        ways.append(("const", {"BFQ_POSBIN_POLARITY": "const"}))
    return ways + [("dense", {"BFQ_POSBIN_SPARSE": "0"}), ("walks", {"BFQ_POSBINS": "0"})]


def _set_env(env):
    for k in ENV:
        os.environ.pop(k, None)
    os.environ.update(env)


def _all_ways(engine, b, q, r, orc=None, **par):
    """Every way of the module docstring on one input; returns {way: (polarity, rows_sent)} and the statistics."""
    full = dict(BASE); full.update(par)
    got, last = {}, {}
    try:
        for name, env in _ways(full["M"]):
            _set_env(env)
            engine.set_params(**full)                                 # (the environment is read here)
            got[name] = _device_run(engine, b, q, r)
            last[name] = engine.posbin_sparse_last()
    finally:
        _set_env({})
        engine.set_params()
    wb, wq, wst = got["walks"]
    for name, (ob, oq, ost) in got.items():
        assert np.array_equal(ob, wb), ("bases", name, par)
        assert np.array_equal(oq, wq), ("quals", name, par)
        assert ost == wst, (ost, wst, name, par)
    assert last["dense"][0] == -1 and last["walks"][0] == -1, last
    if len(r) == 1:                                                   # no rows: no stage runs at all
        assert all(v == (-1, 0) for v in last.values()), last
        last["out"] = (wb, wq)
        return last, wst
    assert last["keep"][0] == KEEP and last["default"][0] in (KEEP, CONST), last
    if "const" in last:
        assert last["const"][0] == CONST, last
    else:
        assert last["default"][0] == KEEP, last                       # const is for M = 2 alone
    for name in ("default", "keep", "const"):
        if name in last:
            pol, sent = last[name]
            want = _differ(b, q, wb, wq, pol, full)
            print("%s: polarity %d, rows sent %d, positions that differ %d of %d" % (name, pol, sent, want, len(b)))
            assert sent == want, (name, pol, sent, want, par)
    if orc is not None:
        p = orc.params(K=full["k"], m=full["m"], v=full["v"], f=full["f"], t=full["t"], M=full["M"], B=full["B"])
        eb, eq, est = orc.run_reads(b, q, r, p)
        assert np.array_equal(wb, eb) and np.array_equal(wq, eq), ("oracle", par)
        for k in est:
            assert est[k] == wst[k], (k, par)
    last["out"] = (wb, wq)
    return last, wst


@functools.lru_cache(maxsize=None)
def _flip_input(coverage):
    return api.synth_host(api.synth_spec(4000, 100, seed=4100, coverage=coverage))


@functools.lru_cache(maxsize=None)
def _several_windows_input():
    W, _ = _geometry(1)
    N = (512 * W) // 101 + 2000
    _, s1 = _geometry(N * 101)
    assert (1 << s1) > W
    return api.synth_host(api.synth_spec(N, 100, seed=99, coverage=25))


@pytest.mark.parametrize("B", [0, 1])
def test_nothing_sent(engine, orc, B):
    """Unrelated random reads: no cluster, no edit.  keep sends no row at all, and the output is the input (binned at B = 1)."""
    rng = np.random.default_rng(31)
    N, L = 60, 100
    b = np.array(list(b"ACGT"), np.uint8)[rng.integers(0, 4, N * L)]
    q = rng.integers(35, 75, N * L).astype(np.uint8)
    r = np.arange(N + 1, dtype=np.uint64) * L
    last, st = _all_ways(engine, b, q, r, orc, B=B)
    assert st["qs_smoothed"] == 0 and st["modified"] == 0
    assert last["default"] == (KEEP, 0) and last["keep"] == (KEEP, 0)
    assert last["const"][1] == _differ(b, q, b, _bin8(q) if B else q, CONST, dict(BASE, B=B)) > 0


def test_almost_nothing_sent_under_const(engine, orc):
    """Many identical reads whose qualities are v already: whatever is smoothed stays what the const default says."""
    rng = np.random.default_rng(32)
    N, L = 90, 100
    one = np.array(list(b"ACGT"), np.uint8)[rng.integers(0, 4, L)]
    b = np.tile(one, N)
    q = np.full(N * L, BASE["v"], np.uint8)
    r = np.arange(N + 1, dtype=np.uint64) * L
    last, st = _all_ways(engine, b, q, r, orc, m=2)
    assert st["qs_smoothed"] > N * L // 2 and last["default"][0] == CONST
    assert last["const"][1] == 0 and last["default"][1] == 0


@pytest.mark.parametrize("coverage,want", [(25, CONST), (6, KEEP), (2, KEEP)])
def test_polarity_flips_with_coverage(engine, coverage, want):
    b, q, r = _flip_input(coverage)
    last, st = _all_ways(engine, b, q, r, None, M=2, m=5)
    assert last["default"][0] == want, (last, st)
    assert (2 * st["qs_smoothed"] > len(b)) == (want == CONST)
    # the device took the cheaper default
    assert last["default"][1] == min(last["keep"][1], last["const"][1])


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_window_edges(engine, orc, delta):
    """W - 1, W and W + 1 rows: one window that is just not full, exactly full, and a second window of one row (a terminator)."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(300 + delta)
    b, q, r = _reads_with_rows(rng, W + delta, [100] * 300)
    for M in (2, 3):
        _, st = _all_ways(engine, b, q, r, None, M=M, m=3, k=8, B=1)
        assert st["n_rows"] == W + delta and st["qs_smoothed"] > 0


def test_terminators_on_window_borders_and_straddling_reads(engine):
    """A terminator on the last position of window 0, an empty read whose terminator is the first position of window 1, a
    read of 300 bases across the border of windows 1 and 2, reads of lengths 1 and 17 beside them."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(41)
    k1 = (W - 1) // 101
    lens = [100] * (k1 - 1)
    lens += [W - 1 - sum(lens) - len(lens)]                           # its terminator stands at W - 1
    assert sum(lens) + len(lens) - 1 == W - 1
    lens += [0, 1, 17]                                                # the empty read's terminator: position W
    pos = sum(lens) + len(lens)
    k2 = (2 * W - 150 - pos) // 101
    lens += [100] * (k2 - 1)
    pos = sum(lens) + len(lens)
    lens += [2 * W - 150 - pos - 1, 300]                              # the 300-base read starts 150 positions before 2 W
    assert sum(lens[:-1]) + len(lens) - 1 == 2 * W - 150
    b, q, r = _reads_with_rows(rng, 2 * W + 2000, lens)
    for M in (2, 1):
        _, st = _all_ways(engine, b, q, r, None, M=M, m=3, k=8, B=M - 1)
        assert st["qs_smoothed"] > 0


def test_smallest_collections(engine, orc):
    _all_ways(engine, A(b"A"), A(b"I"), np.array([0, 1], np.uint64), orc, m=2, k=1)                    # one read of one base
    _all_ways(engine, A(b""), A(b""), np.array([0], np.uint64))                                        # no rows
    _all_ways(engine, A(b""), A(b""), np.array([0, 0, 0], np.uint64), orc, m=2, k=1)                   # only empty reads
    rng = np.random.default_rng(11)
    b, q, r = _reads_with_rows(rng, 1 + 17 + 300 + 3, [1, 17])
    assert list(np.diff(r.astype(np.int64))) == [1, 17, 300]
    _all_ways(engine, b, q, r, orc, m=2, k=2, B=1)


def test_windows_of_terminators_only(engine):
    """More empty reads than two windows hold positions, then reads that get edited: whole windows of terminators."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(43)
    b, q, r = _reads_with_rows(rng, 2 * W + 500 + 40 * 101 + 1, [0] * (2 * W + 500) + [100] * 39)
    _, st = _all_ways(engine, b, q, r, None, m=3, k=8)
    assert st["qs_smoothed"] > 0 and st["n_reads"] == 2 * W + 540


def test_window_without_a_record_between_two_with(engine):
    """Windows 0 and 2 hold reads of a short genome (edited); between them lie unrelated random reads that cover window 1, none
    of whose rows differs from the input: under keep that window gets no record."""
    W, _ = _geometry(1)
    rng = np.random.default_rng(44)
    per = W // 101
    b0, q0, _ = _reads_with_rows(rng, per * 101, [100] * (per - 1))
    b2, q2, _ = _reads_with_rows(rng, per * 101, [100] * (per - 1))
    L1 = -(-(2 * W - per * 101) // per)                               # per random reads from below W to 2 W and beyond
    assert per * 101 <= W and per * 101 + per * (L1 + 1) >= 2 * W
    b1 = np.array(list(b"ACGT"), np.uint8)[rng.integers(0, 4, per * L1)]
    q1 = rng.integers(35, 75, per * L1).astype(np.uint8)
    b = np.concatenate([b0, b1, b2]); q = np.concatenate([q0, q1, q2])
    lens = [100] * per + [L1] * per + [100] * per
    r = np.zeros(len(lens) + 1, np.uint64); r[1:] = np.cumsum(lens)
    last, st = _all_ways(engine, b, q, r, None, m=3, k=24)
    ob, oq = last["out"]
    mid = slice(len(b0), len(b0) + len(b1))
    assert np.array_equal(ob[mid], b[mid]) and np.array_equal(oq[mid], q[mid])
    assert np.count_nonzero(oq[:len(b0)] != q0) > 0 and np.count_nonzero(oq[len(b0) + len(b1):] != q2) > 0


def test_two_bins_plus_one_row(engine):
    """Exactly two first-level bins plus one row, as tests/test_gpu_posbins.py builds it: a read of 300 bases across the first
    border, and the last terminator alone in the third bin."""
    W, s1 = _geometry(100000)
    bin1 = 1 << s1
    rows = 2 * bin1 + 1
    assert _geometry(rows) == (W, s1)
    rng = np.random.default_rng(5)
    k1 = (bin1 - 150) // 101
    lens = [100] * (k1 - 1) + [bin1 - 150 - 101 * (k1 - 1) - 1, 300]
    pos = sum(lens) + len(lens)
    k2 = (2 * bin1 - 17 - pos) // 101
    lens += [100] * (k2 - 1)
    pos = sum(lens) + len(lens)
    lens += [2 * bin1 - 17 - pos - 1]
    b, q, r = _reads_with_rows(rng, rows, lens)
    assert int(r[-1] - r[-2]) == 17 and int(r[-1]) + len(r) - 2 == 2 * bin1
    _, st = _all_ways(engine, b, q, r, None, M=3, m=3, k=8)
    assert st["n_rows"] == rows and st["qs_smoothed"] > 0


def test_bins_of_several_windows(engine):
    """Above 512 windows: first-level bins of two windows with head, gap and tail; the second level really partitions."""
    b, q, r = _several_windows_input()
    last, st = _all_ways(engine, b, q, r, None, m=5, B=1)
    assert st["n_rows"] == len(b) + len(r) - 1 and st["modified"] > 0
    assert 0 < last["default"][1] < len(b) // 2


def test_poly_g_block(engine, orc):
    """Clusters far above CL_BIG rows (k_big_*), whose edits are row-local too."""
    rng = np.random.default_rng(77)
    N, L = 1500, 100
    b = np.full(N * L, ord("G"), np.uint8)
    hit = rng.random(N * L) < 0.01
    b[hit] = np.array(list(b"ACTN"), np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    q = rng.integers(35, 75, N * L).astype(np.uint8)
    r = np.arange(N + 1, dtype=np.uint64) * L
    for M in (1, 2):
        _, st = _all_ways(engine, b, q, r, None, m=5, M=M, B=1)
        assert st["qs_smoothed"] > 2048


@pytest.mark.parametrize("M,B", [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1)])
def test_all_modes(engine, M, B):
    b, q, r = api.synth_host(api.synth_spec(2000, 100, seed=4100 + 2 * M + B, coverage=25))
    _, st = _all_ways(engine, b, q, r, None, M=M, B=B, m=5)
    assert st["qs_smoothed"] > 0 and st["modified"] > 0


def test_small_case_against_the_oracle(engine, orc):
    b, q, r = api.synth_host(api.synth_spec(100, 100, seed=7, coverage=25))
    for M, B in ((1, 1), (2, 0), (2, 1), (3, 0)):
        _all_ways(engine, b, q, r, orc, M=M, B=B, m=3)


def test_const_is_refused_without_m2(engine):
    b, q, r = api.synth_host(api.synth_spec(100, 50, seed=3, coverage=25))
    try:
        _set_env({"BFQ_POSBIN_POLARITY": "const"})
        engine.set_params(**dict(BASE, M=1))
        with pytest.raises(Exception, match="const"):
            _device_run(engine, b, q, r)
    finally:
        _set_env({})
        engine.set_params()
    _all_ways(engine, b, q, r, None, M=1)                             # and the context goes on working


def test_inputs_aligned_otherwise_than_outputs(engine):
    """The last kernel reads the inputs in 16-byte pieces only where they are aligned like the outputs: bases one byte and
    qualities five bytes off, in exact-size views (three windows, both polarities), against the walks on the same views."""
    torch = pytest.importorskip("torch")
    W, _ = _geometry(1)
    rng = np.random.default_rng(47)
    b, q, r = _reads_with_rows(rng, 2 * W + 700, [100] * 500)
    dev = torch.device("cuda:0")
    n = len(b)
    hb = torch.zeros(n + 64, dtype=torch.uint8, device=dev); hq = torch.zeros_like(hb)
    db, dq = hb[1:1 + n], hq[5:5 + n]
    db.copy_(torch.from_numpy(b).to(dev)); dq.copy_(torch.from_numpy(q).to(dev))
    dr = torch.from_numpy(r.astype(np.int64)).to(dev)
    assert db.data_ptr() % 16 == 1 and dq.data_ptr() % 16 == 5
    got = {}
    try:
        for name, env in _ways(2):
            _set_env(env)
            engine.set_params(**dict(BASE, m=3, k=8, B=1))
            ob = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev); oq = torch.full_like(ob, 0xEE)
            assert ob.data_ptr() % 16 == 0 and oq.data_ptr() % 16 == 0
            st = engine.run_reads_device(db.data_ptr(), dq.data_ptr(), dr.data_ptr(), len(r) - 1, n, ob.data_ptr(), oq.data_ptr())
            torch.cuda.synchronize()
            got[name] = (ob.cpu().numpy(), oq.cpu().numpy(), st)
    finally:
        _set_env({})
        engine.set_params()
    wb, wq, wst = got["walks"]
    assert wst["qs_smoothed"] > 0
    for name, (ob, oq, st) in got.items():
        assert np.array_equal(ob, wb) and np.array_equal(oq, wq) and st == wst, name


def test_profile_names(engine):
    """The three stages launch under their names whichever way, k_posbin_check in the chunked forms, even with nothing to send."""
    rng = np.random.default_rng(31)
    b = np.array(list(b"ACGT"), np.uint8)[rng.integers(0, 4, 3000)]
    q = rng.integers(35, 75, 3000).astype(np.uint8)
    r = np.arange(31, dtype=np.uint64) * 100
    seen = {}
    try:
        for name, env in (("default", {}), ("dense", {"BFQ_POSBIN_SPARSE": "0"}), ("runs", {"BFQ_POSBIN_WC": "0"})):
            _set_env(env)
            engine.set_params(**BASE)
            engine.prof_reset()
            _device_run(engine, b, q, r)
            seen[name] = {k for k, v in engine.prof().items() if v["launches"]}
            assert engine.posbin_sparse_last() == ((KEEP, 0) if name == "default" else (-1, 0))
    finally:
        _set_env({})
        engine.set_params()
    assert STAGES | {"k_posbin_check"} <= seen["default"] and STAGES | {"k_posbin_check"} <= seen["dense"]
    assert STAGES <= seen["runs"] and "k_posbin_check" not in seen["runs"]


@pytest.mark.parametrize("byte", [0xC3, 0x41])
def test_poisoned_workspace(engine, byte):
    """The arena holds the byte when the call starts: the gaps of partially filled bins and windows (never written) must not
    reach the result.  The reference is the unpoisoned LF-walk run."""
    cases = [(_several_windows_input(), dict(m=5, B=1)), (_flip_input(25), dict(M=2, m=5)), (_flip_input(6), dict(M=2, m=5))]
    refs = []
    try:
        _set_env({"BFQ_POSBINS": "0"})
        for (b, q, r), par in cases:
            engine.set_params(**dict(BASE, **par))
            refs.append(_device_run(engine, b, q, r))
    finally:
        _set_env({})
        engine.set_params()
    old = os.environ.get("BFQ_POISON")
    os.environ["BFQ_POISON"] = "0x%02X" % byte
    try:
        e = api.Engine(0)
        try:
            for ((b, q, r), par), (wb, wq, wst) in zip(cases, refs):
                full = dict(BASE, **par)
                for name, env in _ways(2)[:3]:
                    _set_env(env)
                    e.set_params(**full)
                    ob, oq, ost = _device_run(e, b, q, r)
                    pol, sent = e.posbin_sparse_last()
                    assert np.array_equal(ob, wb) and np.array_equal(oq, wq) and ost == wst, (name, byte, par)
                    assert sent == _differ(b, q, wb, wq, pol, full), (name, byte, par)
        finally:
            e.close()
    finally:
        _set_env({})
        if old is None:
            os.environ.pop("BFQ_POISON", None)
        else:
            os.environ["BFQ_POISON"] = old
