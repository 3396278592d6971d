"""GPU tests against the REFERENCE's own record, with no oracle in between: every path of the engine must reproduce the md5
of the FASTQ the compiled reference bfq_int wrote and the eight counters it printed, for the collections of
tests/golden/ref_wide* (make_golden.py --ref-wide: the input space of tests/soak_gpu.py -- plateaus of equal LCP, empty /
one-base / N-only reads, clusters beyond CL_BIG rows with two frequent symbols, qualities up to 126 and as raw bytes, the
whole range of -k -m -v -f -t in every (M,B) build).  Reads only tests/golden/."""
import numpy as np
import pytest
from bfqzip_amd import fastq
from tests import util

pytestmark = pytest.mark.gpu
CASES, TIES, _ = util.ref_wide()


def _par(c, **kw):
    return dict(k=c["k"], m=c["m"], v=c["v"], f=c["f"], t=c["t"], M=c["M"], B=c["B"], **kw)


def _same(c, ob, oq, roff, st, what):
    """The reference's output (it writes no headers: '@' lines) and its statistics block."""
    assert util.md5(fastq.format_fastq(np.asarray(ob), np.asarray(oq), roff)) == c["out_md5"], (what, c["id"])
    assert {k: st[k] for k in util.STAT_KEYS} == c["stats"], (what, c["id"])


@pytest.fixture(scope="module")
def ebwts(engine):
    """The engine's own eBWT / permuted qualities / LCP of every collection, once; the reference has inverted exactly these
    bytes back to the reads (the generator's identity check), so they are compared with their recorded md5."""
    engine.set_params()
    out = {}
    for c in CASES:
        bwt, qs, lcp = engine.build_ebwt(c["bases"], c["quals"], c["roff"])
        assert len(bwt) == c["n"] and util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], c["id"]
        out[c["id"]] = (bwt, qs, lcp)
    return out


PATHS = ["fused", "ebwt_nolcp", "ebwt_lcp", "piles1", "piles2", "compact", "compact_small", "posmode", "fastq_job"]


@pytest.mark.parametrize("path", PATHS)
def test_path_reproduces_the_reference(engine, ebwts, monkeypatch, path):
    if path.startswith("compact"):
        monkeypatch.setenv("BFQ_COMPACT", "1")                    # steps 2-4 without the LF table (k_compact.hip)
        if path == "compact_small":                               # levels in chunks / the queue in host memory; the LCP in pieces
            monkeypatch.setenv("BFQ_COMPACT_RING", "64"); monkeypatch.setenv("BFQ_COMPACT_WIN", "1000")
    if path == "posmode":
        torch = pytest.importorskip("torch")
        monkeypatch.setenv("BFQ_POSMODE", "1")                    # edits written to the text positions, no LF table, no walks
        dev = torch.device("cuda:0")
    done = 0
    try:
        for c in CASES:
            b, q, r = c["bases"], c["quals"], c["roff"]
            if path == "fastq_job" and c["family"] == "raw":
                continue                                          # raw bytes are no FASTQ text
            engine.set_params(**_par(c, piles={"piles1": 1, "piles2": 2}.get(path, 0)))   # (the environment is read here)
            if path in ("fused", "piles1", "piles2"):
                ob, oq, st = engine.run_reads(b, q, r)
                _same(c, ob, oq, r, st, path)
                if path == "piles1":                              # step 1 pile by pile: the same eBWT
                    bwt, qs, lcp = engine.build_ebwt(b, q, r)
                    assert util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], c["id"]
                    assert np.array_equal(lcp, ebwts[c["id"]][2]), c["id"]
            elif path == "fastq_job":
                res = engine.fastq_job([fastq.format_fastq(b, q, r)], fastq=True)
                assert util.md5(np.asarray(res.fastq).tobytes()) == c["out_md5"], c["id"]
                assert {k: res.stats[k] for k in util.STAT_KEYS} == c["stats"], c["id"]
            elif path == "posmode":
                n = max(len(b), 1)
                db = torch.zeros(n, dtype=torch.uint8, device=dev); dq = torch.zeros_like(db)
                db[:len(b)] = torch.from_numpy(b.copy()).to(dev); dq[:len(b)] = torch.from_numpy(q.copy()).to(dev)
                dr = torch.from_numpy(r.astype(np.int64)).to(dev)
                ob = torch.zeros_like(db); oq = torch.zeros_like(db)
                st = engine.run_reads_device(db.data_ptr(), dq.data_ptr(), dr.data_ptr(), len(r) - 1, len(b), ob.data_ptr(), oq.data_ptr())
                torch.cuda.synchronize()
                _same(c, ob.cpu().numpy()[:len(b)], oq.cpu().numpy()[:len(b)], r, st, path)
            else:
                bwt, qs, lcp = ebwts[c["id"]]
                if path != "ebwt_lcp":                            # bfq_int's job: the LCP deduced from the BWT alone
                    ob, oq, roff, st = engine.smooth_invert(bwt, qs)
                    assert np.array_equal(roff, r), c["id"]
                    _same(c, ob, oq, roff, st, path)
                if path != "ebwt_nolcp":                          # bfq_ext's job: the LCP given (the engine's own)
                    ob, oq, roff, st = engine.smooth_invert(bwt, qs, lcp)
                    assert np.array_equal(roff, r), c["id"]
                    _same(c, ob, oq, roff, st, path + " lcp")
            done += 1
    finally:
        monkeypatch.undo()
        engine.set_params()
    assert done == len(CASES) - (12 if path == "fastq_job" else 0)


@pytest.mark.parametrize("path", ["table", "compact"])
def test_tie_shuffled_ebwts_reproduce_the_reference(engine, monkeypatch, path):
    """eBWTs whose identical suffixes (and terminator rows) are in any order, as another step-1 tool may give them: bfq_int's
    job (LCP deduced from the BWT) in every (M,B) and K in {1,2,3,5,8}, with and without the LF table."""
    if path == "compact":
        monkeypatch.setenv("BFQ_COMPACT", "1")
    try:
        for c in TIES:
            engine.set_params(**_par(c))
            ob, oq, roff, st = engine.smooth_invert(c["bwt"], c["qs"])
            _same(c, ob, oq, roff, st, path)
    finally:
        monkeypatch.undo()
        engine.set_params()
    assert len(TIES) == 24
