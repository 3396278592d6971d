"""GPU tests of the read reordering (bfq_fastq_reorder / bfq_fastq_reorder_fd / dropin/bfq_reorder / parallel.py --reorder):
the output text and the permutation are pinned, byte for byte, to the numpy restatement of the interface
(tests/reorder_model.py); then what the reorder is for -- nothing changes for one block, and eight blocks of a reordered
collection keep more of their clusters than eight blocks of the input order.  Golden inputs: `example` is the reference's
example/reads.fastq, paired_inputs() its reads_1 / reads_2."""
import os, subprocess, sys
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import reorder_model as model, util
from tests.test_parallel_gloo import paired_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dropin", "bfq_reorder")
E_ARG, E_TOO_LONG, E_NOMEM = -1, -5, -7
SENTINEL = 0xA5
COUNTERS = ("num_clust", "num_clust_discarded", "num_clust_amb_discarded", "num_clust_mod", "num_clust_alleq", "bases_inside",
            "qs_smoothed", "modified")


def _raw(name):
    return open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read()


def _check(engine, texts, **kw):
    """engine.fastq_reorder == model, text and permutation; returns the permutation."""
    want, wperm = model.reorder(texts, **kw)
    got, perm = engine.fastq_reorder(texts, **kw)
    assert len(got) == len(texts)
    for g, w, t in zip(got, want, texts):
        assert len(g) == len(t) + (1 if t and not t.endswith(b"\n") else 0)
        assert g.tobytes() == w
    assert np.array_equal(perm, wperm)
    return perm


def test_golden_inputs(engine, tmp_path):
    f1, f2 = paired_inputs(str(tmp_path))
    cases = [[_raw("example")], [open(f1, "rb").read(), open(f2, "rb").read()], [_raw("synth_var")], [_raw("synth_fix")]]
    for texts in cases:
        for kw in (dict(), dict(k=8), dict(k=32), dict(mode=1), dict(mode=1, seed=12345)):
            perm = _check(engine, texts, **kw)
            assert sorted(perm) == list(range(len(perm)))
    perm = _check(engine, cases[2])
    assert not np.array_equal(perm, np.arange(len(perm)))


def _collection(rng, n, lmin, lmax, p_n=0.05, dup=0.2, crlf=False, plus_text=False, final_newline=True):
    b, q, r = util.random_reads(rng, n, lmin, lmax, p_n=p_n, dup=dup)
    eol = b"\r\n" if crlf else b"\n"
    recs = []
    for i in range(n):
        s, e = int(r[i]), int(r[i + 1])
        hdr = b"@" + bytes(rng.integers(48, 123, int(rng.integers(0, 60))).astype(np.uint8))
        plus = b"+" + (hdr[1:] if plus_text and i % 2 else b"")
        recs.append(hdr + eol + b[s:e].tobytes() + eol + plus + eol + q[s:e].tobytes() + eol)
    text = b"".join(recs)
    return text if final_newline or not text else text[:-len(eol)]


def test_random_collections(engine):
    rng = np.random.default_rng(20241101)
    texts = [_collection(rng, 500, 1, 300),
             _collection(rng, 3000, 15, 120, p_n=0.3),                              # N-heavy: many reads without a window
             _collection(rng, 4000, 30, 150, dup=0.5),                              # ties: the stable order shows
             _collection(rng, 800, 1, 300, crlf=True, plus_text=True),
             _collection(rng, 700, 20, 90, plus_text=True, final_newline=False),
             _collection(rng, 300, 20, 90, crlf=True, final_newline=False),
             _collection(rng, 1, 100, 100), _collection(rng, 1, 1, 1), _collection(rng, 1, 50, 50, final_newline=False), b""]
    for t in texts:
        for kw in (dict(), dict(k=8), dict(k=32), dict(mode=1, seed=1)):
            _check(engine, [t], **kw)
    # mates of different read lengths; mate 1 N-heavy so that mate 2 lends its key
    m1, m2 = _collection(rng, 2500, 10, 60, p_n=0.3), _collection(rng, 2500, 30, 200, crlf=True)
    _check(engine, [m1, m2]); _check(engine, [m1, m2], k=8); _check(engine, [m1, m2], mode=1, seed=9)
    # the duplicates' order: equal keys keep their input order
    perm = _check(engine, [texts[2]])
    a, _, _, st, ln = model.records(texts[2])
    keys, _ = model.locus_keys(a, st, ln, 21)
    ks = keys[perm.astype(np.int64)]
    assert (np.diff(ks.astype(np.int64)) >= 0).all() and (np.diff(ks.astype(np.int64)) == 0).sum() > 500
    tie = np.flatnonzero(np.diff(ks.astype(np.int64)) == 0)
    assert (perm[tie + 1] > perm[tie]).all()
    # mode 1: seeded -- two seeds, two orders, each twice the same
    pa, pb = engine.fastq_reorder([texts[0]], mode=1, seed=1)[1], engine.fastq_reorder([texts[0]], mode=1, seed=2)[1]
    assert not np.array_equal(pa, pb)
    assert np.array_equal(pa, engine.fastq_reorder([texts[0]], mode=1, seed=1)[1])
    assert np.array_equal(pb, engine.fastq_reorder([texts[0]], mode=1, seed=2)[1])


def _synth_text(engine, n, L, **kw):
    sp = api.synth_spec(n, L, **kw)
    buf = np.empty(n * (2 * L + 40), np.uint8)
    return buf[:engine.synth_fastq(sp, buf)]


@pytest.fixture(scope="module")
def coll200k(engine):
    """200 000 x 100 bp of the synthetic generator at its defaults: coverage 30, both strands, default error rates."""
    return _synth_text(engine, 200_000, 100)


def test_one_million_reads(engine):
    """Several radix tiles and blocks, a text of 230 MB."""
    text = _synth_text(engine, 1_000_000, 100, seed=11)
    want, wperm = model.reorder([text.tobytes()])
    out = np.empty(len(text) + 64, np.uint8)
    (got,), perm = engine.fastq_reorder([text], out=[out])
    assert np.array_equal(perm, wperm)
    assert len(got) == len(text) and got.tobytes() == want[0]
    assert engine.prof()["k_reorder_keys"]["launches"] >= 1 and engine.prof()["k_reorder_gather"]["launches"] >= 1
    pin = api.PinnedBuffer(len(text) + 64)                             # a pinned destination: direct DMA
    try:
        (got,), perm = engine.fastq_reorder([text], mode=1, seed=5, out=[pin.array])
        w1, p1 = model.reorder([text.tobytes()], mode=1, seed=5)
        assert np.array_equal(perm, p1) and got.tobytes() == w1[0]
    finally:
        pin.free()


def test_nothing_changes_for_one_block(engine, coll200k):
    """The unsharded run does not care about the order of the reads: all eight cluster counters are the same."""
    (re,), perm = engine.fastq_reorder([coll200k])
    assert len(perm) == 200_000 and not np.array_equal(perm, np.arange(200_000))
    a = engine.fastq_job([coll200k]).stats
    b = engine.fastq_job([re]).stats
    print("unsharded, input order:", {k: a[k] for k in COUNTERS})
    print("unsharded, reordered  :", {k: b[k] for k in COUNTERS})
    assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS}


def test_eight_blocks_keep_more_clusters(engine, coll200k, tmp_path):
    """What the reorder is for: parallel.run_files with t = 8 on one GPU, with and without --reorder 2 -- bases inside
    clusters and bases modified, summed over the blocks, are both strictly larger with the reorder."""
    src = str(tmp_path / "c.fastq")
    coll200k.tofile(src)
    plain = parallel.run_files(engine, parallel.Comm(), [src], 8, parallel.output_names([src], str(tmp_path / "P"), False))
    new = parallel.reorder_inputs(engine, parallel.Comm(), [src], 2)
    assert new == [str(tmp_path / "c.reordered.fastq")]
    reo = parallel.run_files(engine, parallel.Comm(), new, 8, parallel.output_names(new, str(tmp_path / "R"), False))
    one = engine.fastq_job([coll200k]).stats
    for name, st in (("unsharded", one), ("8 blocks", plain["stats"]), ("8 blocks reordered", reo["stats"])):
        print(f"{name}: bases_inside {st['bases_inside']} modified {st['modified']} qs_smoothed {st['qs_smoothed']}")
    assert plain["blocks"] == reo["blocks"] == 8 and plain["reads"] == reo["reads"] == 200_000
    assert reo["stats"]["bases_inside"] > plain["stats"]["bases_inside"]
    assert reo["stats"]["modified"] > plain["stats"]["modified"]


def _refused(engine, code, texts, sizes=None, match=None, **kw):
    outs = [np.full(s if sizes is None else sizes[i], SENTINEL, np.uint8) for i, s in enumerate(len(t) + 16 for t in texts)]
    with pytest.raises(api.BfqError, match=match) as e:
        engine.fastq_reorder(texts, out=outs, **kw)
    assert e.value.code == code, str(e.value)
    assert all((o == SENTINEL).all() for o in outs)
    return str(e.value)


def test_refusals_leave_the_output_untouched(engine, coll200k, tmp_path):
    rng = np.random.default_rng(5)
    good = _collection(rng, 400, 30, 120)
    lines = good.split(b"\n")
    # what bfq_fastq_run says about the same text is what the reorder says
    for bad in (b"\n".join(lines[:4 * 200 + 3]) + b"\n",                           # a truncated record
                b"\n".join(lines[:4 * 100 + 3] + [lines[4 * 100 + 3][:-1]] + lines[4 * 101:])):   # a quality line one byte short
        with pytest.raises(api.BfqError) as ref:
            engine.fastq_run(bad)
        msg = _refused(engine, ref.value.code, [bad])
        assert msg == str(ref.value) and ref.value.code == E_ARG
    long = b"@l\n" + b"A" * 65001 + b"\n+\n" + b"I" * 65001 + b"\n"
    with pytest.raises(api.BfqError) as ref:
        engine.fastq_run(long)
    assert _refused(engine, E_TOO_LONG, [good + long]) == str(ref.value)
    # mates with different record counts; a bad mate 2
    other = _collection(rng, 399, 30, 120)
    _refused(engine, E_ARG, [good, other], match="400 in the first file, 399 in the second")
    _refused(engine, E_ARG, [good, b"\n".join(lines[:-2]) + b"\n"], match="multiple of 4")
    # parameters
    _refused(engine, E_ARG, [good], mode=3); _refused(engine, E_ARG, [good], mode=0)
    _refused(engine, E_ARG, [good], k=7); _refused(engine, E_ARG, [good], k=33)
    _refused(engine, E_ARG, [good, good, good])
    # capacity one byte short (with and without the supplied newline); exactly enough is enough
    _refused(engine, E_ARG, [good], sizes=[len(good) - 1], match="output buffer")
    _refused(engine, E_ARG, [good[:-1]], sizes=[len(good) - 1], match="output buffer")
    _refused(engine, E_ARG, [good, good], sizes=[len(good), len(good) - 1], match="output buffer")
    out = np.full(len(good), SENTINEL, np.uint8)
    (got,), _ = engine.fastq_reorder([good[:-1]], out=[out])
    assert got.tobytes() == model.reorder([good])[0][0]
    # a workspace cap below input + output + index: BFQ_E_NOMEM with the size, before anything is written; the engine goes on
    small = api.Engine(0, ws_cap_mib=100)
    try:
        msg = _refused(small, E_NOMEM, [coll200k], match="GiB")
        assert "cap" in msg and "input + output" in msg
        (got,), _ = small.fastq_reorder([good])
        assert got.tobytes() == model.reorder([good])[0][0]
        # ... and through the files: the outputs are left empty
        src, dst = str(tmp_path / "big.fastq"), str(tmp_path / "big.out")
        coll200k.tofile(src)
        with pytest.raises(api.BfqError) as e:
            small.fastq_reorder_files([src], [dst])
        assert e.value.code == E_NOMEM and os.path.getsize(dst) == 0
    finally:
        small.close()
    bad, dst = str(tmp_path / "bad.fastq"), str(tmp_path / "bad.out")
    open(bad, "wb").write(b"\n".join(lines[:4 * 200 + 3]) + b"\n")
    with pytest.raises(api.BfqError) as e:
        engine.fastq_reorder_files([bad], [dst])
    assert e.value.code == E_ARG and os.path.getsize(dst) == 0


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, **kw)


def test_tool_and_driver(engine, coll200k, tmp_path):
    """dropin/bfq_reorder on files == the API; `parallel.py IN -t 4 --reorder 2` == the same command without the flag on
    the tool's output."""
    assert os.path.exists(TOOL), f"{TOOL} missing: run __graft_entry__.build()"
    tmp = str(tmp_path)
    f1, f2 = paired_inputs(tmp)
    big = os.path.join(tmp, "big.fastq")
    coll200k.tofile(big)
    nonl = os.path.join(tmp, "nonl.fastq")
    open(nonl, "wb").write(_raw("synth_var")[:-1])
    for src in (os.path.join(util.GOLDEN, "example.fastq"), nonl, big):
        text = open(src, "rb").read()
        for flags, kw in (([], {}), (["-r", "1", "-s", "7"], dict(mode=1, seed=7)), (["-k", "12"], dict(k=12))):
            r = _run([TOOL, "-i", src, "-o", os.path.join(tmp, "o.fq"), "-V"] + flags)
            assert r.returncode == 0 and b"[bfq phases]" in r.stdout and b"reads" in r.stdout, r.stdout
            (want,), _ = engine.fastq_reorder([text], **kw)
            assert open(os.path.join(tmp, "o.fq"), "rb").read() == want.tobytes(), (src, flags)
    t1, t2 = open(f1, "rb").read(), open(f2, "rb").read()
    for flags, kw in (([], {}), (["-r", "1", "-s", "7"], dict(mode=1, seed=7))):
        r = _run([TOOL, "-i", f1, "-j", f2, "-o", os.path.join(tmp, "o1.fq"), "-p", os.path.join(tmp, "o2.fq")] + flags)
        assert r.returncode == 0, r.stdout
        (w1, w2), _ = engine.fastq_reorder([t1, t2], **kw)
        assert open(os.path.join(tmp, "o1.fq"), "rb").read() == w1.tobytes() and open(os.path.join(tmp, "o2.fq"), "rb").read() == w2.tobytes()
    # the file entry point of the engine
    sizes, n = engine.fastq_reorder_files([f1, f2], [os.path.join(tmp, "e1.fq"), os.path.join(tmp, "e2.fq")])
    assert sizes == [len(t1), len(t2)] and n == 100
    assert open(os.path.join(tmp, "e1.fq"), "rb").read() == model.reorder([t1, t2])[0][0]
    # failures: exit 1, the message, empty outputs
    bad = os.path.join(tmp, "bad.fastq")
    open(bad, "wb").write(t1[:len(t1) // 2])
    for cmd in ([TOOL, "-i", bad, "-o", os.path.join(tmp, "b.fq")], [TOOL, "-i", f1, "-j", bad, "-o", os.path.join(tmp, "b.fq"), "-p", os.path.join(tmp, "b2.fq")],
                [TOOL, "-i", f1, "-o", os.path.join(tmp, "b.fq"), "-k", "40"]):
        r = _run(cmd)
        assert r.returncode == 1 and b"bfq_reorder:" in r.stdout, r.stdout
        assert os.path.getsize(os.path.join(tmp, "b.fq")) == 0
    assert _run([TOOL, "-i", f1, "-j", f2, "-o", os.path.join(tmp, "b.fq")]).returncode == 1      # -j without -p: usage
    # the driver
    src = os.path.join(tmp, "drv.fastq")
    open(src, "wb").write(_raw("synth_var"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _run([sys.executable, "-m", "bfqzip_amd.parallel", src, "-t", "4", "--reorder", "2", "-o", os.path.join(tmp, "A")], env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout
    mid = os.path.join(tmp, "drv.reordered.fastq")
    assert _run([TOOL, "-i", src, "-o", os.path.join(tmp, "tool.fastq")]).returncode == 0
    assert open(mid, "rb").read() == open(os.path.join(tmp, "tool.fastq"), "rb").read()
    r = _run([sys.executable, "-m", "bfqzip_amd.parallel", os.path.join(tmp, "tool.fastq"), "-t", "4", "-o", os.path.join(tmp, "B")], env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout
    assert open(os.path.join(tmp, "A.fastq"), "rb").read() == open(os.path.join(tmp, "B.fastq"), "rb").read()
