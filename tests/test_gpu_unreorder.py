"""GPU tests of the way back from a reordering (bfq_fastq_reorder_keep / bfq_fastq_unreorder / bfq_fastq_restore_ordered, their
_fd forms, dropin/bfq_reorder -P / -u, dropin/bfq_restore -P, parallel.py --keep-order): the kept permutation is, byte for byte,
the BFQPERM1 container the model (tests/perm_model.py) makes of the permutation the existing call returns; un-reordering a
reordered text gives the input back; the ordered restore is the plain restore with its records moved as the model moves
them.  Every refusal is found before anything is written."""
import os, re, subprocess, sys
import numpy as np
import pytest
from bfqzip_amd import api, fastq, parallel
from tests import perm_model as pm, reorder_model as model, util
from tests.test_parallel_gloo import paired_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REORDER = os.path.join(ROOT, "dropin", "bfq_reorder")
RESTORE = os.path.join(ROOT, "dropin", "bfq_restore")
E_ARG, E_NOMEM = -1, -7
SENTINEL = 0xA5
SIZES = (0, 1, 2, 3, 65, 4097, 131_073)                              # w = 1, 1, 1, 2, 7, 13, 18


def _raw(name):
    return open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read()


def _collection(rng, n, lmin=0, lmax=300, crlf=False, plus_text=False, final_newline=True):
    """n records made like _collection of tests/test_gpu_reorder.py, the random draws taken at once: read lengths lmin..lmax,
    headers of 0..59 bytes after the '@'; every 7th read is empty with a bare '@' (a 6-byte record with LF lines)."""
    L = rng.integers(lmin, lmax + 1, n)
    H = rng.integers(0, 60, n)
    L[3::7] = 0
    H[3::7] = 0
    so, ho = np.concatenate([[0], np.cumsum(L)]), np.concatenate([[0], np.cumsum(H)])
    seq = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, int(so[-1]), p=[.24, .24, .24, .24, .04])].tobytes()
    qual = rng.integers(33, 75, int(so[-1])).astype(np.uint8).tobytes()
    hdr = rng.integers(48, 123, int(ho[-1])).astype(np.uint8).tobytes()
    eol = b"\r\n" if crlf else b"\n"
    recs = []
    for i in range(n):
        h = hdr[ho[i]:ho[i + 1]]
        plus = b"+" + (h if plus_text and i % 2 else b"")
        recs.append(b"@" + h + eol + seq[so[i]:so[i + 1]] + eol + plus + eol + qual[so[i]:so[i + 1]] + eol)
    text = b"".join(recs)
    return text if final_newline or not text else text[:-len(eol)]


def _nl(t):
    return t + (b"\n" if t and not t.endswith(b"\n") else b"")


@pytest.fixture(scope="module")
def sized():
    """One collection per read count of SIZES (short reads at the large counts), shared by the tests below."""
    rng = np.random.default_rng(20250301)
    return {n: _collection(rng, n, 0, 300 if n <= 4097 else 40, crlf=n == 65, plus_text=n in (3, 4097), final_newline=n not in (2, 4097))
            for n in SIZES}


def _kept(engine, texts, **kw):
    """fastq_reorder(keep=True) against the existing call and the model's container; returns (texts, container, perm)."""
    want, perm = engine.fastq_reorder(texts, **kw)
    got, z = engine.fastq_reorder(texts, keep=True, **kw)
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]
    opts = dict(mode=kw.get("mode", 2), k=kw.get("k", 21), seed=kw.get("seed", 0))
    assert len(z) == pm.bound(len(perm)) == api.perm_bound(len(perm))
    assert z.tobytes() == pm.encode(perm, opts=opts), (len(perm), kw)
    return [g.tobytes() for g in got], z, perm


def test_kept_permutation_is_the_models_container(engine, sized, tmp_path):
    f1, f2 = paired_inputs(str(tmp_path))
    cases = [[_raw("example")], [open(f1, "rb").read(), open(f2, "rb").read()], [_raw("synth_var")]] + [[sized[n]] for n in SIZES]
    cases.append([sized[4097], _collection(np.random.default_rng(1), 4097, 1, 80)])               # mates of another shape
    for texts in cases:
        _, z, perm = _kept(engine, texts)
        assert sorted(int(x) for x in perm) == list(range(len(perm)))
        got, opts = api.perm_decode(z)
        assert np.array_equal(got, perm) and opts == dict(mode=2, k=21, seed=0)
    _kept(engine, [sized[4097]], mode=1, seed=12345)
    _kept(engine, [sized[65]], k=8)
    assert engine.prof()["k_perm_pack"]["launches"] >= 1
    # through the files
    src, dst, pz = str(tmp_path / "a.fq"), str(tmp_path / "a.out"), str(tmp_path / "a.perm")
    open(src, "wb").write(sized[4097])
    want, z, perm = _kept(engine, [sized[4097]], mode=1, seed=3)
    sizes, n = engine.fastq_reorder_files([src], [dst], mode=1, seed=3, perm_path=pz)
    assert n == 4097 and sizes == [len(want[0])] and open(dst, "rb").read() == want[0] and open(pz, "rb").read() == z.tobytes()
    open(pz, "wb").write(b"x" * 100_000)                                                             # a longer file from before is cut
    engine.fastq_reorder_files([src], [dst], mode=1, seed=3, perm_path=pz)
    assert open(pz, "rb").read() == z.tobytes()


def test_unreorder_gives_the_input_back(engine, sized, tmp_path):
    rng = np.random.default_rng(20250302)
    texts = [sized[n] for n in SIZES] + [_collection(rng, 900, 0, 300, crlf=True, plus_text=True),
                                         _collection(rng, 700, 0, 90, plus_text=True, final_newline=False),
                                         _collection(rng, 300, 0, 20, crlf=True, final_newline=False), _raw("example")]
    for t in texts:
        (re_,), z, perm = _kept(engine, [t])
        (back,) = engine.fastq_unreorder([re_], z)
        assert back.tobytes() == _nl(t), len(perm)
    # mates: one permutation for both
    m1, m2 = _collection(rng, 2500, 0, 60), _collection(rng, 2500, 0, 300, crlf=True, final_newline=False)
    (r1, r2), z, perm = _kept(engine, [m1, m2])
    b1, b2 = engine.fastq_unreorder([r1, r2], z)
    assert b1.tobytes() == m1 and b2.tobytes() == _nl(m2)
    # a missing final newline on the way back as well; exactly enough room is enough
    out = np.full(len(m1), SENTINEL, np.uint8)
    (b1,) = engine.fastq_unreorder([r1[:-1]], z, out=[out])
    assert b1.tobytes() == m1
    # any permutation, not one the reorder made
    for t in (texts[5], texts[7], texts[8]):
        n = len(model.records(t)[1])
        p = rng.permutation(n).astype(np.uint64)
        (got,) = engine.fastq_unreorder([t], api.perm_encode(p))
        assert got.tobytes() == pm.unreorder([t], p)[0]
    p = rng.permutation(2500).astype(np.uint64)
    g1, g2 = engine.fastq_unreorder([m1, m2], pm.encode(p))
    assert [g1.tobytes(), g2.tobytes()] == pm.unreorder([m1, m2], p)
    assert engine.prof()["k_perm_invert"]["launches"] >= 3 and engine.prof()["k_reorder_gather"]["launches"] >= 1
    # through the files
    tmp = str(tmp_path)
    for name, data in (("m1", m1), ("m2", m2), ("p", pm.encode(p))):
        open(os.path.join(tmp, name), "wb").write(data)
    sizes, n = engine.fastq_unreorder_files([os.path.join(tmp, "m1"), os.path.join(tmp, "m2")], [os.path.join(tmp, "o1"), os.path.join(tmp, "o2")],
                                            os.path.join(tmp, "p"))
    assert n == 2500 and sizes == [len(m1), len(m2) + 1]
    assert [open(os.path.join(tmp, o), "rb").read() for o in ("o1", "o2")] == pm.unreorder([m1, m2], p)


def _headed(rng, nreads, lmin, lmax, **kw):
    b, q, r = util.random_reads(rng, nreads, lmin, lmax, **kw)
    hdrs = [b"@r%d/%d len=%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), int(r[i + 1] - r[i])) for i in range(nreads)]
    return fastq.format_fastq(b, q, r, hdrs)


@pytest.fixture(scope="module")
def reordered(engine):
    """A collection of 3000 reads of 1..300 bases with headers, reordered: (its text in run order, the container, perm)."""
    rng = np.random.default_rng(20250303)
    t = _headed(rng, 3000, 1, 300, p_n=0.1, dup=0.4)
    (re_,), z = engine.fastq_reorder([t], keep=True)
    return t, re_.tobytes(), np.array(z), api.perm_decode(z)[0]


@pytest.mark.parametrize("keep_headers", [False, True])
@pytest.mark.parametrize("compress", [1, 2, 3])
def test_ordered_restore_is_the_restore_unreordered(engine, reordered, tmp_path, compress, keep_headers):
    _, re_, pz, perm = reordered
    engine.set_params(m=3, k=8)
    try:
        z = engine.fastq_job([re_], keep_headers=keep_headers, fastq=False, streams=True, hdr=keep_headers, compress=compress)
    finally:
        engine.set_params()
    dna, qs, hdr = np.array(z.dna), np.array(z.qs), np.array(z.hdr) if keep_headers else None
    plain, nr = engine.fastq_restore(dna, qs, hdr)
    assert nr == 3000
    want = pm.unreorder([plain.tobytes()], perm)[0]
    assert want != plain.tobytes()
    got, nr = engine.fastq_restore(dna, qs, hdr, perm=pz)
    assert nr == 3000 and got.tobytes() == want
    assert engine.prof()["k_fq_format_ordered"]["launches"] >= 1
    pin = api.PinnedBuffer(len(want) + 64)                             # a pinned destination: direct DMA
    try:
        got, _ = engine.fastq_restore(dna, qs, hdr, out=pin.array, perm=pz)
        assert got.tobytes() == want
    finally:
        pin.free()
    out = np.full(len(want), SENTINEL, np.uint8)                       # exactly enough room is enough
    assert engine.fastq_restore(dna, qs, hdr, out=out, perm=pz)[0].tobytes() == want
    paths = {}
    for name, data in (("dna", dna), ("qs", qs), ("hdr", hdr), ("perm", pz)):
        if data is not None:
            paths[name] = str(tmp_path / name)
            data.tofile(paths[name])
    ol, nr = engine.fastq_restore_files(paths["dna"], paths["qs"], paths.get("hdr"), str(tmp_path / "back.fq"), perm_path=paths["perm"])
    assert (ol, nr) == (len(want), 3000) and open(str(tmp_path / "back.fq"), "rb").read() == want


def test_ordered_restore_of_two_members(engine, reordered):
    """Two blocks compressed separately and concatenated, as parallel.py --compress writes them: the permutation runs over
    both."""
    _, re_, pz, perm = reordered
    lines = re_.split(b"\n")
    cut = len(b"\n".join(lines[:4 * 1234])) + 1
    engine.set_params(m=3, k=8)
    try:
        za, zb = (engine.fastq_job([part], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1) for part in (re_[:cut], re_[cut:]))
    finally:
        engine.set_params()
    dna, qs, hdr = (np.concatenate([np.array(getattr(za, k)), np.array(getattr(zb, k))]) for k in ("dna", "qs", "hdr"))
    plain, nr = engine.fastq_restore(dna, qs, hdr)
    got, nr2 = engine.fastq_restore(dna, qs, hdr, perm=pz)
    assert nr == nr2 == 3000 and got.tobytes() == pm.unreorder([plain.tobytes()], perm)[0]


def test_round_trip_is_the_identity(engine, reordered):
    """K = 10000: no cluster forms, nothing is smoothed.  reorder -> job with the headers kept -> restore with the permutation
    gives back the input text itself (bare '+' lines, no CR)."""
    t, re_, pz, _ = reordered
    engine.set_params(k=10000)
    try:
        z = engine.fastq_job([re_], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1)
    finally:
        engine.set_params()
    got, nr = engine.fastq_restore(z.dna, z.qs, z.hdr, perm=pz)
    assert nr == 3000 and got.tobytes() == t
    plain, _ = engine.fastq_restore(z.dna, z.qs, z.hdr)
    assert plain.tobytes() == re_


def _poke(z, j, v):
    """The container (bytes) with entry j overwritten."""
    w = int.from_bytes(z[16:20], "little")
    big = int.from_bytes(z[pm.HDR:], "little")
    big = (big & ~(((1 << w) - 1) << (j * w))) | (v << (j * w))
    return z[:pm.HDR] + big.to_bytes(len(z) - pm.HDR, "little")


def _bad_containers(z, perm):
    """(name, bytes, what the message must say); the positions are the model's first_bad.  3000 entries of 12 bits."""
    z, n = bytes(z), len(perm)
    out = [("not a container", b"BFQPERM2" + z[8:], "not a BFQPERM1 container"), ("truncated", z[:-8], "not a BFQPERM1 container"),
           ("cut inside the header", z[:20], "not a BFQPERM1 container"), ("empty", b"", "not a BFQPERM1 container")]
    oor = _poke(z, 1500, 4095)
    for name, bad, where in (("a value twice", _poke(z, 17, int(perm[2000])), 2000), ("out of range", oor, 1500),
                             ("two faults", _poke(oor, 700, int(perm[1200])), 1200)):
        with pytest.raises(ValueError) as e:
            pm.decode(bad)
        assert e.value.args[0] == where, name
        out.append((name, bad, rf"entry {where}\b"))
    other = pm.encode(np.random.default_rng(0).permutation(n - 1))
    out.append(("another read count", other, rf"{n - 1} reads for .* {n} re"))
    return out


def test_refusals_leave_the_output_untouched(engine, reordered, tmp_path):
    t, re_, pz, perm = reordered
    engine.set_params(m=3, k=8)
    try:
        z = engine.fastq_job([re_], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1)
        other = engine.fastq_job([_headed(np.random.default_rng(1), 3000, 1, 300)], fastq=False, streams=True, compress=1)
    finally:
        engine.set_params()
    dna, qs, hdr = np.array(z.dna), np.array(z.qs), np.array(z.hdr)
    tmp = str(tmp_path)
    for name, data in (("re.fq", re_), ("dna", dna.tobytes()), ("qs", qs.tobytes()), ("hdr", hdr.tobytes())):
        open(os.path.join(tmp, name), "wb").write(data)
    P = lambda n: os.path.join(tmp, n)

    def refused(fn, match, code=E_ARG, size=len(re_) + 4096):
        out = np.full(size, SENTINEL, np.uint8)
        with pytest.raises(api.BfqError, match=match) as e:
            fn(out)
        assert e.value.code == code, str(e.value)
        assert (out == SENTINEL).all()
        return str(e.value)

    for name, bad, match in _bad_containers(pz.tobytes(), perm):
        refused(lambda out: engine.fastq_unreorder([re_], np.frombuffer(bad, np.uint8), out=[out]), match)
        refused(lambda out: engine.fastq_unreorder([re_, re_], np.frombuffer(bad, np.uint8), out=[out, out.copy()]), match)
        refused(lambda out: engine.fastq_restore(dna, qs, hdr, out=out, perm=np.frombuffer(bad, np.uint8)), match)
        # the streams' own faults are named first
        msg = refused(lambda out: engine.fastq_restore(dna, np.array(other.qs), hdr, out=out, perm=np.frombuffer(bad, np.uint8)), r"read \d+")
        assert "perm" not in msg, name
        # the files and the tools: exit 1, the message, empty outputs
        open(P("bad.perm"), "wb").write(bad)
        with pytest.raises(api.BfqError, match=match) as e:
            engine.fastq_unreorder_files([P("re.fq")], [P("o.fq")], P("bad.perm"))
        assert e.value.code == E_ARG and os.path.getsize(P("o.fq")) == 0
        with pytest.raises(api.BfqError, match=match) as e:
            engine.fastq_restore_files(P("dna"), P("qs"), P("hdr"), P("o2.fq"), perm_path=P("bad.perm"))
        assert e.value.code == E_ARG and os.path.getsize(P("o2.fq")) == 0
        if name in ("truncated", "a value twice", "another read count"):
            for cmd, o in (([REORDER, "-u", "-P", P("bad.perm"), "-i", P("re.fq"), "-o", P("t.fq")], "t.fq"),
                           ([RESTORE, "-d", P("dna"), "-q", P("qs"), "-H", P("hdr"), "-P", P("bad.perm"), "-o", P("t2.fq")], "t2.fq")):
                r = _run(cmd)
                assert r.returncode == 1 and re.search(match.encode(), r.stdout), r.stdout
                assert os.path.getsize(P(o)) == 0
    # room one byte short: the text, and the container of the keeping call (nothing is written then, the texts neither)
    refused(lambda out: engine.fastq_unreorder([re_], pz, out=[out]), "output buffer", size=len(re_) - 1)
    refused(lambda out: engine.fastq_restore(dna, qs, hdr, out=out, perm=pz), "output buffer", size=len(t) - 1)
    L = engine.L
    for cap in (0, 39, len(pz) - 1):
        out, zbuf = np.full(len(re_) + 16, SENTINEL, np.uint8), np.full(len(pz), SENTINEL, np.uint8)
        arrs, np_, tp, outs, ho, capv, ol = engine._text_parts([t], [out])
        zl, nr = api.C.c_uint64(9), api.C.c_uint64(9)
        O = api._lib.ReorderOpts(mode=2, k=21, seed=0)
        rc = L.bfq_fastq_reorder_keep(engine.h, tp, 1, api.C.byref(O), ho, capv, ol, api._ptr(zbuf), cap, api.C.byref(zl), api.C.byref(nr))
        assert rc == E_ARG and zl.value == 0 and ol[0] == 0 and (out == SENTINEL).all() and (zbuf == SENTINEL).all()
        assert b"permutation buffer" in L.bfq_last_error(engine.h)
    # a failing keeping call through the files leaves the permutation file empty too
    open(P("half.fq"), "wb").write(t[:len(t) // 2 + 1])
    open(P("k.perm"), "wb").write(b"old")
    with pytest.raises(api.BfqError):
        engine.fastq_reorder_files([P("half.fq")], [P("k.fq")], perm_path=P("k.perm"))
    assert os.path.getsize(P("k.fq")) == 0 and os.path.getsize(P("k.perm")) == 0
    # malformed text: what bfq_fastq_run says
    with pytest.raises(api.BfqError) as ref:
        engine.fastq_run(t[:len(t) // 2 + 1])
    msg = refused(lambda out: engine.fastq_unreorder([t[:len(t) // 2 + 1]], pz, out=[out]), None, code=ref.value.code)
    assert msg == str(ref.value)
    # -u without -P: usage
    r = _run([REORDER, "-u", "-i", P("re.fq"), "-o", P("t.fq")])
    assert r.returncode == 1 and b"usage" in r.stdout


@pytest.fixture(scope="module")
def coll200k(engine):
    """200 000 x 100 bp of the synthetic generator at its defaults (the collection of tests/test_gpu_reorder.py)."""
    sp = api.synth_spec(200_000, 100)
    buf = np.empty(200_000 * 240, np.uint8)
    return buf[:engine.synth_fastq(sp, buf)]


def test_workspace_cap(engine, sized, coll200k):
    """A cap below input + output + index: BFQ_E_NOMEM with the size, before anything is written; the engine goes on."""
    (re_,), z = engine.fastq_reorder([coll200k], keep=True)
    small = api.Engine(0, ws_cap_mib=100)
    try:
        out = np.full(len(coll200k) + 16, SENTINEL, np.uint8)
        with pytest.raises(api.BfqError, match="GiB") as e:
            small.fastq_unreorder([re_], z, out=[out])
        assert e.value.code == E_NOMEM and "cap" in str(e.value) and (out == SENTINEL).all()
        (r65,), z65 = small.fastq_reorder([sized[65]], keep=True)
        assert small.fastq_unreorder([r65], z65)[0].tobytes() == sized[65]
        # the ordered restore: the decoded streams, the text and the index
        job = engine.fastq_job([re_], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1)
        with pytest.raises(api.BfqError, match="GiB") as e:
            small.fastq_restore(job.dna, job.qs, job.hdr, out=out, perm=z)
        assert e.value.code == E_NOMEM and "cap" in str(e.value) and (out == SENTINEL).all()
    finally:
        small.close()


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, **kw)


def test_tools_round_trip_a_pair(engine, tmp_path):
    """bfq_reorder -P, then bfq_reorder -u -P: the two files come back; then the compressed route -- parallel.py --compress on
    the reordered files, bfq_restore -P per mate -- gives the un-reordered uncompressed output."""
    assert os.path.exists(REORDER) and os.path.exists(RESTORE), "tools missing: run __graft_entry__.build()"
    tmp = str(tmp_path)
    P = lambda n: os.path.join(tmp, n)
    f1, f2 = paired_inputs(tmp)
    t1, t2 = open(f1, "rb").read(), open(f2, "rb").read()
    r = _run([REORDER, "-i", f1, "-j", f2, "-o", P("ro1.fastq"), "-p", P("ro2.fastq"), "-P", P("pair.perm"), "-V"])
    assert r.returncode == 0 and b"[bfq phases]" in r.stdout, r.stdout
    (w1, w2), z = engine.fastq_reorder([t1, t2], keep=True)
    assert open(P("ro1.fastq"), "rb").read() == w1.tobytes() and open(P("ro2.fastq"), "rb").read() == w2.tobytes()
    assert open(P("pair.perm"), "rb").read() == z.tobytes()
    r = _run([REORDER, "-u", "-P", P("pair.perm"), "-i", P("ro1.fastq"), "-j", P("ro2.fastq"), "-o", P("b1.fastq"), "-p", P("b2.fastq"),
              "-r", "1", "-k", "99", "-s", "4"])                                                    # -r / -k / -s are ignored with -u
    assert r.returncode == 0, r.stdout
    assert open(P("b1.fastq"), "rb").read() == t1 and open(P("b2.fastq"), "rb").read() == t2
    # without the new options: as before
    assert _run([REORDER, "-i", f1, "-o", P("plain.fastq")]).returncode == 0
    assert open(P("plain.fastq"), "rb").read() == engine.fastq_reorder([t1])[0][0].tobytes()
    # the compressed route
    perm = pm.decode(z.tobytes())[0]
    inputs = [P("ro1.fastq"), P("ro2.fastq")]
    engine.set_params(m=5)
    try:
        plain = parallel.output_names(inputs, P("PL"), True)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, plain, paired=True, headers=True, want_streams=True, want_hdr=True)
        zz = parallel.output_names(inputs, P("Z"), True)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, zz, paired=True, headers=True, want_streams=True, want_hdr=True, compress=True)
    finally:
        engine.set_params()
    want = pm.unreorder([open(n["fastq"], "rb").read() for n in plain], perm)
    for o in range(2):
        r = _run([RESTORE, "-d", zz[o]["dna"] + ".bsc", "-q", zz[o]["qs"] + ".bsc", "-H", zz[o]["hdr"] + ".bsc", "-P", P("pair.perm"),
                  "-o", P(f"back{o}.fastq")])
        assert r.returncode == 0, r.stdout
        assert open(P(f"back{o}.fastq"), "rb").read() == want[o]
        # without -P: run order, as before
        assert _run([RESTORE, "-d", zz[o]["dna"] + ".bsc", "-q", zz[o]["qs"] + ".bsc", "-H", zz[o]["hdr"] + ".bsc", "-o", P("ro.fastq")]).returncode == 0
        assert open(P("ro.fastq"), "rb").read() == open(plain[o]["fastq"], "rb").read()


def test_driver_keeps_the_order_of_200k_reads(engine, coll200k, tmp_path):
    """`parallel.py IN -t 4 --reorder 2 --keep-order` on the 200 000-read synthetic collection: the model's un-reordering of
    the run without the flag, and the .perm file of the kept permutation."""
    tmp = str(tmp_path)
    text = coll200k
    src = os.path.join(tmp, "c.fastq")
    text.tofile(src)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _run([sys.executable, "-m", "bfqzip_amd.parallel", src, "-t", "4", "--reorder", "2", "--keep-order", "-o", os.path.join(tmp, "K")], env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout
    permfile = os.path.join(tmp, "c.reordered.fastq.perm")
    _, wperm = engine.fastq_reorder([text])
    assert open(permfile, "rb").read() == pm.encode(wperm, opts=dict(mode=2, k=21, seed=0))
    engine.set_params(m=5)                                            # what the driver runs with
    try:
        names = parallel.output_names([os.path.join(tmp, "c.reordered.fastq")], os.path.join(tmp, "R"), False)
        parallel.run_files(engine, parallel.Comm(), [os.path.join(tmp, "c.reordered.fastq")], 4, names)
    finally:
        engine.set_params()
    assert open(os.path.join(tmp, "K.fastq"), "rb").read() == pm.unreorder([open(names[0]["fastq"], "rb").read()], wperm)[0]
    assert sorted(f for f in os.listdir(tmp) if f.startswith("K")) == ["K.fastq"]
