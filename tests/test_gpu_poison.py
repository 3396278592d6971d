"""Every GPU entry-point family on a poisoned workspace (BFQ_POISON, include/bfqzip_hip.h: bfq_workspace_read).

All calls of a context carve their temporaries out of one device buffer that is kept between calls; a one-shot tool sees it
zero-filled, a long-lived Engine sees the leftovers of its earlier calls.  With BFQ_POISON=<byte> the library fills that
buffer with the byte whenever a call starts over in it, and every other device allocation once when it is made, so that a
forgotten clear, a pad that is too short or a read past an array's end meets a value chosen to hurt:

  0x00  what a fresh process sees: must pass, or this module is wrong
  0x41  'A': a valid base, a valid quality, a printable name byte, and 0x41414141 as a count
  0x0A  the newline every text kernel scans for
  0xFF  all-ones in every width

Every assertion is against the reference the family already has (recorded md5s and counters of the compiled reference, the
CPU statement of the codec, the Python models, zlib, the host forms), never against another run of the code under test.  The
case builders and the guarded-buffer helpers are imported from the models and the tests that own them.  The module keeps an
Engine of its own per byte (module scope), created after the variable is set.  Inputs stay at or under 3 MB: of
codec_cases.cases() the one case above that (reads_low_coverage, 4 MB) is left to tests/test_gpu_codec.py.  Nothing here
reaches an index width above 4 GiB or the multi-GPU drivers."""
import functools
import gzip
import os
import zlib
import numpy as np
import pytest
from bfqzip_amd import api, fastq
from oracle import orc
from tests import bam_model as BM
from tests import bam_patch_model as BP
from tests import bgzf_model as BG
from tests import codec_cases
from tests import compare_model as cm
from tests import deflate_cases as D
from tests import gzip_model as GZ
from tests import names_model as nm
from tests import perm_model as pm
from tests import quals_model as qm
from tests import reorder_model as rm
from tests import ubam_model as UB
from tests import util
from tests import test_gpu_bam_patch as t_patch
from tests import test_gpu_bgzf as t_bgzf
from tests import test_gpu_compare as t_cmp
from tests import test_gpu_deflate as t_defl
from tests import test_gpu_reference as t_ref
from tests import test_gpu_ubam as t_ubam
from tests import test_gpu_unreorder as t_unre
from tests import test_restore_groups_host as t_groups

pytestmark = pytest.mark.gpu
host = api.HostText
BYTES = (0x00, 0x41, 0x0A, 0xFF)
GUARD = 4096
SENT = 0xA5
E_ARG = -1
MAX_INPUT = 3_000_000
IDX = util.golden_index()
CASES, TIES, _ = util.ref_wide()
FAMILIES = ("empty", "prefix", "long", "tiny", "raw", "lowcx", "rand", "synth")


class poisoned:
    """BFQ_POISON=<byte> in the environment for the time of the block; what stood there before comes back."""

    def __init__(self, byte):
        self.value = "0x%02X" % byte

    def __enter__(self):
        self.old = os.environ.get("BFQ_POISON")
        os.environ["BFQ_POISON"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("BFQ_POISON", None)
        else:
            os.environ["BFQ_POISON"] = self.old


@pytest.fixture(scope="module", params=BYTES, ids=["0x%02X" % b for b in BYTES])
def eng(request):
    """An Engine of this module's own whose workspace and private allocations hold request.param before every call."""
    with poisoned(request.param):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 16)
            assert e.workspace_bytes() > 0 and (e.workspace_read(0, 1 << 16) == request.param).all()    # the switch is on for this engine
            yield e
        finally:
            e.close()


def _u8(b):
    return np.frombuffer(b, np.uint8)


def _lines(xs):
    return b"".join(x + b"\n" for x in xs)


# ---------------------------------------------------------------- engine core: the recorded reference of tests/golden/ref_wide*
def _core():
    first = {}
    for c in CASES:
        first.setdefault(c["family"], c)
    assert tuple(sorted(first)) == tuple(sorted(FAMILIES))
    cs = [first[f] for f in FAMILIES]
    assert all(len(c["bases"]) <= MAX_INPUT for c in cs)
    return cs


CORE = _core()


@pytest.mark.parametrize("path", t_ref.PATHS + ["capped"])
def test_engine_core(eng, monkeypatch, path):
    """Every path of tests/test_gpu_reference.py (and the capped mode through the FASTQ job, as test_capped_mode selects it:
    piles = 2) on the first collection of every family: the md5 of the reference's FASTQ and its eight counters."""
    if path.startswith("compact"):
        monkeypatch.setenv("BFQ_COMPACT", "1")
        if path == "compact_small":
            monkeypatch.setenv("BFQ_COMPACT_RING", "64"); monkeypatch.setenv("BFQ_COMPACT_WIN", "1000")
    if path == "posmode":
        torch = pytest.importorskip("torch")
        monkeypatch.setenv("BFQ_POSMODE", "1")
        dev = torch.device("cuda:0")
    done = 0
    try:
        for c in CORE:
            b, q, r = c["bases"], c["quals"], c["roff"]
            if path in ("fastq_job", "capped") and c["family"] == "raw":
                continue                                          # raw bytes are no FASTQ text
            eng.set_params(**t_ref._par(c, piles={"piles1": 1, "piles2": 2, "capped": 2}.get(path, 0)))   # (the environment is read here)
            if path in ("fused", "piles1", "piles2"):
                ob, oq, st = eng.run_reads(b, q, r)
                t_ref._same(c, ob, oq, r, st, path)
                if path == "piles1":
                    bwt, qs, _lcp = eng.build_ebwt(b, q, r)
                    assert util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], c["id"]
            elif path in ("fastq_job", "capped"):
                res = eng.fastq_job([fastq.format_fastq(b, q, r)], fastq=True)
                assert util.md5(np.asarray(res.fastq).tobytes()) == c["out_md5"], (path, c["id"])
                assert {k: res.stats[k] for k in util.STAT_KEYS} == c["stats"], (path, c["id"])
            elif path == "posmode":
                n = max(len(b), 1)
                db = torch.zeros(n, dtype=torch.uint8, device=dev); dq = torch.zeros_like(db)
                db[:len(b)] = torch.from_numpy(b.copy()).to(dev); dq[:len(b)] = torch.from_numpy(q.copy()).to(dev)
                dr = torch.from_numpy(r.astype(np.int64)).to(dev)
                ob = torch.zeros_like(db); oq = torch.zeros_like(db)
                st = eng.run_reads_device(db.data_ptr(), dq.data_ptr(), dr.data_ptr(), len(r) - 1, len(b), ob.data_ptr(), oq.data_ptr())
                torch.cuda.synchronize()
                t_ref._same(c, ob.cpu().numpy()[:len(b)], oq.cpu().numpy()[:len(b)], r, st, path)
            else:
                eng.set_params()
                bwt, qs, lcp = eng.build_ebwt(b, q, r)            # (the reference inverted exactly these bytes: their md5 is recorded)
                assert len(bwt) == c["n"] and util.md5(bwt.tobytes()) == c["bwt_md5"] and util.md5(qs.tobytes()) == c["qs_md5"], c["id"]
                eng.set_params(**t_ref._par(c))
                if path != "ebwt_lcp":
                    ob, oq, roff, st = eng.smooth_invert(bwt, qs)
                    assert np.array_equal(roff, r), c["id"]
                    t_ref._same(c, ob, oq, roff, st, path)
                if path != "ebwt_nolcp":
                    ob, oq, roff, st = eng.smooth_invert(bwt, qs, lcp)
                    assert np.array_equal(roff, r), c["id"]
                    t_ref._same(c, ob, oq, roff, st, path + " lcp")
            done += 1
    finally:
        monkeypatch.undo()
        eng.set_params()
    assert done == len(CORE) - (1 if path in ("fastq_job", "capped") else 0)


@pytest.mark.parametrize("path", ["table", "compact"])
def test_engine_core_tie_shuffled_ebwts(eng, monkeypatch, path):
    if path == "compact":
        monkeypatch.setenv("BFQ_COMPACT", "1")
    try:
        for c in TIES[:2]:
            eng.set_params(**t_ref._par(c))
            ob, oq, roff, st = eng.smooth_invert(c["bwt"], c["qs"])
            t_ref._same(c, ob, oq, roff, st, path)
    finally:
        monkeypatch.undo()
        eng.set_params()


# ---------------------------------------------------------------- FASTQ text: tests/golden/* and the CPU statements of the codecs
@functools.lru_cache(None)
def _golden(name):
    """(input text, the reference's OUT.fq, its 2~4p / 4~4p line streams, 1~4p of the input) -- read once, never changed"""
    raw = open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read()
    out = open(os.path.join(util.GOLDEN, name + ".M2B0.fq"), "rb").read()
    ref = out.split(b"\n")[:-1]
    src = raw.split(b"\n")
    if src[-1] == b"":
        src.pop()
    return raw, out, _lines(ref[1::4]), _lines(ref[3::4]), _lines(src[0::4])


@functools.lru_cache(None)
def _golden_containers(name):
    """what the CPU statement / the Python models make of the golden streams: the job's containers must be these bytes"""
    _, _, dna, qs, hdr = _golden(name)
    return orc.codec_encode(_u8(dna)).tobytes(), qm.choose(qs), nm.choose(hdr)


@pytest.mark.parametrize("name", list(IDX))
def test_fastq_text(eng, name):
    raw, want, dna, qs, hdr = _golden(name)
    assert len(raw) <= MAX_INPUT
    _b, _q, _r, _h, bwt, bqs, lcp = util.golden_set(name)
    try:
        eng.set_params()
        gb, gq, gl = eng.fastq_build_ebwt(raw)
        assert np.array_equal(gb, bwt) and np.array_equal(gq, bqs) and np.array_equal(gl, lcp)
        eng.set_params(m=5)
        out, st = eng.fastq_run(raw)
        assert out == want
        key = "M2B0 -m 5 -H"
        if key in IDX[name]["out"]:
            outh, sth = eng.fastq_run(raw, keep_headers=True)
            assert util.md5(outh) == IDX[name]["out"][key]
        d, q, h, _st = eng.fastq_run_streams(raw)
        assert d == dna and q == qs and h == hdr
        res = eng.fastq_job([raw], fastq=True)
        assert np.asarray(res.fastq).tobytes() == want
        z = eng.fastq_job([raw], keep_headers=True, fastq=True, streams=True, hdr=True, compress=True, names=True, quals=True)
        zd, zq, zh = _golden_containers(name)
        assert np.asarray(z.dna).tobytes() == zd and np.asarray(z.qs).tobytes() == zq and np.asarray(z.hdr).tobytes() == zh
        if key in IDX[name]["out"]:
            assert util.md5(np.asarray(z.fastq).tobytes()) == IDX[name]["out"][key]
    finally:
        eng.set_params()


# ---------------------------------------------------------------- codecs: the CPU statement, the Python models, the round trip
@functools.lru_cache(None)
def _codec_cases():
    return {k: v for k, v in codec_cases.cases().items() if len(v) <= MAX_INPUT}


@functools.lru_cache(None)
def _codec_want(name):
    return orc.codec_encode(_codec_cases()[name])


@pytest.mark.parametrize("name", sorted(_codec_cases()))
def test_codec(eng, name):
    data = _codec_cases()[name]
    blob = eng.stream_compress(data)
    want = _codec_want(name)
    assert len(blob) == len(want) and (np.asarray(blob) == want).all()
    back = eng.stream_decompress(blob)
    assert len(back) == len(data) and (np.asarray(back) == data).all()


@functools.lru_cache(None)
def _names_want():
    return {k: nm.container(v) for k, v in nm.edge_cases().items()}


def test_codec_names(eng):
    for name, data in nm.edge_cases().items():
        got = eng.names_compress(_u8(data), always=True)
        assert got.tobytes() == _names_want()[name], name
        assert eng.stream_decompress(got).tobytes() == data, name


@functools.lru_cache(None)
def _quals_want():
    return {k: qm.container(v) for k, v in qm.cases().items()}


def test_codec_quals(eng):
    for name, data in qm.cases().items():
        assert len(data) <= MAX_INPUT
        got = eng.quals_compress(_u8(data), always=True)
        assert got.tobytes() == _quals_want()[name], name
        assert eng.stream_decompress(got).tobytes() == data, name


# ---------------------------------------------------------------- the way back
def _z(raw):
    return orc.codec_encode(_u8(raw))


def test_restore(eng):
    """containers made by the CPU statement -> the text of fastq.restore_text: plain, in the order before a permutation,
    group by group"""
    for name in ("example", "synth_var"):
        _, want, dna, qs, hdr = _golden(name)
        zd, zq, zh = _z(dna), _z(qs), _z(hdr)
        out, nr = eng.fastq_restore(zd, zq)
        assert out.tobytes() == want == fastq.restore_text(dna, qs) and nr == IDX[name]["reads"]
        out, nr = eng.fastq_restore(zd, zq, zh)
        headed = fastq.restore_text(dna, qs, hdr)
        assert out.tobytes() == headed
        p = np.random.default_rng(len(want)).permutation(nr).astype(np.uint64)
        buf = np.full(len(headed) + 2 * GUARD, SENT, np.uint8)
        out, nr2 = eng.fastq_restore(zd, zq, zh, out=buf[GUARD:GUARD + len(headed)], perm=pm.encode(p))
        assert out.tobytes() == pm.unreorder([headed], p)[0] and nr2 == nr
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + len(headed):] == SENT).all()
    rng = np.random.default_rng(1)
    blocks = [t_groups._block(rng, n, tag=b"t%d" % n) for n in (400, 7, 1200)]
    dna, qs, hdr, _want = t_groups._archive(orc, blocks, cut_dna=(2,))
    text = b"".join(fastq.restore_text(d, q, h) for d, q, h in blocks)
    out, nr = eng.fastq_restore(dna, qs, hdr, groups=True)
    assert out.tobytes() == text and nr == 1607
    out, nr = eng.fastq_restore(dna, qs, hdr, groups=(1, 2))
    assert out.tobytes() == b"".join(fastq.restore_text(d, q, h) for d, q, h in blocks[1:]) and nr == 1207


@functools.lru_cache(None)
def _reorder_cases():
    rng = np.random.default_rng(20250301)
    one = t_unre._collection(rng, 4097, 0, 120, plus_text=True, final_newline=False)
    m1, m2 = t_unre._collection(rng, 700, 0, 60), t_unre._collection(rng, 700, 0, 300, crlf=True, final_newline=False)
    out = []
    for texts, kw in (([_golden("synth_var")[0]], dict(mode=2)), ([one], dict(mode=1, seed=12345)), ([one], dict(mode=2, k=8)), ([m1, m2], dict(mode=2)),
                      ([m1, m2], dict(mode=1, seed=3))):
        opts = dict(mode=kw.get("mode", 2), k=kw.get("k", 21), seed=kw.get("seed", 0))
        want, perm = rm.reorder(texts, **opts)
        out.append((texts, kw, want, pm.encode(perm, opts=opts), perm))
    return out


def test_reorder_and_unreorder(eng):
    for texts, kw, want, wz, perm in _reorder_cases():
        got, z = eng.fastq_reorder(texts, keep=True, **kw)
        assert [g.tobytes() for g in got] == want, kw
        assert z.tobytes() == wz, kw
        back = eng.fastq_unreorder(want, wz)
        assert [b.tobytes() for b in back] == pm.unreorder(want, perm) == [t_unre._nl(t) for t in texts], kw
        p = np.random.default_rng(len(perm)).permutation(len(perm)).astype(np.uint64)      # any permutation, not one the reorder made
        outs = [np.full(len(t_unre._nl(t)) + 2 * GUARD, SENT, np.uint8) for t in texts]
        got = eng.fastq_unreorder(texts, pm.encode(p), out=[o[GUARD:len(o) - GUARD] for o in outs])
        assert [g.tobytes() for g in got] == pm.unreorder(texts, p), kw
        assert all((o[:GUARD] == SENT).all() and (o[len(o) - GUARD:] == SENT).all() for o in outs)


@functools.lru_cache(None)
def _compare_cases():
    out = []
    for name in ("example", "synth_var"):
        a, b = _golden(name)[:2]
        out.append(([a], [b], None, cm.compare([a], [b], max_diffs=10 ** 6)))
    a, b = _golden("synth_fix")[:2]
    N = IDX["synth_fix"]["reads"]
    perm = np.random.default_rng(5).permutation(N).astype(np.uint64)
    rb = t_cmp.record_list(b)
    moved = b"".join(rb[int(v)] for v in perm)
    ra = t_cmp.record_list(a)
    cut = len(b"".join(ra[:len(ra) // 2 + 1]))                        # A in two parts, cut between two records
    out.append(([a[:cut], a[cut:]], [moved], perm, cm.compare([a], [moved], perm=perm, max_diffs=10 ** 6)))
    return out


def test_compare(eng):
    for a_parts, b_parts, perm, M in _compare_cases():
        permz = pm.encode(perm) if perm is not None else None
        for md in (1, 100, M["n_diffs"] + 1):
            t_cmp.check(eng, a_parts, b_parts, M, md, permz=_u8(permz) if permz is not None else None)


# ---------------------------------------------------------------- inflate: zlib's text, the host form's statistics
@functools.lru_cache(None)
def _bgzf_cases():
    out = {"synth-c4096-l9": BG.matrix()["synth-c4096-l9"], "synth-c700-stored": BG.matrix()["synth-c700-stored"],
           "synth-c700-fixed": BG.matrix()["synth-c700-fixed"]}
    out.update(BG.crafted())
    return {k: (v, BG.expected(v)) for k, v in out.items()}


def test_inflate_bgzf(eng):
    import torch
    cases = _bgzf_cases()
    assert len(BG.directory(cases["synth-c4096-l9"][0])) > 40            # more than one member, more than one workgroup
    for name, (blob, text) in cases.items():
        assert len(blob) <= MAX_INPUT and len(text) <= MAX_INPUT
        t_bgzf.inflate_guarded(eng, blob, text)
        d = torch.full((len(text) + 2 * GUARD,), SENT, dtype=torch.uint8, device="cuda")
        n = eng.bgzf_inflate_device(blob, d.data_ptr() + GUARD, len(text))
        h = d.cpu().numpy()
        assert n == len(text) and h[GUARD:GUARD + n].tobytes() == text, name
        assert (h[:GUARD] == SENT).all() and (h[GUARD + n:] == SENT).all(), name


GZIP_NAMES = ("a-l6-m1", "e-repeat", "f-boundary", "h-reach", "i-false")


@functools.lru_cache(None)
def _gzip_cases():
    out = {}
    for name in GZIP_NAMES:
        blob = GZ.good()[name]
        out[name] = (blob, GZ.expected(blob), {c: host.gzip_inflate_host(blob, c)[1].as_dict() for c in (1024, 0)})
    return out


@pytest.mark.parametrize("name", GZIP_NAMES)
def test_inflate_gzip(eng, name):
    import torch
    blob, text, want = _gzip_cases()[name]
    assert len(text) <= MAX_INPUT
    for chunk in (1024, 0):
        buf = np.full(len(text) + 2 * GUARD, SENT, np.uint8)
        got, st = eng.gzip_inflate(blob, out=buf[GUARD:GUARD + len(text)], chunk=chunk)
        assert len(got) == len(text) and got.tobytes() == text, (name, chunk)
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + len(text):] == SENT).all(), (name, chunk)
        assert st.as_dict() == want[chunk], (name, chunk)
        d = torch.full((len(text) + 2 * GUARD,), SENT, dtype=torch.uint8, device="cuda")
        n, st = eng.gzip_inflate_device(blob, d.data_ptr() + GUARD, len(text), chunk=chunk)
        h = d.cpu().numpy()
        assert n == len(text) and h[GUARD:GUARD + n].tobytes() == text, (name, chunk)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + n:] == SENT).all(), (name, chunk)
        assert st.as_dict() == want[chunk], (name, chunk)
        assert eng.gzip_measure(blob, chunk)[:2] == (len(text), want[chunk]["members"]), (name, chunk)


# ---------------------------------------------------------------- deflate: the host form's bytes; zlib inflates them back
@functools.lru_cache(None)
def _deflate_want():
    return {name: (host.bgzf_deflate_model(text).tobytes(), host.bgzf_deflate_model(text, level=0).tobytes()) for name, text in D.texts().items()}


@pytest.mark.parametrize("name", list(D.texts()))
def test_deflate(eng, name):
    text = D.texts()[name]
    assert len(text) <= MAX_INPUT
    coded, stored = _deflate_want()[name]
    got = t_defl.deflate_guarded(eng, text)
    assert got == coded
    assert (gzip.decompress(got) if text else b"") == text
    got0 = t_defl.deflate_guarded(eng, text, level=0)
    assert got0 == stored and len(got0) == D.bound(len(text))
    assert b"".join(zlib.decompress(got0[m[0]:m[0] + m[2]], 31) for m in BG.directory(got0)) == text


# ---------------------------------------------------------------- BAM: the models and the host forms
def test_bam_to_fastq(eng):
    import torch
    for name, opts in (("a-ubam", dict()), ("a-ubam", dict(piece=256)), ("h-paired", dict(split=1)), ("h-paired", dict(split=1, paired_check=1, piece=1024))):
        c = BM.good()[name]
        assert len(c.blob) <= MAX_INPUT
        model = {k: v for k, v in opts.items() if k not in ("piece", "paired_check")}
        want = BM.expect(c, **model)[0]
        _hw, wst = host.bam_to_fastq_host(c.stream, **opts)
        bufs = [np.full(len(w) + 2 * GUARD, SENT, np.uint8) for w in want]
        got, st = eng.bam_to_fastq(c.blob, outs=[b[GUARD:GUARD + len(w)] for b, w in zip(bufs, want)], **opts)
        assert [g.tobytes() for g in got] == want and st.as_dict() == wst.as_dict(), (name, opts)
        assert all((b[:GUARD] == SENT).all() and (b[GUARD + len(w):] == SENT).all() for b, w in zip(bufs, want))
        d = [torch.full((len(w) + 2 * GUARD,), SENT, dtype=torch.uint8, device="cuda") for w in want]
        lens, reads, st = eng.bam_to_fastq_device(c.blob, [t.data_ptr() + GUARD for t in d], [len(w) for w in want], **opts)
        assert lens == [len(w) for w in want] and reads == list(wst.written) and st.as_dict() == wst.as_dict(), (name, opts)
        for t, w in zip(d, want):
            h = t.cpu().numpy()
            assert h[GUARD:GUARD + len(w)].tobytes() == w and (h[:GUARD] == SENT).all() and (h[GUARD + len(w):] == SENT).all(), (name, opts)


_ROT = bytes.maketrans(b"ACGTNacgtn", b"CGTAACGTAA")


def _all_changed(texts):
    """texts whose every base is another letter of ACGT and whose every quality is another character: every read with a base changes"""
    out, reads = [], 0
    for t in texts:
        if t is None:
            out.append(None)
            continue
        ls = t.split(b"\n")[:-1]
        for i in range(0, len(ls), 4):
            ls[i + 1] = ls[i + 1].translate(_ROT)
            ls[i + 3] = bytes(0x36 if ch == 0x35 else 0x35 for ch in ls[i + 3])
            reads += 1 if ls[i + 3] else 0
        out.append(_lines(ls))
    return out, reads


def test_bam_patch(eng):
    """every read changed: the model's patched stream (the host form gives the statistics), and the compressed form"""
    for name, opts in (("a-ubam", dict()), ("h-paired", dict(split=1)), ("p-straddle", dict(piece=256))):
        c = BP.cases()[name]
        model = {k: v for k, v in opts.items() if k != "piece"}
        texts, reads = _all_changed(BP.identity_texts(c, **model))
        want, mst = BP.patched(c, texts, **opts)
        hw, wst = host.bam_patch_host(c.stream, texts, **opts)
        assert hw.tobytes() == bytes(want) and wst.as_dict() == mst and wst.reads_changed == reads > 64, (name, wst, reads)
        got, st = t_patch.patch_device(eng, c.blob, texts, len(c.stream), **opts)
        assert got == bytes(want) and st.as_dict() == wst.as_dict(), (name, opts)
        bound = host.bgzf_deflate_bound(len(got))
        buf = np.full(bound + 2 * GUARD, SENT, np.uint8)
        z, st = eng.bam_patch(c.blob, texts, out=buf[GUARD:GUARD + bound], **opts)
        assert z.tobytes() == host.bgzf_deflate_model(got, 1).tobytes() and gzip.decompress(z.tobytes()) == got and st.as_dict() == wst.as_dict()
        assert (buf[:GUARD] == SENT).all() and (buf[GUARD + len(z):] == SENT).all()


@pytest.mark.parametrize("name", ("edges", "lanes-rg", "pairs+0-rg", "many"))
def test_fastq_to_bam(eng, name):
    texts, opts = UB.cases()[name]
    want = UB.expect(name)[0]
    _hw, wst = host.fastq_to_bam_host(texts, **opts)
    assert _hw.tobytes() == bytes(want)
    for align in (0, 1):
        got, st = t_ubam.to_bam_device(eng, texts, len(want), align=align, **opts)
        assert got == bytes(want) and st.as_dict() == wst.as_dict(), (name, align)
    bound = host.bgzf_deflate_bound(len(want))
    buf = np.full(bound + 2 * GUARD, SENT, np.uint8)
    z, st = eng.fastq_to_bam(texts, out=buf[GUARD:GUARD + bound], **opts)
    assert z.tobytes() == host.bgzf_deflate_model(bytes(want), 1).tobytes() and gzip.decompress(z.tobytes()) == bytes(want)
    assert st.as_dict() == wst.as_dict()
    assert (buf[:GUARD] == SENT).all() and (buf[GUARD + len(z):] == SENT).all()


# ---------------------------------------------------------------- refusals: the same message, the same first offender, the
# output untouched, the next good call right.  These inputs have passed the host programs under sanitizers; none is meant to fault.
def _refused(call, code=E_ARG):
    with pytest.raises(api.BfqError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_refusal_bgzf(eng):
    """a distance before the member's first byte, found by the kernel; of two damaged members the lower one is named"""
    bad, good, bare = BG.refusals()
    blob, reason, member, off = bad["dist-far"]
    buf = np.full(1 << 16, SENT, np.uint8)
    msg = _refused(lambda: eng.bgzf_inflate(blob, out=buf))
    assert msg.endswith("damaged BGZF input: member %d at byte %d: %s" % (member, off, BG.REASON_TEXT[reason])) and (buf == SENT).all()
    two = good + bare["crc-only"] + good + bare["dist-far"] + BG.EOF
    assert "member 1 at byte %d: %s" % (len(good), BG.REASON_TEXT[bad["crc-only"][1]]) in _refused(lambda: eng.bgzf_inflate(two, out=buf))
    assert (buf == SENT).all() and eng.bgzf_inflate(good + BG.EOF).tobytes() == BG.expected(good)


def test_refusal_gzip(eng):
    """the far distance in a later piece of the second member"""
    import torch
    blob, reason, member, off = GZ.refusals()["dist-far-later-piece-member1"]
    buf = np.full(1 << 16, SENT, np.uint8)
    for chunk in (1024, 0):
        d = torch.full(((1 << 16) + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        assert _refused(lambda: eng.gzip_inflate(blob, out=buf, chunk=chunk)).endswith(GZ.message(member, off, reason))
        assert _refused(lambda: eng.gzip_inflate_device(blob, d.data_ptr(), 1 << 16, chunk=chunk)).endswith(GZ.message(member, off, reason))
        # (the device form decodes in place: "the text of a refused call is undefined", include/bfqzip_hip.h -- but it ends at cap)
        assert (buf == SENT).all() and bool((d[1 << 16:] == SENT).all())
    g, gt, _gs = _gzip_cases()["h-reach"]
    assert eng.gzip_inflate(g, chunk=1024)[0].tobytes() == gt


def test_refusal_bam(eng):
    """a record whose fields do not fit its block"""
    goodc = BM.good()["a-ubam"]
    blob, _stream, code, msg = BM.refusals()["rec-layout"]
    for piece in (256, 0):
        outs = [np.full(1 << 20, SENT, np.uint8), np.full(16, SENT, np.uint8), np.full(16, SENT, np.uint8)]
        assert msg in _refused(lambda: eng.bam_to_fastq(blob, outs=outs, piece=piece), code)
        assert all((o == SENT).all() for o in outs)
    assert [t.tobytes() for t in eng.bam_to_fastq(goodc.blob, piece=1024)[0]] == BM.expect(goodc)[0]


def test_refusal_bam_patch(eng):
    """of three reads of the wrong length the lowest is named (patch_device asserts the output untouched)"""
    c, texts, opts, msg = BP.refusals()["length-lowest-of-three"]
    for piece in (256, 0):
        assert _refused(lambda: t_patch.patch_device(eng, c.blob, texts, len(c.stream) + 4096, piece=piece, **opts)).endswith(msg)
    gc = BP.cases()["p-straddle"]
    gtexts = BP.edited(gc, BP.identity_texts(gc), 7)[0]
    assert t_patch.patch_device(eng, gc.blob, gtexts, len(gc.stream), piece=1024)[0] == bytes(BP.patched(gc, gtexts)[0])


def test_refusal_fastq_to_bam(eng):
    """of the offending reads of three texts the one whose record comes first in the file"""
    texts, opts, code, msg = UB.refusals()["first-of-three"]
    assert _refused(lambda: t_ubam.to_bam_device(eng, texts, 1 << 18, align=3, **opts), code).endswith(msg)
    zbuf = np.full(host.bgzf_deflate_bound(1 << 18), SENT, np.uint8)
    assert _refused(lambda: eng.fastq_to_bam(texts, out=zbuf, **opts), code).endswith(msg) and (zbuf == SENT).all()
    gtx, gopts = UB.cases()["pairs+0-rg"]
    assert t_ubam.to_bam_device(eng, gtx, len(UB.expect("pairs+0-rg")[0]), **gopts)[0] == bytes(UB.expect("pairs+0-rg")[0])


def test_refusal_way_back(eng):
    """streams that do not belong together (the model names the read), a container that is no permutation (the model names
    the entry), texts whose reads differ in length (the model names the lowest read)"""
    raw, want, dna, qs, hdr = _golden("synth_var")
    ql = qs.split(b"\n")[:-1]
    ql[1234] = ql[1234][:-1]; ql[1700] = ql[1700][:-1]
    with pytest.raises(ValueError, match=r"read 1234\b"):
        fastq.restore_text(dna, _lines(ql))
    out = np.full(len(want) + 4096, SENT, np.uint8)
    assert "read 1234" in _refused(lambda: eng.fastq_restore(_z(dna), _z(_lines(ql)), _z(hdr), out=out)) and (out == SENT).all()
    assert eng.fastq_restore(_z(dna), _z(qs), out=out)[0].tobytes() == want
    N = IDX["synth_var"]["reads"]
    p = np.random.default_rng(3).permutation(N).astype(np.uint64)
    badz = t_unre._poke(t_unre._poke(pm.encode(p), 17, int(p[1500])), 700, int(p[1200]))
    with pytest.raises(ValueError) as e:
        pm.decode(badz)
    assert e.value.args[0] == 1200
    out = np.full(len(raw) + 4096, SENT, np.uint8)
    assert "entry 1200" in _refused(lambda: eng.fastq_unreorder([raw], _u8(badz), out=[out])) and (out == SENT).all()
    assert eng.fastq_unreorder([raw], pm.encode(p), out=[out])[0].tobytes() == pm.unreorder([raw], p)[0]
    rec = lambda i, L: b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT" * (L // 4), b"I" * L)
    a, b = b"".join(rec(i, 40) for i in range(100)), b"".join(rec(i, 44 if i in (37, 12) else 40) for i in range(100))
    with pytest.raises(cm.Refused) as e:
        cm.compare([a], [b])
    assert e.value.kind == "length" and e.value.index == 12
    msg = t_cmp.refused(eng, [a], [b])
    assert "read 12" in msg and "37" not in msg
    t_cmp.check(eng, [a], [a], cm.compare([a], [a], max_diffs=4), 4)


def test_refusal_codecs(eng):
    """the containers' lies that the decoding kernels find, not the header's parser"""
    for mod, tag, names in ((nm, "BFQNAME1", ("op_byte_1", "text_past_share")), (qm, "BFQQUAL1", ("zeroed_segment", "lens_that_move_a_value"))):
        goodraw, cases = mod.refusal_cases()
        for name in names:
            assert tag in _refused(lambda: eng.stream_decompress(_u8(cases[name]))), name
            assert eng.stream_decompress(_u8(mod.container(goodraw))).tobytes() == goodraw, name


# ---------------------------------------------------------------- the switch itself
def test_switch_is_live():
    """Without this the module could pass with the fill gone: on a fresh engine under BFQ_POISON=0xC3 the whole workspace reads
    0xC3 after a reservation, a call leaves its own bytes below its high-water mark, and the next reservation wipes them."""
    raw = _golden("example")[0]
    with poisoned(0xC3):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 20)
            n = e.workspace_bytes()
            assert n >= 1 << 20
            assert (e.workspace_read(0, n) == 0xC3).all()
            assert len(e.workspace_read(n - 1, 100)) == 1 and len(e.workspace_read(n, 1)) == 0      # cut at the workspace's end
            e.set_params(m=5)
            out, _st = e.fastq_run(raw)
            assert out == _golden("example")[1]
            n = e.workspace_bytes()
            assert (e.workspace_read(0, n) != 0xC3).any()
            e.stream_reserve(1 << 20)
            assert e.workspace_bytes() == n and (e.workspace_read(0, n) == 0xC3).all()
        finally:
            e.close()
    with poisoned(0xC3):
        pass
    assert os.environ.get("BFQ_POISON") is None or os.environ["BFQ_POISON"] != "0xC3"
