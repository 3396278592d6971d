"""GPU tests of the BAM output (bfq_bam_patch*, k_bam_patch.hip): the patched stream and the statistics equal the host
form's -- which tests/test_bam_patch_host.py holds against the model (tests/bam_patch_model.py) -- over the model's cases,
option sets and piece sizes; the four forms agree, into guarded buffers; every refusal gives the model's message, writes
nothing and leaves the engine usable; the identity and the round trip through a real run; the tool and the multi-GPU driver.
Every refusal input has passed the host program under sanitizers first (test_bam_patch_program_under_sanitizers): they
test refusal, none is meant to fault."""
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import bam_model as M
from tests import bam_patch_model as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
GUARD = 4096
host = api.HostText


def edited_texts(case, opts, seed=7):
    return P.edited(case, P.identity_texts(case, **opts), seed, **opts)[0]


def patch_device(engine, blob, texts, raw_len, align=0, **opts):
    """the device form: texts in torch buffers (at `align` bytes past an aligned address), the stream into a guarded one"""
    import torch
    texts = list(texts) + [None] * (3 - len(texts))
    d = [None if t is None else torch.from_numpy(np.frombuffer(b"\0" * (16 + align) + t, np.uint8).copy()).cuda() for t in texts]
    out = torch.full((raw_len + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        n, st = engine.bam_patch_device(blob, [None if t is None else t.data_ptr() + 16 + align for t in d], [0 if t is None else len(t) for t in texts],
                                        out.data_ptr() + GUARD, raw_len, **opts)
    except api.BfqError:
        assert bool((out == 0xA5).all()), "a refusal wrote into the output buffer"
        raise
    h = out.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
    return h[GUARD:GUARD + n].tobytes(), st


@pytest.mark.parametrize("name", P.NAMES)
def test_engine_equals_the_host_form(engine, name):
    c = P.cases()[name]
    for opts in M.OPTION_SETS:
        for texts in (P.identity_texts(c, **opts), edited_texts(c, opts)):
            first = None
            for piece in P.PIECES:
                want, wst = host.bam_patch_host(c.stream, texts, piece=piece, **opts)
                got, st = patch_device(engine, c.blob, texts, len(c.stream), piece=piece, **opts)
                assert got == want.tobytes(), (name, piece, opts)
                assert st.as_dict() == wst.as_dict(), (name, piece, opts)
                first = first or got
                assert got == first, (name, piece, opts)


@pytest.mark.parametrize("name", ("b-edges", "p-lanes", "p-straddle", "a-ubam"))
def test_identity_and_round_trip(engine, name):
    c = P.cases()[name]
    for opts in (dict(), dict(split=1), dict(default_qual=30)):
        got, st = patch_device(engine, c.blob, P.identity_texts(c, **opts), len(c.stream), check_names=1, piece=1024, **opts)
        assert got == c.stream and st.reads_changed == 0 and st.bases_changed == 0 and st.quals_changed == 0, (name, opts, st)
        texts, nb, nq = P.edited(c, P.identity_texts(c, **opts), 11, **opts)
        got, st = patch_device(engine, c.blob, texts, len(c.stream), align=3, **opts)      # (texts at odd addresses: copied before they are indexed)
        assert st.bases_changed == nb and st.quals_changed == nq, (name, opts, st)
        back = engine.bam_to_fastq(got, **opts)[0]
        assert [b.tobytes() for b in back] == texts, (name, opts)


@pytest.mark.parametrize("name", ("b-edges", "p-lanes", "h-paired", "g-empty", "j-raw"))
def test_forms_agree(engine, tmp_path, name):
    c = P.cases()[name]
    for opts in (dict(), dict(split=1, piece=1024)):
        ident = P.identity_texts(c, **opts)
        for texts in (edited_texts(c, opts), [None] + edited_texts(c, opts)[1:], P.variants(ident)["crlf"]):
            want, wst = host.bam_patch_host(c.stream, texts, **opts)
            want = want.tobytes()
            dev, st = patch_device(engine, c.blob, texts, len(c.stream), **opts)
            assert dev == want and st.as_dict() == wst.as_dict(), (name, opts)
            for level in (1, 0):
                model = host.bgzf_deflate_model(dev, level).tobytes()
                # host buffers, with guard bytes behind and in front
                bound = host.bgzf_deflate_bound(len(want))
                buf = np.full(bound + 2 * GUARD, 0xA5, np.uint8)
                z, st = engine.bam_patch(c.blob, texts, level=level, out=buf[GUARD:GUARD + bound], **opts)
                assert z.tobytes() == model and st.as_dict() == wst.as_dict(), (name, opts, level)
                assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + len(z):] == 0xA5).all()
                assert engine.bgzf_inflate(z).tobytes() == dev
                # files
                src, dst = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
                tp = []
                for k, t in enumerate(texts):
                    tp.append(None if t is None else str(tmp_path / ("t%d.fq" % k)))
                    if t is not None:
                        with open(tp[-1], "wb") as f:
                            f.write(t)
                with open(src, "wb") as f:
                    f.write(c.blob)
                n, st = engine.bam_patch_files(src, tp, dst, level=level, **opts)
                assert open(dst, "rb").read() == model and n == len(model) and st.as_dict() == wst.as_dict(), (name, opts, level)
            z, _ = engine.bam_patch(c.blob, texts, **opts)             # sized by the call
            assert z.tobytes() == host.bgzf_deflate_model(dev, 1).tobytes()


@pytest.mark.parametrize("name", ("b-edges", "p-lanes", "p-straddle"))
def test_texts_written_another_way(engine, name):
    """lowercase bases, CRLF, no final LF: the same stream as the plain text; bytes outside the alphabet: N, counted by the
    lanes and summed over the wave -- on forward and 0x10 records, at every piece size, as the host form has it"""
    c = P.cases()[name]
    assert any(r.flag & 0x10 and len(r.seq) > 64 for r in c.recs) and any(not r.flag & 0x10 and len(r.seq) > 64 for r in c.recs)
    texts = edited_texts(c, {})
    plain = host.bam_patch_host(c.stream, texts)[0].tobytes()
    odd, n_odd, odd_back = P.non_alphabet(texts)
    assert n_odd > 64
    for how, other in dict(P.variants(texts), **{"non-alphabet": odd}).items():
        for piece in P.PIECES:
            want, wst = host.bam_patch_host(c.stream, other, piece=piece)
            got, st = patch_device(engine, c.blob, other, len(c.stream), piece=piece)
            assert got == want.tobytes() and st.as_dict() == wst.as_dict(), (name, how, piece)
            if how == "non-alphabet":
                assert st.unknown_bases == n_odd and got != plain, (name, piece, st)
                assert engine.bam_to_fastq(got)[0][0].tobytes() == odd_back[0], (name, piece)
            else:
                assert st.unknown_bases == 0 and got == plain, (name, how, piece)
    z, st = engine.bam_patch(c.blob, P.variants(odd)["lower"], piece=256)     # the compressed form, host texts in: lowercase and unknown at once
    assert st.unknown_bases == n_odd and engine.bam_to_fastq(z)[0][0].tobytes() == odd_back[0]


def test_capacity_one_byte_short(engine):
    import torch
    c = P.cases()["h-paired"]
    texts = edited_texts(c, dict(split=1))
    want = host.bam_patch_host(c.stream, texts, split=1)[0].tobytes()
    bound = host.bgzf_deflate_bound(len(want))
    buf = np.full(bound - 1 + GUARD, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.bam_patch(c.blob, texts, out=buf[:bound - 1], split=1)
    assert e.value.code == -1 and e.value.needed == bound and (buf == 0xA5).all()
    d = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dt = [torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda() for t in texts]
    with pytest.raises(api.BfqError) as e:
        engine.bam_patch_device(c.blob, [t.data_ptr() for t in dt], [len(t) for t in texts], d.data_ptr(), len(want) - 1, split=1)
    assert e.value.code == -1 and e.value.needed == len(want) and bool((d == 0xA5).all())
    for bad in (dict(piece=63), dict(default_qual=94), dict(level=2)):
        with pytest.raises(api.BfqError) as e:
            engine.bam_patch(c.blob, texts, **dict(dict(split=1), **bad))
        assert e.value.code == -1, bad
    assert engine.bgzf_inflate(engine.bam_patch(c.blob, texts, split=1)[0]).tobytes() == want
    assert patch_device(engine, c.blob, texts, len(want), split=1)[0] == want


def test_refusals(engine, tmp_path):
    good = P.cases()["p-straddle"]
    good_texts = edited_texts(good, {})
    good_want = host.bam_patch_host(good.stream, good_texts)[0].tobytes()
    bad = [(n, c.blob, t, o, -1, m) for n, (c, t, o, m) in P.refusals().items()]
    ident = P.identity_texts(P.cases()["h-paired"])
    for n in ("rec-layout", "stream-ends-in-record", "header-l-text", "too-long", "bgzf-damaged"):
        blob, stream, code, msg = M.refusals()[n]
        bad.append((n, blob, [ident[0]], {}, code, msg))
    for name, blob, texts, opts, code, msg in bad:
        raw = len(good.stream) + (1 << 20)
        for piece in (256, 0):
            buf = np.full(host.bgzf_deflate_bound(raw), 0xA5, np.uint8)
            with pytest.raises(api.BfqError) as e:
                engine.bam_patch(blob, texts, out=buf, piece=piece, **opts)
            assert e.value.code == code and (msg in str(e.value) if name == "bgzf-damaged" else str(e.value).endswith(msg)), (name, piece, str(e.value), msg)
            assert (buf == 0xA5).all(), name
        with pytest.raises(api.BfqError) as e:
            patch_device(engine, blob, texts, raw, **opts)
        assert e.value.code == code and msg in str(e.value), (name, str(e.value))
        assert patch_device(engine, good.blob, good_texts, len(good.stream), piece=1024)[0] == good_want, name
    c, texts, opts, msg = P.refusals()["length"]                   # the file form leaves the output empty
    paths = []
    for k, t in enumerate(texts):
        paths.append(None if t is None else str(tmp_path / ("t%d.fq" % k)))
        if t is not None:
            open(paths[-1], "wb").write(t)
    open(str(tmp_path / "in.bam"), "wb").write(c.blob)
    with pytest.raises(api.BfqError) as e:
        engine.bam_patch_files(str(tmp_path / "in.bam"), paths, str(tmp_path / "out.bam"), **opts)
    assert str(e.value).endswith(msg) and os.path.getsize(str(tmp_path / "out.bam")) == 0


def test_end_to_end_through_a_run(engine):
    """a-ubam -> FASTQ -> the smoother without kept headers -> back into the BAM -> FASTQ: the run's sequence and quality lines"""
    c = M.good()["a-ubam"]
    fq = engine.bam_to_fastq(c.blob)[0][0]
    engine.set_params(m=5)
    run, _ = engine.fastq_run(fq.tobytes())
    assert run.split(b"\n")[0] == b"@"
    z, st = engine.bam_patch(c.blob, [run])
    back = engine.bam_to_fastq(z)[0][0].tobytes()
    assert back.split(b"\n")[1::2] == run.split(b"\n")[1::2] and back.split(b"\n")[0::4] == fq.tobytes().split(b"\n")[0::4]
    rep = engine.fastq_compare([run], [back])
    assert rep.bases_changed == 0 and rep.quals_changed == 0 and rep.n_reads == st.patched[0] == 2874
    diff = engine.fastq_compare([fq], [run])
    assert (st.bases_changed, st.quals_changed) == (diff.bases_changed, diff.quals_changed) and st.reads_changed == diff.reads_changed
    stream = engine.bgzf_inflate(z).tobytes()
    m = np.frombuffer(P.mask(c, [run]), np.uint8)
    assert not ((np.frombuffer(stream, np.uint8) != np.frombuffer(c.stream, np.uint8)) & (m == 0)).any()


def test_tool(tmp_path):
    tool = os.path.join(DROP, "bfq_bam")
    run = lambda *a: subprocess.run([tool] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    path = lambda n: str(tmp_path / n)

    def put(name, data):
        with open(path(name), "wb") as f:
            f.write(data)
        return path(name)

    c = P.cases()["h-paired"]
    a = put("a.bam", c.blob)
    one = edited_texts(c, {})
    want = host.bam_patch_host(c.stream, one)[0]
    r = run("-i", a, "-u", path("one.bam"), "-o", put("one.fq", one[0]))
    assert r.returncode == 0 and b"1000 records: 1000 + 0 + 0 patched" in r.stdout, (r.stdout, r.stderr)
    assert open(path("one.bam"), "rb").read() == host.bgzf_deflate_model(want, 1).tobytes()
    two = edited_texts(c, dict(split=1))
    want = host.bam_patch_host(c.stream, two, split=1, check_names=1)[0]
    r = run("-i", a, "-u", path("two.bam"), "-1", put("t1.fq", two[1]), "-2", put("t2.fq", two[2]), "-N", "-L", "0", "-C", "1024")
    assert r.returncode == 0 and open(path("two.bam"), "rb").read() == host.bgzf_deflate_model(want, 0).tobytes(), (r.stdout, r.stderr)
    _, texts, _, msg = P.refusals()["length"]
    r = run("-i", a, "-u", path("bad.bam"), "-1", put("b1.fq", texts[1]), "-2", put("b2.fq", texts[2]))
    assert r.returncode == 1 and msg.encode() in r.stderr and os.path.getsize(path("bad.bam")) == 0, r.stderr
    assert run("-i", a, "-u", path("x.bam")).returncode == 1 and run("-i", a, "-o", path("x.fq"), "-N").returncode == 1
    r = run("-i", a, "-o", path("plain.fq"))                        # without -u: as before
    assert r.returncode == 0 and open(path("plain.fq"), "rb").read() == M.expect(c)[0][0]


def test_parallel_bam_out(engine, tmp_path):
    c = P.cases()["h-paired"]
    bam = str(tmp_path / "in.bam")
    with open(bam, "wb") as f:
        f.write(c.blob)
    for d in "abc":
        os.mkdir(str(tmp_path / d))
    out = lambda d, n: str(tmp_path / d / n)
    # refused before any work is done
    assert parallel.main([bam, "--bam", "--reorder", "2", "-o", out("c", "OUT"), "-t", "2", "-0", "--bam-out", out("c", "o.bam")]) == 1
    assert parallel.main([bam, "-o", out("c", "OUT"), "-t", "2", "-0", "--bam-out", out("c", "o.bam")]) == 1
    fq = str(tmp_path / "plain.fastq")
    with open(fq, "wb") as f:
        f.write(M.expect(c)[0][0])
    assert parallel.main([fq, "--bam", "-o", out("c", "OUT"), "-t", "2", "-0", "--bam-out", out("c", "o.bam")]) == 1      # no BAM file
    assert os.listdir(str(tmp_path / "c")) == []
    # one text
    assert parallel.main([bam, "--bam", "-o", out("a", "OUT"), "-t", "2", "-0", "--bam-out", out("a", "o.bam")]) == 0
    run = open(out("a", "OUT.fastq"), "rb").read()
    back = engine.bam_to_fastq(open(out("a", "o.bam"), "rb").read())[0][0].tobytes()
    assert back.split(b"\n")[1::2] == run.split(b"\n")[1::2] and back.split(b"\n")[0::4] == M.expect(c)[0][0].split(b"\n")[0::4]
    # paired, headers kept: the names are compared
    assert parallel.main([bam, "--bam", "-p", "-H", "-o", out("b", "OUT"), "-t", "2", "-0", "--bam-out", out("b", "o.bam")]) == 0
    names = sorted(n for n in os.listdir(str(tmp_path / "b")) if n.endswith((".fastq", ".fq")))
    assert len(names) == 2, os.listdir(str(tmp_path / "b"))
    runs = [open(out("b", n), "rb").read() for n in names]
    back = engine.bam_to_fastq(open(out("b", "o.bam"), "rb").read(), split=1)[0]
    assert back[0].tobytes() == b"" and [b.tobytes() for b in back[1:]] == runs
