"""GPU tests of the unaligned BAM output (bfq_fastq_to_bam*, k_ubam.hip): the stream and the statistics equal the host
form's -- which tests/test_ubam_host.py holds against the model (tests/ubam_model.py) -- over the model's cases, into guarded
buffers, with the texts at aligned and odd addresses; the four forms agree; the round trips through the BAM input; every
refusal gives the model's message, writes nothing and leaves the engine usable; the restore to BAM, the tool and the
multi-GPU driver.  Every refusal input has passed the host program under sanitizers first
(test_ubam_program_under_sanitizers): they test refusal, none is meant to fault."""
import gzip
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import bam_model as M
from tests import bgzf_model as B
from tests import ubam_model as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
GUARD = 4096
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
host = api.HostText


def to_bam_device(engine, texts, raw_len, align=0, **opts):
    """the device form: texts in torch buffers (at `align` bytes past an aligned address), the stream into a guarded one"""
    import torch
    texts = list(texts) + [None] * (3 - len(texts))
    d = [None if t is None else torch.from_numpy(np.frombuffer(b"\0" * (16 + align) + t, np.uint8).copy()).cuda() for t in texts]
    out = torch.full((raw_len + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        n, st = engine.fastq_to_bam_device([None if t is None else t.data_ptr() + 16 + align for t in d], [0 if t is None else len(t) for t in texts],
                                           out.data_ptr() + GUARD, raw_len, **opts)
    except api.BfqError:
        assert bool((out == 0xA5).all()), "a refusal wrote into the output buffer"
        raise
    h = out.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
    return h[GUARD:GUARD + n].tobytes(), st


@pytest.mark.parametrize("name", U.NAMES)
def test_engine_equals_the_host_form(engine, name):
    texts, opts = U.cases()[name]
    want, wst = host.fastq_to_bam_host(texts, **opts)
    for align in (0, 1, 7, 8):
        got, st = to_bam_device(engine, texts, len(want), align=align, **opts)
        assert got == want.tobytes(), (name, align)
        assert st.as_dict() == wst.as_dict(), (name, align)
    raw, n_reads, mst = engine.fastq_to_bam_measure(texts, **opts)
    assert raw == len(want) and n_reads == list(wst.written) and mst.as_dict() == dict(wst.as_dict(), unknown_bases=0), name


@pytest.mark.parametrize("name", ("empty", "edges", "edges-crlf", "lanes-rg", "pairs+0-rg", "pairs-header", "unnamed", "many"))
def test_forms_agree(engine, tmp_path, name):
    texts, opts = U.cases()[name]
    want, wst = host.fastq_to_bam_host(texts, **opts)
    want = want.tobytes()
    dev, st = to_bam_device(engine, texts, len(want), **opts)
    assert dev == want and st.as_dict() == wst.as_dict(), name
    for level in (1, 0):
        model = host.bgzf_deflate_model(want, level).tobytes()
        bound = host.bgzf_deflate_bound(len(want))
        buf = np.full(bound + 2 * GUARD, 0xA5, np.uint8)           # host buffers, with guard bytes behind and in front
        z, st = engine.fastq_to_bam(texts, out=buf[GUARD:GUARD + bound], level=level, **opts)
        assert z.tobytes() == model and st.as_dict() == wst.as_dict(), (name, level)
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + len(z):] == 0xA5).all()
        tp = []
        for k, t in enumerate(texts):
            tp.append(None if t is None else str(tmp_path / ("t%d.fq" % k)))
            if t is not None:
                with open(tp[-1], "wb") as f:
                    f.write(t)
        dst = str(tmp_path / "out.bam")
        n, st = engine.fastq_to_bam_files(tp, dst, level=level, **opts)
        blob = open(dst, "rb").read()
        assert blob == model and n == len(model) and st.as_dict() == wst.as_dict(), (name, level)
        assert gzip.decompress(blob) == want and blob.endswith(EOF_MEMBER) and len(EOF_MEMBER) == 28
        assert st.members == len(B.directory(blob)), (name, level)
    z, _ = engine.fastq_to_bam(texts, **opts)                       # sized by the call
    assert z.tobytes() == host.bgzf_deflate_model(want, 1).tobytes()
    if name == "many":
        assert wst.members >= 15


def test_round_trip_text_to_bam_to_text(engine):
    """bam_to_fastq(fastq_to_bam(text)) gives the normalised text back: the first word of the name, upper-case bases, a bare '+'"""
    for g in ("example.fastq", "synth_var.fastq"):
        text = B.golden_text(g)
        z, st = engine.fastq_to_bam([text])
        back = engine.bam_to_fastq(z)[0][0].tobytes()
        assert back == U.normalised(text) and st.records == text.count(b"\n") // 4, g
    texts, opts = U.cases()["pairs+0"]
    z, st = engine.fastq_to_bam(texts, rg_id="grp1", paired_check=1)
    back = engine.bam_to_fastq(z, split=1, paired_check=1)[0]
    for k in range(3):                                             # both mates' texts come back with their suffixes
        assert back[k].tobytes() == U.normalised(texts[k], k), k
    assert back[1].tobytes().split(b"\n")[0].endswith(b"/1") and back[2].tobytes().split(b"\n")[0].endswith(b"/2")
    one = engine.bam_to_fastq(z)[0][0].tobytes().split(b"\n")       # unsplit: the file's order, interleaved, text 0 behind
    assert one[0].endswith(b"/1") and one[4].endswith(b"/2") and one[0][:-2] == one[4][:-2] and one[4 * 600].startswith(b"@s0")


def test_round_trip_bam_to_text_to_bam(engine):
    """fastq_to_bam of the texts bam_to_fastq wrote from bam_model's a-ubam case: that case's records carry tags (RG, XB), so the
    result equals them in every field but the tags -- names, flags of text 0, SEQ and QUAL as the texts state them --; a file
    without tags, forward records and qualities <= 93 comes back byte for byte"""
    c = M.good()["a-ubam"]
    recs = [r for r in c.recs if not r.flag & 0x900]
    text = engine.bam_to_fastq(c.blob)[0][0].tobytes()
    z, st = engine.fastq_to_bam([text], header_text=b"")
    sfx = lambda r: (b"/1", b"/2")[M.mate(r.flag) - 1] if M.mate(r.flag) else b""
    fwd = lambda r: (r.seq, r.qual) if not r.flag & 16 else (bytes(M.COMP[M.SEQ.index(ch)] for ch in reversed(r.seq)), r.qual[::-1])
    want = M.header(b"") + b"".join(M.encode(M.rec(r.name + sfx(r), 4, *fwd(r))) for r in recs)
    assert engine.bgzf_inflate(z).tobytes() == want and st.records == len(recs) == 2874
    plain = M.Case([r._replace(aux=b"") for r in M.paired(200)], text=U.DEFAULT_HEADER)
    t = engine.bam_to_fastq(plain.blob, split=1)[0]
    z, st = engine.fastq_to_bam([None, t[1].tobytes(), t[2].tobytes()], paired_check=1)
    assert engine.bgzf_inflate(z).tobytes() == plain.stream and list(st.written) == [0, 200, 200]


def test_capacity_one_byte_short(engine):
    import torch
    texts, opts = U.cases()["pairs+0"]
    want = U.expect("pairs+0")[0]
    bound = host.bgzf_deflate_bound(len(want))
    buf = np.full(bound - 1 + GUARD, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.fastq_to_bam(texts, out=buf[:bound - 1], **opts)
    assert e.value.code == -1 and e.value.needed == bound and (buf == 0xA5).all()
    d = torch.full((len(want) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    dt = [torch.from_numpy(np.frombuffer(t, np.uint8).copy()).cuda() for t in texts]
    with pytest.raises(api.BfqError) as e:
        engine.fastq_to_bam_device([t.data_ptr() for t in dt], [len(t) for t in texts], d.data_ptr(), len(want) - 1, **opts)
    assert e.value.code == -1 and e.value.needed == len(want) and bool((d == 0xA5).all())
    assert to_bam_device(engine, texts, len(want), **opts)[0] == want


def test_refusals(engine, tmp_path):
    good_texts, good_opts = U.cases()["pairs+0-rg"]
    good_want = U.expect("pairs+0-rg")[0]
    for name, (texts, opts, code, msg) in U.refusals().items():
        buf = np.full(host.bgzf_deflate_bound(1 << 18), 0xA5, np.uint8)
        with pytest.raises(api.BfqError) as e:
            engine.fastq_to_bam(texts, out=buf, **opts)
        assert e.value.code == code and str(e.value).endswith(msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all(), name
        with pytest.raises(api.BfqError) as e:
            to_bam_device(engine, texts, 1 << 18, align=3, **opts)
        assert e.value.code == code and str(e.value).endswith(msg), (name, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.fastq_to_bam_measure(texts, **opts)
        assert e.value.code == code and str(e.value).endswith(msg), (name, str(e.value))
        assert to_bam_device(engine, good_texts, len(good_want), **good_opts)[0] == good_want, name
    texts, opts, code, msg = U.refusals()["first-of-three"]        # the file form leaves the output empty
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(tmp_path / ("t%d.fq" % k)))
        open(paths[-1], "wb").write(t)
    with pytest.raises(api.BfqError) as e:
        engine.fastq_to_bam_files(paths, str(tmp_path / "out.bam"), **opts)
    assert str(e.value).endswith(msg) and os.path.getsize(str(tmp_path / "out.bam")) == 0


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_restore_to_bam(engine, tmp_path):
    """bfq_restore -b on the containers of a small run equals fastq_to_bam of bfq_restore's text"""
    restore = os.path.join(DROP, "bfq_restore")
    P = lambda n: str(tmp_path / n)
    text = B.golden_text("example.fastq")

    def containers(tag, t):
        job = engine.fastq_job([t], keep_headers=True, fastq=False, streams=True, hdr=True, compress=True)
        for k in ("dna", "qs", "hdr"):
            with open(P(tag + "." + k), "wb") as f:
                f.write(getattr(job, k).tobytes())
        return ["-d", P(tag + ".dna"), "-q", P(tag + ".qs"), "-H", P(tag + ".hdr")]

    plain = containers("a", text)
    (reordered,), permz = engine.fastq_reorder([text], keep=True)
    with open(P("perm"), "wb") as f:
        f.write(np.asarray(permz, np.uint8).tobytes())
    kept = containers("b", np.asarray(reordered, np.uint8).tobytes()) + ["-P", P("perm")]
    for tag, args in (("a", plain), ("b", kept), ("c", plain[:4])):     # (c: without the headers: every name a number)
        r = _run([restore] + args + ["-o", P(tag + ".fq")])
        assert r.returncode == 0, r.stderr
        restored = open(P(tag + ".fq"), "rb").read()
        r = _run([restore] + args + ["-b", "-o", P(tag + ".bam")])
        assert r.returncode == 0, r.stderr
        blob = open(P(tag + ".bam"), "rb").read()
        want, st = host.fastq_to_bam_host([restored])
        assert gzip.decompress(blob) == want.tobytes() and blob == host.bgzf_deflate_model(want, 1).tobytes(), tag
        assert blob == engine.fastq_to_bam([restored])[0].tobytes() and st.records == 100 and st.named == (100 if tag == "c" else 0), tag
        assert ("%d records, %d bytes of stream -> %d bytes" % (st.records, len(want), len(blob))).encode() in r.stdout
    # the library call on named files, with options
    n, reads = engine.fastq_restore_files(P("a.dna"), P("a.qs"), P("a.hdr"), P("lib.bam"), ubam=True, level=0, rg_id="g")
    want = host.fastq_to_bam_host([open(P("a.fq"), "rb").read()], rg_id="g")[0]
    assert open(P("lib.bam"), "rb").read() == host.bgzf_deflate_model(want, 0).tobytes() and n == os.path.getsize(P("lib.bam")) and reads == 100
    for flags in (["-g", "-b"], ["-z", "-b"]):
        r = _run([restore] + plain + flags + ["-o", P("x.bam")])
        assert r.returncode != 0 and b"-b does not go with" in r.stderr


def test_tool(tmp_path):
    tool = os.path.join(DROP, "bfq_bam")
    path = lambda n: str(tmp_path / n)

    def put(name, data):
        with open(path(name), "wb") as f:
            f.write(data)
        return path(name)

    text = B.golden_text("example.fastq")
    r = _run([tool, "-w", path("one.bam"), "-o", put("one.fq", text)])
    want, st = host.fastq_to_bam_host([text])
    assert r.returncode == 0 and b"100 records: 100 + 0 + 0 written" in r.stdout, (r.stdout, r.stderr)
    assert open(path("one.bam"), "rb").read() == host.bgzf_deflate_model(want, 1).tobytes()
    texts, _ = U.cases()["pairs+0"]
    header = b"@HD\tVN:1.6\tSO:unsorted\n@RG\tID:rg7\tSM:x\n"
    want, st = host.fastq_to_bam_host(texts, rg_id="rg7", header_text=header, paired_check=1)
    r = _run([tool, "-w", path("two.bam"), "-1", put("t1.fq", texts[1]), "-2", put("t2.fq", texts[2]), "-0", put("t0.fq", texts[0]), "-T", put("h.sam", header),
              "-R", "rg7", "-c", "-L", "0"])
    assert r.returncode == 0 and open(path("two.bam"), "rb").read() == host.bgzf_deflate_model(want, 0).tobytes(), (r.stdout, r.stderr)
    want, st = host.fastq_to_bam_host(texts, mate_suffix=0)
    r = _run([tool, "-w", path("kept.bam"), "-1", path("t1.fq"), "-2", path("t2.fq"), "-0", path("t0.fq"), "-n"])
    assert r.returncode == 0 and open(path("kept.bam"), "rb").read() == host.bgzf_deflate_model(want, 1).tobytes(), (r.stdout, r.stderr)
    btexts, _, _, msg = U.refusals()["first-of-three"]
    r = _run([tool, "-w", path("bad.bam"), "-1", put("b1.fq", btexts[1]), "-2", put("b2.fq", btexts[2]), "-0", put("b0.fq", btexts[0])])
    assert r.returncode == 1 and msg.encode() in r.stderr and os.path.getsize(path("bad.bam")) == 0, r.stderr
    for args in (["-w", path("x.bam")], ["-w", path("x.bam"), "-1", path("t1.fq")], ["-w", path("x.bam"), "-i", path("one.bam"), "-o", path("one.fq")],
                 ["-w", path("x.bam"), "-o", path("one.fq"), "-c"], ["-i", path("one.bam"), "-o", path("y.fq"), "-R", "g"]):
        assert _run([tool] + args).returncode == 1, args
    r = _run([tool, "-i", path("one.bam"), "-o", path("plain.fq")])         # the way in takes what -w wrote
    assert r.returncode == 0 and open(path("plain.fq"), "rb").read() == U.normalised(text)


def test_parallel_ubam_out(engine, tmp_path):
    for d in "ab":
        os.mkdir(str(tmp_path / d))
    out = lambda d, n: str(tmp_path / d / n)
    fq = str(tmp_path / "in.fastq")
    with open(fq, "wb") as f:
        f.write(B.golden_text("example.fastq"))
    assert parallel.main([fq, "-o", out("a", "OUT"), "-t", "2", "-0", "-H", "--ubam-out", out("a", "u.bam")]) == 0
    run = open(out("a", "OUT.fastq"), "rb").read()
    blob = open(out("a", "u.bam"), "rb").read()
    assert blob == engine.fastq_to_bam([run])[0].tobytes() and engine.bam_to_fastq(blob)[0][0].tobytes() == U.normalised(run)
    p1, p2 = str(tmp_path / "p_1.fastq"), str(tmp_path / "p_2.fastq")
    t1 = B.golden_text("paired.fastq")
    ls = t1.split(b"\n")[:-1]
    with open(p1, "wb") as f:
        f.write(b"\n".join(ls[:200]) + b"\n")
    with open(p2, "wb") as f:
        f.write(b"\n".join(ls[200:400]) + b"\n")
    assert parallel.main([p1, p2, "-p", "-o", out("b", "OUT"), "-t", "2", "-0", "--ubam-out", out("b", "u.bam")]) == 0
    names = sorted(n for n in os.listdir(str(tmp_path / "b")) if n.endswith((".fastq", ".fq")))
    assert len(names) == 2, os.listdir(str(tmp_path / "b"))
    runs = [open(out("b", n), "rb").read() for n in names]
    blob = open(out("b", "u.bam"), "rb").read()
    assert blob == engine.fastq_to_bam([None, runs[0], runs[1]])[0].tobytes()
    back = engine.bam_to_fastq(blob, split=1, mate_suffix=0)[0]
    assert back[0].tobytes() == b"" and [b.tobytes().split(b"\n")[1::2] for b in back[1:]] == [r.split(b"\n")[1::2] for r in runs]
