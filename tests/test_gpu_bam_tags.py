"""GPU tests of the aux tags in FASTQ header lines, both ways (the TAGS variants of k_bam.hip and k_ubam.hip): the device
gives the host forms' bytes, statistics and tag counts -- which tests/test_bam_tags_host.py holds against the model
(tests/bam_tags_model.py) -- on the model's cases, at piece sizes of 64, 256 and 65 536 bytes so that tagged records
straddle pieces and the chain repairs some; every refusal names the model's record and leaves the engine usable; the
identity BAM -> text -> BAM, the patch, the name codec, the file forms, the tool and the driver; one case of each way on a
poisoned workspace in a process of its own; and plain options still give the untagged bytes.  Every refusal input has
passed the host program under sanitizers first (test_bam_tags_program_under_sanitizers): they test refusal, none is meant
to fault."""
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import bam_model as M
from tests import bam_tags_model as T
from tests import ubam_model as U
from tests.test_bam_tags_host import split_opts, tags_of
from tests.test_gpu_ubam import to_bam_device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
GUARD = 4096
host = api.HostText


def texts_of(arrs):
    return [a.tobytes() for a in arrs]


def way_in_case():
    return M.Case(T.way_in_recs())


@pytest.mark.parametrize("opts", T.WAY_IN_OPTS, ids=[str(i) for i in range(len(T.WAY_IN_OPTS))])
def test_way_in_engine_equals_the_host_form(engine, opts):
    import torch
    c = way_in_case()
    call, model = split_opts(opts)
    for piece in T.PIECES:
        want, wst = host.bam_to_fastq_host(c.stream, piece=piece, **call)
        got, st = engine.bam_to_fastq(c.blob, piece=piece, **call)
        assert texts_of(got) == texts_of(want), (opts, piece)
        assert st.as_dict() == wst.as_dict() and st.tags.as_dict() == wst.tags.as_dict(), (opts, piece)
        lens, reads, mst = engine.bam_measure(c.stream, piece=piece, **call)             # the inflated stream itself
        assert lens == [len(w) for w in want] and mst.tags.as_dict() == wst.tags.as_dict(), (opts, piece)
        d = [torch.full((len(w) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for w in want]
        lens, reads, st = engine.bam_to_fastq_device(c.blob, [t.data_ptr() + GUARD for t in d], [len(w) for w in want], piece=piece, **call)
        assert lens == [len(w) for w in want] and st.tags.as_dict() == wst.tags.as_dict(), (opts, piece)
        for t, w in zip(d, want):
            h = t.cpu().numpy()
            assert h[GUARD:GUARD + len(w)].tobytes() == w.tobytes() and (h[:GUARD] == 0xA5).all() and (h[GUARD + len(w):] == 0xA5).all(), (opts, piece)
    assert texts_of(want) == T.expected(T.way_in_recs(), opts["tags"], **model)[0] and wst.tags.as_dict() == T.expected(T.way_in_recs(), opts["tags"], **model)[2]


@pytest.mark.parametrize("name", T.REPAIRED)
def test_way_in_on_a_repaired_chain(engine, name):
    """a walker that starts inside a tag area (a B array that holds well-formed records at a piece boundary): the chain walks
    the piece again, and texts and tag counts are the host form's"""
    c = M.good()[name]
    repaired = 0
    for piece in T.PIECES:
        want, wst = host.bam_to_fastq_host(c.stream, piece=piece, tags="*")
        got, st = engine.bam_to_fastq(c.blob, piece=piece, tags="*")
        assert texts_of(got) == texts_of(want) and st.as_dict() == wst.as_dict() and st.tags.as_dict() == wst.tags.as_dict(), (name, piece)
        repaired += st.repaired
    assert repaired == 2


def test_way_in_refusals_name_the_models_record(engine):
    good = way_in_case()
    good_text = T.expected(T.way_in_recs(), "*")[0]
    cases = dict((k, (v, 0)) for k, v in T.bad_tag_recs().items())
    cases["strict"] = (T.strict_recs(), 1)
    for name, (recs, strict) in cases.items():
        c = M.Case(recs, raw=(name != "z-without-nul"))
        with pytest.raises(T.Refused) as w:
            T.expected(recs, "*", strict=strict)
        for piece in T.PIECES:
            outs = [np.full(1 << 17, 0xA5, np.uint8) for _ in range(3)]
            with pytest.raises(api.BfqError) as e:
                engine.bam_to_fastq(c.blob, outs=outs, piece=piece, tags="*", strict_tags=strict)
            assert e.value.code == w.value.code and str(e.value).endswith(w.value.msg), (name, piece, str(e.value), w.value.msg)
            assert all((o == 0xA5).all() for o in outs), (name, piece)
        with pytest.raises(api.BfqError) as e:
            engine.bam_measure(c.blob, tags="*", strict_tags=strict)
        assert str(e.value).endswith(w.value.msg), name
        assert texts_of(engine.bam_to_fastq(c.blob)[0]) == M.expected(recs)[0], name                  # with tags off nothing new is checked
        assert texts_of(engine.bam_to_fastq(good.blob, piece=256, tags="*")[0]) == good_text, name      # and the engine stays usable
    for bad in (dict(tags=["B-"]), dict(tags=[b"\0\0"])):
        with pytest.raises(api.BfqError) as e:
            engine.bam_to_fastq(good.blob, **bad)
        assert e.value.code == -1 and "tags" in str(e.value)
        with pytest.raises(api.BfqError) as e:
            engine.fastq_to_bam_measure([b"@a\tBC:Z:x\nA\n+\nI\n"], **bad)
        assert e.value.code == -1 and "tags" in str(e.value)


@pytest.mark.parametrize("name", T.WAY_OUT_NAMES)
def test_way_out_engine_equals_the_host_form(engine, name):
    texts, opts = T.way_out_cases()[name]
    want, wst = host.fastq_to_bam_host(texts, **opts)
    for align in (0, 1):
        got, st = to_bam_device(engine, texts, len(want), align=align, **opts)
        assert got == want.tobytes(), (name, align)
        assert st.as_dict() == wst.as_dict() and st.tags.as_dict() == wst.tags.as_dict(), (name, align)
    raw, n_reads, mst = engine.fastq_to_bam_measure(texts, **opts)
    assert raw == len(want) and mst.tags.as_dict() == wst.tags.as_dict() and mst.comments_dropped == wst.comments_dropped, name
    assert want.tobytes() == T.expect_out(name)[0] and wst.tags.as_dict() == T.expect_out(name)[2]
    plain = {k: v for k, v in opts.items() if k != "tags"}          # plain options: the untagged model's bytes
    got, st = to_bam_device(engine, texts, len(want), **plain)
    assert got == U.convert(texts, **plain)[0] and st.tags is None, name


@pytest.mark.parametrize("paired", (0, 1))
def test_identity_and_patch(engine, paired):
    """BAM -> text (every tag) -> BAM (tags on, the original header's text) gives the inflated stream byte for byte; the
    tagged texts go back through the patch with the names compared; the tagged header lines through the name codec"""
    c = M.Case(T.identity_recs(paired), text=T.IDENTITY_HEADER)
    t, st = engine.bam_to_fastq(c.blob, tags="*", split=1, paired_check=paired)
    texts = [None, t[1].tobytes(), t[2].tobytes()] if paired else [t[0].tobytes()]
    z, st2 = engine.fastq_to_bam(texts, tags="*", header_text=T.IDENTITY_HEADER, paired_check=paired)
    assert engine.bgzf_inflate(z).tobytes() == c.stream
    assert st.tags.tags_dropped == 0 and st2.tags.fields_dropped == 0 and st.tags.tags_written == st2.tags.tags_written > 1000
    back, _ = engine.bam_to_fastq(z, tags="*", split=1)              # text -> BAM -> text
    assert texts_of(back) == texts_of(t)
    p, pst = engine.bam_patch(c.blob, texts, split=1, check_names=1, tags="*")
    assert engine.bgzf_inflate(p).tobytes() == c.stream and pst.reads_changed == 0
    lines = b"".join(l + b"\n" for x in texts if x is not None for l in x.split(b"\n")[0:-1:4])
    assert b"\tBC:Z:" in lines
    assert engine.stream_decompress(engine.names_compress(lines, always=True)).tobytes() == lines


def test_files_and_tool(engine, tmp_path):
    P = lambda n: str(tmp_path / n)
    c = M.Case(T.identity_recs(0), text=T.IDENTITY_HEADER)
    with open(P("in.bam"), "wb") as f:
        f.write(c.blob)
    with open(P("h.sam"), "wb") as f:
        f.write(T.IDENTITY_HEADER)
    want, wst = host.bam_to_fastq_host(c.stream, tags="*")
    lens, reads, st = engine.bam_to_fastq_files(P("in.bam"), (P("lib.fq"), None, None), tags="*")
    assert open(P("lib.fq"), "rb").read() == want[0].tobytes() and st.tags.as_dict() == wst.tags.as_dict()
    n, st = engine.fastq_to_bam_files((P("lib.fq"),), P("lib.bam"), tags="*", header_text=T.IDENTITY_HEADER)
    assert gzip.decompress(open(P("lib.bam"), "rb").read()) == c.stream and st.tags.tags_written == wst.tags.tags_written
    tool = os.path.join(DROP, "bfq_bam")
    run = lambda args: subprocess.run([tool] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = run(["-i", P("in.bam"), "-o", P("tool.fq"), "-a", "*", "-S", "-V"])
    assert r.returncode == 0 and open(P("tool.fq"), "rb").read() == want[0].tobytes(), r.stderr
    assert b"tags: %d written, 0 dropped, %d bytes of text" % (wst.tags.tags_written, wst.tags.tag_bytes) in r.stderr
    r = run(["-w", P("tool.bam"), "-o", P("tool.fq"), "-a", "*", "-T", P("h.sam")])
    assert r.returncode == 0 and gzip.decompress(open(P("tool.bam"), "rb").read()) == c.stream, r.stderr
    r = run(["-i", P("in.bam"), "-o", P("list.fq"), "-a", "BC,XN"])
    assert r.returncode == 0 and open(P("list.fq"), "rb").read() == host.bam_to_fastq_host(c.stream, tags="BC,XN")[0][0].tobytes()
    r = run(["-i", P("in.bam"), "-o", P("plain.fq")])                 # without -a: what the tool wrote before
    assert r.returncode == 0 and open(P("plain.fq"), "rb").read() == M.expected(c.recs)[0][0]
    bad = M.Case(T.strict_recs())
    with open(P("bad.bam"), "wb") as f:
        f.write(bad.blob)
    r = run(["-i", P("bad.bam"), "-o", P("bad.fq"), "-a", "*", "-S"])
    assert r.returncode == 1 and b"tag XF of type f cannot be carried" in r.stderr and os.path.getsize(P("bad.fq")) == 0
    for args in (["-i", P("in.bam"), "-o", P("x.fq"), "-a", "BCD"], ["-i", P("in.bam"), "-o", P("x.fq"), "-S"], ["-w", P("x.bam"), "-o", P("tool.fq"), "-a", "*", "-S"]):
        assert run(args).returncode == 1, args


def test_restore_and_driver(engine, tmp_path):
    """bfq_restore -b -a on the containers of the tagged text; parallel.py --bam --bam-tags -H --ubam-out: the tags of the
    input's records are those of the output's"""
    P = lambda n: str(tmp_path / n)
    c = M.Case(T.identity_recs(0), text=T.IDENTITY_HEADER)
    text = host.bam_to_fastq_host(c.stream, tags="*")[0][0].tobytes()
    job = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=True)
    for k in ("dna", "qs", "hdr"):
        with open(P("a." + k), "wb") as f:
            f.write(getattr(job, k).tobytes())
    r = subprocess.run([os.path.join(DROP, "bfq_restore"), "-d", P("a.dna"), "-q", P("a.qs"), "-H", P("a.hdr"), "-b", "-a", "*", "-o", P("a.bam")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    assert tags_of(gzip.decompress(open(P("a.bam"), "rb").read())) == [x.aux for x in c.recs]
    n, reads = engine.fastq_restore_files(P("a.dna"), P("a.qs"), P("a.hdr"), P("lib.bam"), ubam=True, tags="BC")
    assert [a for a in tags_of(gzip.decompress(open(P("lib.bam"), "rb").read())) if a] == [M.aux_z(b"BC", T.parse_tags(x.aux)[2][2]) for x in c.recs if x.aux]
    os.mkdir(P("o"))
    with open(P("in.bam"), "wb") as f:
        f.write(c.blob)
    assert parallel.main([P("in.bam"), "-o", P("o/OUT"), "-t", "2", "-0", "-H", "--bam", "--bam-tags", "*", "--ubam-out", P("o/u.bam")]) == 0
    out = gzip.decompress(open(P("o/u.bam"), "rb").read())
    assert tags_of(out) == [x.aux for x in c.recs] and out.startswith(M.header(U.DEFAULT_HEADER))


CHILD = r"""
import sys
sys.path.insert(0, %r)
from bfqzip_amd import api
from tests import bam_model as M, bam_tags_model as T
from tests.test_gpu_ubam import to_bam_device
e = api.Engine(0)
e.stream_reserve(1 << 16)
assert (e.workspace_read(0, 1 << 16) == 0x41).all()
host = api.HostText
if sys.argv[1] == "in":
    c = M.Case(T.way_in_recs())
    for piece in (256, 65536):
        want, wst = host.bam_to_fastq_host(c.stream, piece=piece, tags="*", split=1)
        got, st = e.bam_to_fastq(c.blob, piece=piece, tags="*", split=1)
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want] and st.tags.as_dict() == wst.tags.as_dict()
else:
    texts, opts = T.way_out_cases()["pairs+0"]
    want, wst = host.fastq_to_bam_host(texts, **opts)
    got, st = to_bam_device(e, texts, len(want), align=1, **opts)
    assert got == want.tobytes() and st.as_dict() == wst.as_dict() and st.tags.as_dict() == wst.tags.as_dict()
e.close()
print("poisoned ok")
"""


@pytest.mark.parametrize("way", ("in", "out"))
def test_on_a_poisoned_workspace(way):
    """a fresh process whose workspace and private allocations hold 0x41 before every call: the host form's bytes"""
    env = dict(os.environ, BFQ_POISON="0x41")
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, way], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"poisoned ok" in r.stdout, r.stdout.decode()[-3000:]
