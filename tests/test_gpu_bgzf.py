"""GPU tests of the BGZF input (bfq_bgzf_*, k_bgzf.hip): the inflated text equals gzip.decompress over the model's matrix,
extremes and hand-made blocks (tests/bgzf_model.py); every refusal names the member, its offset and the reason, and leaves
the engine usable.  The refusal inputs have passed the host program under sanitizers first (tests/test_bgzf_host.py): they
test refusal, none is meant to fault."""
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import bgzf_model as M, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
E_ARG = -1
GUARD = 4096


def inflate_guarded(engine, blob, text):
    """host-out inflate into a buffer with 0xA5 bands around the exact raw length"""
    buf = np.full(len(text) + 2 * GUARD, 0xA5, np.uint8)
    got = engine.bgzf_inflate(blob, out=buf[GUARD:GUARD + len(text)])
    assert len(got) == len(text) and got.tobytes() == text
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + len(text):] == 0xA5).all()


@pytest.fixture(scope="module")
def matrix():
    return M.matrix()


@pytest.mark.parametrize("writer", list(M.WRITERS))
def test_matrix(engine, matrix, writer):
    names = [n for n in matrix if n.endswith("-" + writer)]
    assert len(names) == 8
    for n in names:
        blob = matrix[n]
        inflate_guarded(engine, blob, M.expected(blob))


def test_extremes_and_crafted(engine):
    for name, blob in {**M.extremes(), **M.crafted()}.items():
        text = M.expected(blob)
        inflate_guarded(engine, blob, text)
        assert engine.bgzf_inflate(blob).tobytes() == text, name
    with pytest.raises(api.BfqError) as e:                         # a buffer below the raw length: refused, nothing written
        buf = np.full(100, 0xA5, np.uint8)
        engine.bgzf_inflate(M.crafted()["len258-dist32768"], out=buf)
    assert e.value.code == E_ARG and (buf == 0xA5).all()


def test_inflate_into_device_memory(engine):
    """bfq_bgzf_inflate_device: the text lands in the caller's device buffer and nowhere beside it (0xA5 bands on the device);
    a capacity below the raw length is refused with the buffer untouched"""
    import torch
    cases = {**M.extremes(), "synth-c700-l9": M.matrix()["synth-c700-l9"], "len258-dist32768": M.crafted()["len258-dist32768"]}
    for name, blob in cases.items():
        text = M.expected(blob)
        d = torch.full((len(text) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        n = engine.bgzf_inflate_device(blob, d.data_ptr() + GUARD, len(text))
        h = d.cpu().numpy()
        assert n == len(text) and h[GUARD:GUARD + n].tobytes() == text, name
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), name
    blob = cases["synth-c700-l9"]
    d = torch.full((1000 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(api.BfqError) as e:
        engine.bgzf_inflate_device(blob, d.data_ptr(), 1000)
    assert e.value.code == E_ARG and bool((d == 0xA5).all())


def test_big(engine):
    blob = M.big()
    assert len(M.directory(blob)) == 307 + 1
    inflate_guarded(engine, blob, M.expected(blob))


def test_refusals(engine):
    bad, good, bare = M.refusals()
    good_text = M.expected(good)
    for name, (blob, reason, member, off) in bad.items():
        with pytest.raises(api.BfqError) as e:
            engine.bgzf_inflate(blob)
        assert e.value.code == E_ARG, name
        if name == "plain-gzip":
            assert "not BGZF" in str(e.value) and "recompress it with bgzip" in str(e.value)
        else:
            assert str(e.value).endswith("damaged BGZF input: member %d at byte %d: %s" % (member, off, M.REASON_TEXT[reason])), (name, str(e.value))
        assert engine.bgzf_inflate(good + M.EOF).tobytes() == good_text, name
    # the lowest failing member wins, whichever way the two are damaged
    for first, second in (("crc-only", "dist-far"), ("dist-far", "crc-only"), ("crc-only", "no-bc"), ("stored-run", "total-small")):
        blob = good + bare[first] + good + bare[second] + M.EOF
        with pytest.raises(api.BfqError) as e:
            engine.bgzf_inflate(blob)
        assert "member 1 at byte %d: %s" % (len(good), M.REASON_TEXT[bad[first][1]]) in str(e.value), (first, second, str(e.value))


# ---------------------------------------------------------------- a BGZF source where FASTQ text is taken
def same_job(a, b):
    for k in ("fastq", "dna", "qs", "hdr"):
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), k
    assert a.stats == b.stats and a.n_reads == b.n_reads and a.total_bases == b.total_bases
    for k in ("part_reads", "part_fastq_off", "part_stream_off", "part_hdr_off"):
        assert getattr(a, k) == getattr(b, k), k


def test_job_from_bgzf(engine):
    engine.set_params(m=5)
    text = M.golden_text("example.fastq")
    kw = dict(keep_headers=True, fastq=True, streams=True, hdr=True)
    want = engine.fastq_job([text], **kw)
    for chunk, level in ((65280, 6), (700, 1), (4096, 0)):           # members cut lines and records anywhere
        same_job(engine.fastq_job([M.bgzf(text, chunk, level)], **kw), want)
    got = engine.fastq_job([M.bgzf(text, 5000)])
    assert got.fastq.tobytes() == M.golden_text("example.M2B0.fq")
    assert engine.fastq_run(M.bgzf(text, 5000))[0] == M.golden_text("example.M2B0.fq")
    # two parts, part 0 BGZF and part 1 plain; then the other way round
    other = M.golden_text("paired.fastq")
    want2 = engine.fastq_job([text, other], **kw)
    same_job(engine.fastq_job([M.bgzf(text, 3000), other], **kw), want2)
    same_job(engine.fastq_job([text, M.bgzf(other, 3000)], **kw), want2)
    # a BGZF part whose text lacks its final newline: known only once it is inflated
    cut = text[:-1]
    assert cut[-1:] != b"\n"
    same_job(engine.fastq_job([M.bgzf(cut, 3000), other], **kw), engine.fastq_job([cut, other], **kw))
    same_job(engine.fastq_job([M.bgzf(cut, 3000)], **kw), engine.fastq_job([cut], **kw))
    z = engine.fastq_job([M.bgzf(text, 3000)], fastq=False, streams=True, hdr=True, compress=True)
    zw = engine.fastq_job([text], fastq=False, streams=True, hdr=True, compress=True)
    same_job(z, zw)
    # a damaged part is refused as the inflate refuses it, and the engine goes on
    bad, good, bare = M.refusals()
    with pytest.raises(api.BfqError) as e:
        engine.fastq_job([bad["crc-only"][0]])
    assert e.value.code == E_ARG and "damaged BGZF input: member 1 at byte %d: CRC32 mismatch" % len(good) in str(e.value)
    with pytest.raises(api.BfqError) as e:
        engine.fastq_job([bad["plain-gzip"][0]])
    assert "recompress it with bgzip" in str(e.value)
    same_job(engine.fastq_job([text], **kw), want)


def test_build_ebwt_from_bgzf(engine, tmp_path):
    b, q, r, h, bwt, qs, lcp = util.golden_set("example")
    text = M.golden_text("example.fastq")
    gb, gq, gl = engine.fastq_build_ebwt(M.bgzf(text, 4096, 9))
    assert np.array_equal(gb, bwt) and np.array_equal(gq, qs) and np.array_equal(gl, lcp)
    # the gsufsort executable on a .fastq.gz writes the files it writes for the text
    gz = str(tmp_path / "example.fastq.gz")
    with open(gz, "wb") as f:
        f.write(M.bgzf(text, 65280, 6))
    out = str(tmp_path / "OUT")
    r = subprocess.run([os.path.join(DROP, "external", "gsufsort", "gsufsort"), gz, "--bwt", "--qs", "-o", out], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout
    assert open(out + ".bwt", "rb").read() == M.golden_text("example.bwt") and open(out + ".bwt.qs", "rb").read() == M.golden_text("example.bwt.qs")


def test_compare_and_reorder(engine):
    a, b = M.golden_text("example.fastq"), M.golden_text("example.M2B0.fq")
    want = engine.fastq_compare([a], [b], max_diffs=50)
    cut = len(b"\n".join(a.split(b"\n")[:400])) + 1              # a record boundary: parts are cut there
    for got in (engine.fastq_compare([M.bgzf(a, 700)], [b], max_diffs=50), engine.fastq_compare([a], [M.bgzf(b, 5000, 1)], max_diffs=50),
                engine.fastq_compare([M.bgzf(a[:cut], 700), a[cut:]], [M.bgzf(b, 65280)], max_diffs=50)):
        assert got.as_dict() == want.as_dict() and np.array_equal(got.diffs, want.diffs)
    assert want.n_diffs > 0
    with pytest.raises(api.BfqError) as e:
        engine.fastq_reorder([M.bgzf(a, 5000)])
    assert e.value.code == E_ARG and "inflate first" in str(e.value)
    assert len(engine.fastq_reorder([a])[0][0]) == len(a)           # the engine goes on


def test_tool(tmp_path):
    tool = os.path.join(DROP, "bfq_bgzf")
    text = M.synth_var()
    gz, out = str(tmp_path / "in.fq.gz"), str(tmp_path / "out.fq")
    with open(gz, "wb") as f:
        f.write(M.bgzf(text, 700, 6))
    run = lambda *a: subprocess.run([tool] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = run("-l", gz)
    assert r.returncode == 0 and r.stdout.decode().startswith("274 members, %d bytes compressed, 190990 bytes raw" % os.path.getsize(gz))
    r = run("-d", gz, "-o", out)
    assert r.returncode == 0 and open(out, "rb").read() == text, r.stderr
    r = run("-t", gz)
    assert r.returncode == 0 and b"190990 bytes verified" in r.stdout
    bad, good, _ = M.refusals()
    with open(gz, "wb") as f:
        f.write(bad["dist-far"][0])
    for args in (("-d", gz, "-o", out), ("-t", gz)):
        r = run(*args)
        assert r.returncode == 1
        assert ("damaged BGZF input: member 1 at byte %d: a match distance reaches before the start of the member" % len(good)).encode() in r.stderr
    assert os.path.getsize(out) == 0
    with open(gz, "wb") as f:
        f.write(bad["plain-gzip"][0])
    r = run("-t", gz)
    assert r.returncode == 1 and b"recompress it with bgzip" in r.stderr


def test_parallel_on_gz(tmp_path):
    text = M.golden_text("example.fastq")
    plain, gz = str(tmp_path / "in.fastq"), str(tmp_path / "in.fastq.gz")
    with open(plain, "wb") as f:
        f.write(text)
    with open(gz, "wb") as f:
        f.write(M.bgzf(text, 5000))
    os.mkdir(str(tmp_path / "a")); os.mkdir(str(tmp_path / "b")); os.mkdir(str(tmp_path / "c"))
    assert parallel.main([plain, "-o", str(tmp_path / "a" / "OUT"), "-t", "2", "-0", "--m3"]) == 0
    assert parallel.main([gz, "-o", str(tmp_path / "b" / "OUT"), "-t", "2", "-0", "--m3"]) == 0
    assert parallel.main([gz, "-o", str(tmp_path / "c" / "OUT"), "-t", "2", "-0", "--m3", "--keep-inflated"]) == 0
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and len(names) == 4       # the inflated temporary is gone
    assert sorted(os.listdir(str(tmp_path / "c"))) == sorted(names + ["in.inflated.fastq"])
    assert open(str(tmp_path / "c" / "in.inflated.fastq"), "rb").read() == text
    for n in names:
        want = open(str(tmp_path / "a" / n), "rb").read()
        assert open(str(tmp_path / "b" / n), "rb").read() == want and open(str(tmp_path / "c" / n), "rb").read() == want, n
