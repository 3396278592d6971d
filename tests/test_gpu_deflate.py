"""GPU tests of the BGZF output (bfq_bgzf_deflate*, k_deflate.hip): over the texts of tests/deflate_cases.py the kernel gives,
byte for byte, what the host form gives (HostText.bgzf_deflate_model, which has passed the sanitizer program of
tests/test_deflate_host.py), whatever the batch; gzip and the library's own inflate read it back; refusals leave the buffer
untouched and the engine usable; the tools round-trip (bfq_bgzf -c / -t / -d, gsufsort on the result, bfq_restore -z)."""
import gzip
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import api
from tests import bgzf_model as M
from tests import deflate_cases as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
E_ARG = -1
GUARD = 4096


@pytest.fixture(scope="module")
def models():
    """name -> the host form's bytes, made once"""
    return {name: api.HostText.bgzf_deflate_model(text).tobytes() for name, text in D.texts().items()}


def deflate_guarded(engine, text, level=1):
    """into a buffer with 0xA5 bands around exactly `bound` bytes"""
    bound = api.HostText.bgzf_deflate_bound(len(text))
    buf = np.full(bound + 2 * GUARD, 0xA5, np.uint8)
    got = engine.bgzf_deflate(text, level=level, out=buf[GUARD:GUARD + bound]).tobytes()
    assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + bound:] == 0xA5).all()
    return got


@pytest.mark.parametrize("name", list(D.texts()))
def test_same_bytes_as_host_form(engine, models, name):
    text = D.texts()[name]
    got = deflate_guarded(engine, text)
    assert got == models[name]
    assert (gzip.decompress(got) if text else b"") == text
    assert engine.bgzf_inflate(got).tobytes() == text
    assert deflate_guarded(engine, text) == got                              # a second call: the same bytes
    stored = deflate_guarded(engine, text, level=0)
    assert stored == api.HostText.bgzf_deflate_model(text, level=0).tobytes() and len(stored) == D.bound(len(text))


CHILD = """
import sys
from bfqzip_amd import api
e = api.Engine(0)
sys.stdout.buffer.write(e.bgzf_deflate(open(sys.argv[1], 'rb').read()).tobytes())
e.close()
"""


def test_batches(engine, tmp_path):
    """the batch seam, the gather offsets and the single EOF member: other batch sizes, each in a fresh process, give the
    default batch's bytes"""
    text = D.repeated(M.golden_text("example.fastq"), 5 * D.PIECE + 17)
    want = engine.bgzf_deflate(text).tobytes()
    assert want == api.HostText.bgzf_deflate_model(text).tobytes() and len(M.directory(want)) == 7 and gzip.decompress(want) == text
    src = str(tmp_path / "text")
    with open(src, "wb") as f:
        f.write(text)
    for batch in (65280, 130560):
        env = dict(os.environ, BFQ_BGZF_BATCH=str(batch), PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", CHILD, src], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, batch


def test_deflate_from_device_memory(engine, models):
    import torch
    for name in ("example-65281", "synth_var", "one-byte"):
        text = D.texts()[name]
        d = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        assert engine.bgzf_deflate_device(d.data_ptr(), len(text)).tobytes() == models[name], name
    assert engine.bgzf_deflate_device(0, 0).tobytes() == M.EOF


def test_files(engine, models, tmp_path):
    src, dst = str(tmp_path / "in.fq"), str(tmp_path / "out.fq.gz")
    with open(src, "wb") as f:
        f.write(D.texts()["example-65281"])
    assert engine.bgzf_deflate_files(src, dst) == len(models["example-65281"])
    assert open(dst, "rb").read() == models["example-65281"]


def test_refusals(engine, models):
    text = D.texts()["example"]
    bound = api.HostText.bgzf_deflate_bound(len(text))
    buf = np.full(bound, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.bgzf_deflate(text, out=buf[:bound - 1])
    assert e.value.code == E_ARG and (buf == 0xA5).all()
    with pytest.raises(api.BfqError) as e:
        engine.bgzf_deflate(text, level=2, out=buf)
    assert e.value.code == E_ARG and (buf == 0xA5).all()
    gz = models["example"]
    big = np.full(api.HostText.bgzf_deflate_bound(len(gz)), 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.bgzf_deflate(gz, out=big)
    assert e.value.code == E_ARG and "already compressed" in str(e.value) and (big == 0xA5).all()
    assert engine.bgzf_deflate(text).tobytes() == gz                         # the engine goes on


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_tool_round_trip(models, tmp_path):
    tool = os.path.join(DROP, "bfq_bgzf")
    P = lambda n: str(tmp_path / n)
    for name in ("synth_var.fastq", "example.fastq"):
        with open(P(name), "wb") as f:
            f.write(M.golden_text(name))
    text = M.synth_var()
    for flags in ([], ["-0"]):
        r = _run([tool, "-c", P("synth_var.fastq"), "-o", P("sv.fq.gz")] + flags)
        assert r.returncode == 0, r.stderr
        blob = open(P("sv.fq.gz"), "rb").read()
        assert blob == (models["synth_var"] if not flags else api.HostText.bgzf_deflate_model(text, level=0).tobytes())
        r = _run([tool, "-t", P("sv.fq.gz")])
        assert r.returncode == 0 and b"190990 bytes verified" in r.stdout, r.stderr
        r = _run([tool, "-d", P("sv.fq.gz"), "-o", P("back.fq")])
        assert r.returncode == 0 and open(P("back.fq"), "rb").read() == text, r.stderr
        r = _run([tool, "-l", P("sv.fq.gz")])
        assert r.returncode == 0 and r.stdout.decode().startswith("4 members, %d bytes compressed, 190990 bytes raw" % len(blob))
        # a consumer of FASTQ takes the result: gsufsort on the .fq.gz writes the golden eBWT
        r = _run([tool, "-c", P("example.fastq"), "-o", P("example.fastq.gz")] + flags)
        assert r.returncode == 0, r.stderr
        r = _run([os.path.join(DROP, "external", "gsufsort", "gsufsort"), P("example.fastq.gz"), "--bwt", "--qs", "-o", P("OUT")])
        assert r.returncode == 0, r.stdout + r.stderr
        assert open(P("OUT.bwt"), "rb").read() == M.golden_text("example.bwt")
    # an input that is already compressed: exit 1, the message, an empty output
    r = _run([tool, "-c", P("sv.fq.gz"), "-o", P("twice.gz")])
    assert r.returncode == 1 and b"already compressed" in r.stderr and os.path.getsize(P("twice.gz")) == 0


def test_restore_to_bgzf(engine, tmp_path):
    restore = os.path.join(DROP, "bfq_restore")
    P = lambda n: str(tmp_path / n)
    text = M.golden_text("example.fastq")

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
    for tag, args in (("a", plain), ("b", kept)):
        r = _run([restore] + args + ["-o", P(tag + ".fq")])
        assert r.returncode == 0, r.stderr
        want = open(P(tag + ".fq"), "rb").read()
        r = _run([restore] + args + ["-z", "-o", P(tag + ".fq.gz")])
        assert r.returncode == 0, r.stderr
        blob = open(P(tag + ".fq.gz"), "rb").read()
        assert gzip.decompress(blob) == want and blob == api.HostText.bgzf_deflate_model(want).tobytes(), tag
        assert len(want) > 20000
    assert len(open(P("b.fq"), "rb").read()) == len(open(P("a.fq"), "rb").read())
    # the library call on named files
    n, reads = engine.fastq_restore_files(P("a.dna"), P("a.qs"), P("a.hdr"), P("lib.fq.gz"), bgzf=True)
    assert open(P("lib.fq.gz"), "rb").read() == open(P("a.fq.gz"), "rb").read() and n == os.path.getsize(P("a.fq.gz")) and reads > 0
    # the grouped restore is refused by name
    r = _run([restore] + plain + ["-g", "-z", "-o", P("g.fq.gz")])
    assert r.returncode != 0 and b"-z does not go with -g" in r.stderr
