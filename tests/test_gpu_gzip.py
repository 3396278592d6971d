"""GPU tests of the plain gzip input (bfq_gzip_*, k_gzip.hip): the inflated text equals zlib's over the model's inputs
(tests/gzip_model.py) at several piece sizes, into host and device buffers with guard bands; the statistics equal the host
form's; every refusal names the member, its offset and the reason, and leaves the engine usable.  The refusal inputs have
passed the host program under sanitizers first (tests/test_gzip_host.py): they test refusal, none is meant to fault."""
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import gzip_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
E_ARG = -1
GUARD = 4096
CHUNKS = (1024, 4096, 0)
host = api.HostText


@pytest.fixture(scope="module")
def cases():
    """name -> (gzip bytes, zlib's text, {chunk: the host form's statistics}); made once"""
    out = {}
    for name, blob in M.good().items():
        out[name] = (blob, M.expected(blob), {c: host.gzip_inflate_host(blob, c)[1].as_dict() for c in CHUNKS})
    return out


@pytest.mark.parametrize("name", M.GOOD_NAMES)
def test_inflate_into_host_and_device_buffers(engine, cases, name):
    import torch
    blob, text, want = cases[name]
    assert len(text) <= 3_000_000
    for chunk in CHUNKS:
        buf = np.full(len(text) + 2 * GUARD, 0xA5, np.uint8)
        got, st = engine.gzip_inflate(blob, out=buf[GUARD:GUARD + len(text)], chunk=chunk)
        assert len(got) == len(text) and got.tobytes() == text, (name, chunk)
        assert (buf[:GUARD] == 0xA5).all() and (buf[GUARD + len(text):] == 0xA5).all(), (name, chunk)
        assert st.as_dict() == want[chunk], (name, chunk)
        d = torch.full((len(text) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        n, st = engine.gzip_inflate_device(blob, d.data_ptr() + GUARD, len(text), chunk=chunk)
        h = d.cpu().numpy()
        assert n == len(text) and h[GUARD:GUARD + n].tobytes() == text, (name, chunk)
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all(), (name, chunk)
        assert st.as_dict() == want[chunk], (name, chunk)
        assert engine.gzip_measure(blob, chunk)[:2] == (len(text), want[chunk]["members"]), (name, chunk)


def test_chain_is_parallel_on_the_gpu(engine, cases):
    blob, text, _ = cases["a-l6-m1"]
    got, st = engine.gzip_inflate(blob, chunk=4096)
    assert got.tobytes() == text and st.chain >= 20 and st.skipped == 0
    assert engine.gzip_inflate(cases["d-big-m1"][0], chunk=4096)[1].chain >= 20
    assert engine.gzip_inflate(cases["e-repeat"][0], chunk=1024)[1].chain >= 20
    st = engine.gzip_inflate(cases["i-false"][0], chunk=1024)[1]
    assert st.discarded == 1 and st.chain == st.decoders - 1


def test_buffer_too_small(engine, cases):
    import torch
    blob, text, _ = cases["a-l6-m1"]
    buf = np.full(1000, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.gzip_inflate(blob, out=buf)
    assert e.value.code == E_ARG and e.value.needed == len(text) and (buf == 0xA5).all()
    d = torch.full((1000 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(api.BfqError) as e:
        engine.gzip_inflate_device(blob, d.data_ptr(), 1000)
    assert e.value.code == E_ARG and e.value.needed == len(text) and bool((d == 0xA5).all())
    with pytest.raises(api.BfqError) as e:
        engine.gzip_inflate(blob, chunk=3000)
    assert e.value.code == E_ARG and "power of two" in str(e.value)
    assert engine.gzip_inflate(blob)[0].tobytes() == text


def test_refusals(engine, cases):
    good, good_text, _ = cases["a-l1-m1"]
    for name, (blob, reason, member, off) in M.refusals().items():
        for chunk in (1024, 0):
            with pytest.raises(api.BfqError) as e:
                engine.gzip_inflate(blob, out=np.empty(1 << 20, np.uint8), chunk=chunk)
            assert e.value.code == E_ARG and str(e.value).endswith(M.message(member, off, reason)), (name, chunk, str(e.value))
        assert engine.gzip_inflate(good, chunk=1024)[0].tobytes() == good_text, name


def test_tool(tmp_path, cases):
    tool = os.path.join(DROP, "bfq_bgzf")
    blob, text, want = cases["f-inside"]
    gz, out = str(tmp_path / "in.fq.gz"), str(tmp_path / "out.fq")
    with open(gz, "wb") as f:
        f.write(blob)
    run = lambda *a: subprocess.run([tool] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    r = run("-g", "-l", gz)
    w = want[0]
    assert r.returncode == 0 and r.stdout.decode().startswith("3 members, %d bytes compressed, %d bytes raw, %d pieces, chain %d, %d candidates skipped"
                                                              % (len(blob), len(text), w["pieces"], w["chain"], w["skipped"])), (r.stdout, r.stderr)
    r = run("-g", "-d", gz, "-o", out)
    assert r.returncode == 0 and open(out, "rb").read() == text, r.stderr
    r = run("-g", "-t", gz)
    assert r.returncode == 0 and ("%d bytes verified" % len(text)).encode() in r.stdout
    r = run("-t", gz)                                               # without -g: today's words
    assert r.returncode == 1 and b"recompress it with bgzip" in r.stderr
    r = run("-l", gz)
    assert r.returncode == 1 and b"recompress it with bgzip" in r.stderr
    bad, reason, member, off = M.refusals()["dist-far"]
    with open(gz, "wb") as f:
        f.write(bad)
    for args in (("-g", "-d", gz, "-o", out), ("-g", "-t", gz), ("-g", "-l", gz)):
        r = run(*args)
        assert r.returncode == 1 and M.message(member, off, reason).encode() in r.stderr, (args, r.stderr)
    assert os.path.getsize(out) == 0


def test_parallel_gunzip(tmp_path):
    text = M.B.golden_text("example.fastq")
    plain, gz = str(tmp_path / "in.fastq"), str(tmp_path / "in.fastq.gz")
    with open(plain, "wb") as f:
        f.write(text)
    with open(gz, "wb") as f:
        f.write(M.gz(text, 6, 1))
    for d in "abc":
        os.mkdir(str(tmp_path / d))
    assert parallel.main([plain, "-o", str(tmp_path / "a" / "OUT"), "-t", "2", "-0", "--m3"]) == 0
    assert parallel.main([gz, "-o", str(tmp_path / "b" / "OUT"), "-t", "2", "-0", "--m3", "--gunzip"]) == 0
    assert parallel.main([gz, "-o", str(tmp_path / "c" / "OUT"), "-t", "2", "-0", "--m3", "--gunzip", "--keep-inflated"]) == 0
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and len(names) == 4       # the inflated temporary is gone
    assert sorted(os.listdir(str(tmp_path / "c"))) == sorted(names + ["in.inflated.fastq"])
    assert open(str(tmp_path / "c" / "in.inflated.fastq"), "rb").read() == text
    for n in names:
        want = open(str(tmp_path / "a" / n), "rb").read()
        assert open(str(tmp_path / "b" / n), "rb").read() == want and open(str(tmp_path / "c" / n), "rb").read() == want, n
    with pytest.raises(api.BfqError) as e:                          # without --gunzip the library's message stands
        parallel.main([gz, "-o", str(tmp_path / "b" / "OUT2"), "-t", "2", "-0", "--m3"])
    assert "recompress it with bgzip" in str(e.value)
