"""GPU tests of the tokenised read names (bfqzip_amd/csrc/k_names.hip, the BFQNAME1 container): the kernels against the Python
statement tests/names_model.py byte for byte, the flags = 0 rule, the decoder's refusals, the container as the header
stream of a job, of `bsc n`, of bfq_restore and of the sharded driver."""
import os, subprocess, sys
import numpy as np
import pytest
from bfqzip_amd import api, fastq
from tests import names_model as nm, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
E_ARG = -1
CASES = nm.edge_cases()


def _u8(b):
    return np.frombuffer(b, np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_always_equals_the_model(engine, name):
    """always = True: the container of the statement, byte for byte, and stream_decompress gives the input back."""
    data = CASES[name]
    got = engine.names_compress(_u8(data), always=True)
    want = nm.container(data)
    assert got[:8].tobytes() == b"BFQNAME1"
    assert got.tobytes() == want, (len(got), len(want))
    assert engine.stream_decompress(got).tobytes() == data
    assert int(engine.L.bfq_stream_raw_len(api._ptr(got), len(got))) == len(data)


@pytest.fixture(scope="module")
def families():
    return {"sra": nm.sra_names(30000), "illumina": nm.illumina_names(30000), "syn": nm.syn_names(30000)}


def test_flags_0_keeps_the_shorter_container(engine, families):
    for name, data in families.items():
        got = engine.names_compress(_u8(data))
        assert got[:8].tobytes() == b"BFQNAME1" and got.tobytes() == nm.choose(data), name
        assert len(got) < len(engine.stream_compress(_u8(data))), name
        assert engine.stream_decompress(got).tobytes() == data, name
    example = b"".join(open(os.path.join(util.GOLDEN, "example.fastq"), "rb").readlines()[0::4])
    for name, data in (("syn_300", nm.syn_names(300)), ("random_lines", nm.random_lines(3000, 40)), ("example", example)):
        got = engine.names_compress(_u8(data))
        assert got[:8].tobytes() != b"BFQNAME1", name
        assert got.tobytes() == nm.choose(data) == engine.stream_compress(_u8(data)).tobytes(), name
        assert engine.names_compress(_u8(data), always=True).tobytes() == nm.container(data), name


def test_ineligible_streams_take_the_general_container(engine):
    for name, data in nm.ineligible_cases().items():
        want = engine.stream_compress(_u8(data)).tobytes()
        assert want == nm.general(data), name
        for always in (False, True):
            assert engine.names_compress(_u8(data), always=always).tobytes() == want, (name, always)
    out = np.empty(engine.stream_bound(8), np.uint8)
    ol = api.C.c_uint64(0)
    assert engine.L.bfq_names_compress(engine.h, api._ptr(_u8(b"@r 1\n")), 5, 2, api._ptr(out), len(out), api.C.byref(ol)) == E_ARG   # an unknown flag


def test_device_buffers_and_a_growing_workspace(families):
    """bfq_names_compress_device on torch tensors gives the host entry point's bytes.  A fresh engine sizes its workspace for
    typical lines; 8 M empty lines need more for their index than that and the workspace grows on the way."""
    import torch
    eng = api.Engine(0)
    try:
        for name in ("sra", "syn"):
            data = families[name]
            d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            cap = eng.stream_bound(len(data))
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            for always in (False, True):
                n = eng.names_compress_device(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, always=always)
                assert d_out[:n].cpu().numpy().tobytes() == eng.names_compress(_u8(data), always=always).tobytes() == nm.choose(data), (name, always)
    finally:
        eng.close()
    eng = api.Engine(0)
    try:
        data = np.full(8_000_000, 10, np.uint8)
        before = eng.workspace_bytes()
        z = eng.names_compress(data, always=True)
        assert z[:8].tobytes() == b"BFQNAME1" and int(np.frombuffer(z[24:32].tobytes(), np.uint64)[0]) == len(data)
        assert eng.workspace_bytes() > before + 44 * len(data)
        assert np.array_equal(eng.stream_decompress(z), data)
        small = nm.edge_cases()["zeros"]
        assert eng.names_compress(_u8(small), always=True).tobytes() == nm.container(small)
    finally:
        eng.close()


def test_refusals(engine):
    """Containers that parse and whose members' checksums hold, but whose streams lie: BFQ_E_ARG, the message names the
    container, nothing is read or written beyond the stated shares, and the engine goes on."""
    good, cases = nm.refusal_cases()
    ok = nm.container(good)
    assert engine.stream_decompress(_u8(ok)).tobytes() == good
    for name, blob in cases.items():
        with pytest.raises(api.BfqError, match="BFQNAME1") as e:
            engine.stream_decompress(_u8(blob))
        assert e.value.code == E_ARG, name
        assert engine.stream_decompress(_u8(ok)).tobytes() == good, name
    # ... and as the header stream of a restore
    dna, qs = engine.stream_compress(_u8(b"ACGT\nACGT\n")), engine.stream_compress(_u8(b"IIII\nIIII\n"))
    out, nr = engine.fastq_restore(dna, qs, _u8(ok))
    assert out.tobytes() == b"ab 12\nACGT\n+\nIIII\nab 13\nACGT\n+\nIIII\n" and nr == 2
    sentinel = np.full(4096, 0xA5, np.uint8)
    with pytest.raises(api.BfqError, match="BFQNAME1") as e:
        engine.fastq_restore(dna, qs, _u8(cases["op_byte_1"]), out=sentinel)
    assert e.value.code == E_ARG and (sentinel == 0xA5).all()


@pytest.fixture(scope="module")
def collection():
    rng = np.random.default_rng(20261018)
    b, q, r = util.random_reads(rng, 3000, 30, 120)
    hdrs = [b"@SRR1770413.%d %d length=%d" % (i + 1, i + 1, int(r[i + 1] - r[i])) for i in range(3000)]
    return fastq.format_fastq(b, q, r, hdrs)


@pytest.mark.parametrize("compress", [1, 3])
def test_job_with_tokenised_names(engine, collection, compress):
    engine.set_params(m=5)
    try:
        texts, permz = engine.fastq_reorder([collection], mode=2, keep=True)
        text = np.array(texts[0])
        plain = engine.fastq_job([text], keep_headers=True, fastq=True, streams=True, hdr=True)
        z0 = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=compress)
        z1 = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=compress, names=True)
        z0 = (np.array(z0.dna), np.array(z0.qs), np.array(z0.hdr), z0.stats)
        assert np.array_equal(z1.dna, z0[0]) and np.array_equal(z1.qs, z0[1]) and z1.stats == z0[3]
        hdr = np.array(z1.hdr)
        raw = np.asarray(plain.hdr).tobytes()
        assert hdr[:8].tobytes() == b"BFQNAME1" and len(hdr) < len(z0[2])
        assert hdr.tobytes() == nm.choose(raw) == engine.names_compress(_u8(raw)).tobytes()
        assert engine.stream_decompress(hdr).tobytes() == raw
        want = np.asarray(plain.fastq).tobytes()
        out, nr = engine.fastq_restore(z1.dna, z1.qs, hdr)
        assert nr == 3000 and out.tobytes() == want
        back, nr = engine.fastq_restore(z1.dna, z1.qs, hdr, perm=permz)
        assert nr == 3000 and back.tobytes() == engine.fastq_unreorder([_u8(want)], permz)[0].tobytes()
        assert sorted(back.tobytes().split(b"\n")[0::4][:-1]) == sorted(collection.split(b"\n")[0::4][:-1])
    finally:
        engine.set_params()


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, **kw)


def test_front_ends(tmp_path, collection):
    """`bsc n` then `bsc d` round-trip a file; bfq_restore -H takes the `bsc n` output (and the file entry points with it)."""
    bsc, restore = os.path.join(DROP, "external/libbsc/bsc"), os.path.join(DROP, "bfq_restore")
    for p in (bsc, restore):
        assert os.path.exists(p), f"{p} missing: run __graft_entry__.build()"
    lines = collection.split(b"\n")[:-1]
    streams = {"h": lines[0::4], "dna": lines[1::4], "qs": lines[3::4]}
    for k, v in streams.items():
        open(tmp_path / k, "wb").write(b"".join(x + b"\n" for x in v))
        r = _run([bsc, "n" if k == "h" else "e", str(tmp_path / k), str(tmp_path / (k + ".bsc"))])
        assert r.returncode == 0, r.stdout
    z = open(tmp_path / "h.bsc", "rb").read()
    assert z == nm.choose(open(tmp_path / "h", "rb").read()) and z[:8] == b"BFQNAME1"
    r = _run([bsc, "d", str(tmp_path / "h.bsc"), str(tmp_path / "h.back")])
    assert r.returncode == 0, r.stdout
    assert open(tmp_path / "h.back", "rb").read() == open(tmp_path / "h", "rb").read()
    r = _run([restore, "-d", str(tmp_path / "dna.bsc"), "-q", str(tmp_path / "qs.bsc"), "-H", str(tmp_path / "h.bsc"), "-o", str(tmp_path / "back.fq")])
    assert r.returncode == 0, r.stdout
    want = b"".join(lines[i] + b"\n" if i % 4 != 2 else b"+\n" for i in range(len(lines)))
    assert open(tmp_path / "back.fq", "rb").read() == want
    # a damaged container: exit 1, the message names it, the output is left empty
    _, cases = nm.refusal_cases()
    open(tmp_path / "bad.bsc", "wb").write(cases["one_end_too_few"])
    r = _run([bsc, "d", str(tmp_path / "bad.bsc"), str(tmp_path / "bad.out")])
    assert r.returncode == 1 and b"BFQNAME1" in r.stdout, r.stdout


def test_sharded_run_with_names(tmp_path, collection):
    """parallel.py -t 2 --compress --names -H (with the --m3 streams) on one GPU, then bfq_restore: the merged FASTQ of the
    same run without --compress.  Every block's header share is its own member."""
    src = str(tmp_path / "in.fastq")
    open(src, "wb").write(collection)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    plain, z = str(tmp_path / "P"), str(tmp_path / "Z")
    for args in ([src, "-o", plain, "-t", "2", "-H", "--m3"], [src, "-o", z, "-t", "2", "-H", "--m3", "--compress", "--names"]):
        r = _run([sys.executable, "-m", "bfqzip_amd.parallel"] + args, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
    hz = open(z + ".h.bsc", "rb").read()
    raw = open(plain + ".h", "rb").read()
    nlines = raw.count(b"\n")
    first = int.from_bytes(hz[8:16], "little")
    assert hz[:8] == b"BFQNAME1" and 0 < first < len(raw)                   # two members: the first is not the whole stream
    cut = len(nm.choose(raw[:first]))
    assert hz == nm.choose(raw[:first]) + nm.choose(raw[first:]) and hz[cut:cut + 8] == b"BFQNAME1" and nlines == 3000
    r = _run([os.path.join(DROP, "bfq_restore"), "-d", z + ".fastq.dna.bsc", "-q", z + ".fastq.qs.bsc", "-H", z + ".h.bsc", "-o", z + ".back.fastq"])
    assert r.returncode == 0, r.stdout
    assert open(z + ".back.fastq", "rb").read() == open(plain + ".fastq", "rb").read()
