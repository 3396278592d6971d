"""GPU tests of the quality container (bfqzip_amd/csrc/k_quals.hip, BFQQUAL1): the kernels against the Python statement
tests/quals_model.py byte for byte, the flags = 0 rule, a sampled model, the decoder's refusals, the container as the quality
stream of a job, of `bsc q`, of bfq_restore and of the sharded driver."""
import os, subprocess, sys
import numpy as np
import pytest
from bfqzip_amd import api, fastq
from tests import quals_model as qm, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
E_ARG = -1
CASES = qm.cases()
CASES["golden_synth_var"] = b"".join(open(os.path.join(util.GOLDEN, "synth_var.M2B0.fq"), "rb").readlines()[3::4])


def _u8(b):
    return np.frombuffer(b, np.uint8)


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_model(engine, name):
    """always, and every rung forced: the container of the statement, byte for byte; stream_decompress gives the input back."""
    data = CASES[name]
    for rung in (None, 0, 1, 2, 3):
        got = engine.quals_compress(_u8(data), always=True, rung=rung)
        want = qm.container(data, rung)
        assert got[:8].tobytes() == b"BFQQUAL1"
        assert got.tobytes() == want, (rung, len(got), len(want))
        assert engine.stream_decompress(got).tobytes() == data, rung
        assert int(engine.L.bfq_stream_raw_len(api._ptr(got), len(got))) == len(data)


@pytest.fixture(scope="module")
def shaped():
    return qm.shaped(20000, 100, 7)


def test_flags_0_keeps_the_shorter_container(engine, shaped):
    got = engine.quals_compress(_u8(shaped))
    general = engine.stream_compress(_u8(shaped))
    print("shaped 20000 x 100: BFQRANS2", len(general), "BFQQUAL1", len(got), "rung", int.from_bytes(got[44:48].tobytes(), "little"))
    assert got[:8].tobytes() == b"BFQQUAL1" and len(got) < len(general)
    assert got.tobytes() == qm.choose(shaped)
    assert engine.stream_decompress(got).tobytes() == shaped
    rnd = qm.lines_of(np.random.default_rng(1).integers(33, 73, 300).reshape(3, 100))
    assert engine.quals_compress(_u8(rnd)).tobytes() == engine.stream_compress(_u8(rnd)).tobytes() == qm.choose(rnd)
    assert engine.quals_compress(_u8(rnd), always=True).tobytes() == qm.container(rnd)
    # a forced rung without "always" is still held to the rule
    assert engine.quals_compress(_u8(rnd), rung=2).tobytes() == engine.stream_compress(_u8(rnd)).tobytes()


def test_ineligible_streams_take_the_general_container(engine):
    for name, data in qm.ineligible_cases().items():
        want = engine.stream_compress(_u8(data)).tobytes()
        assert want == qm.general(data), name
        for always in (False, True):
            assert engine.quals_compress(_u8(data), always=always).tobytes() == want, (name, always)
    out = np.empty(engine.stream_bound(8), np.uint8)
    ol = api.C.c_uint64(0)
    for flags in (4, 0x100, 0x400, 1 << 31):                          # unknown bits; a rung without "rung forced"
        assert engine.L.bfq_quals_compress(engine.h, api._ptr(_u8(b"II\n")), 3, flags, api._ptr(out), len(out), api.C.byref(ol)) == E_ARG


def test_sampled_model(engine):
    """2^25 + 2^20 values: the model is counted on every second segment (St = 2).  A value and a context that occur only in
    segments the sample skips are coded through the shares every row keeps for every symbol.  Round trip and checksum only."""
    rng = np.random.default_rng(9)
    nreads, length = (2 ** 25 + 2 ** 20) // 128, 128
    walk = np.clip(np.cumsum(rng.integers(-1, 2, (nreads, length), dtype=np.int8), axis=1, dtype=np.int16) + 38, 2, 41).astype(np.uint8) + 33
    walk[8 + 3, 5:9] = 110                         # segment 1 (reads 8..15): a value no sampled segment holds
    walk[24 + 1, ::2] = 35; walk[24 + 1, 1::2] = 74   # segment 3: a read noisier than any other
    data = np.concatenate([walk, np.full((nreads, 1), 10, np.uint8)], axis=1).reshape(-1)
    assert qm.sample_step(nreads * length) == 2
    z = engine.quals_compress(data, always=True)
    assert z[:8].tobytes() == b"BFQQUAL1" and int.from_bytes(z[24:32].tobytes(), "little") == nreads * length
    A = int.from_bytes(z[40:44].tobytes(), "little")
    assert A == len(np.unique(walk)) and 110 in z[72 + int.from_bytes(z[64:72].tobytes(), "little"):][:A]
    assert int.from_bytes(z[56:64].tobytes(), "little") == qm.checksum(data)
    assert len(z) < len(data) // 2
    assert np.array_equal(engine.stream_decompress(z), data)


def test_device_buffers_and_a_growing_workspace(shaped):
    """bfq_quals_compress_device on torch tensors gives the host entry point's bytes.  The workspace is sized from the length
    for reads of 64 values and more; a stream of the same length in lines of 3 needs more and the workspace grows on the way."""
    import torch
    long_lines = shaped[:4_040_000 // 2]
    short_lines = qm.lines_of(np.random.default_rng(2).integers(40, 48, (len(long_lines) // 4, 3)))
    assert len(short_lines) == len(long_lines)
    sizes = {}
    for name, data in (("long", long_lines), ("short", short_lines)):
        eng = api.Engine(0)
        try:
            d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            cap = eng.stream_bound(len(data))
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            for always in (False, True):
                n = eng.quals_compress_device(d_in.data_ptr(), len(data), d_out.data_ptr(), cap, always=always)
                assert d_out[:n].cpu().numpy().tobytes() == eng.quals_compress(_u8(data), always=always).tobytes(), (name, always)
            assert eng.stream_decompress(d_out[:n].cpu().numpy()).tobytes() == data
            sizes[name] = eng.workspace_bytes()
        finally:
            eng.close()
    assert sizes["short"] > sizes["long"] + 24 * (len(short_lines) // 4 - len(long_lines) // 64)


def test_refusals(engine):
    """Containers whose header, lens member, model or payload lie: BFQ_E_ARG, the message names the container, nothing is
    written to the caller's buffer, and the engine goes on."""
    good, cases = qm.refusal_cases()
    ok = qm.container(good, rung=1)
    assert engine.stream_decompress(_u8(ok)).tobytes() == good
    for name, blob in cases.items():
        sentinel = np.full(len(good) + 4096, 0xA5, np.uint8)
        with pytest.raises(api.BfqError, match="BFQQUAL1") as e:
            engine.stream_decompress(_u8(blob), out=sentinel)
        assert e.value.code == E_ARG, name
        assert (sentinel == 0xA5).all(), name
    assert engine.stream_decompress(_u8(ok)).tobytes() == good
    # ... and as the quality stream of a restore
    dna = engine.stream_compress(_u8(good.translate(bytes(10 if b == 10 else 65 for b in range(256)))))
    out, nr = engine.fastq_restore(dna, _u8(ok), None)
    assert nr == good.count(b"\n") and out.tobytes().split(b"\n")[3::4] == good.split(b"\n")[:-1]
    sentinel = np.full(4 * len(good) + 4096, 0xA5, np.uint8)
    with pytest.raises(api.BfqError, match="BFQQUAL1") as e:
        engine.fastq_restore(dna, _u8(cases["payload_flip_3"]), None, out=sentinel)
    assert e.value.code == E_ARG and (sentinel == 0xA5).all()


@pytest.fixture(scope="module")
def collection():
    rng = np.random.default_rng(20261018)
    b, _, r = util.random_reads(rng, 3000, 100, 100)
    q = _u8(qm.shaped(3000, 100, 3).replace(b"\n", b""))
    return fastq.format_fastq(b, q, r, [b"@r%d" % i for i in range(3000)])


@pytest.mark.parametrize("compress", [1, 3])
def test_job_with_quals(engine, collection, compress):
    engine.set_params(m=5)
    try:
        text = _u8(collection)
        plain = engine.fastq_job([text], keep_headers=True, fastq=True, streams=True, hdr=True)
        z0 = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=compress)
        z0 = (np.array(z0.dna), np.array(z0.qs), np.array(z0.hdr), z0.stats)
        z1 = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=compress, quals=True)
        assert np.array_equal(z1.dna, z0[0]) and np.array_equal(z1.hdr, z0[2]) and z1.stats == z0[3]
        qs = np.array(z1.qs)
        raw = engine.stream_decompress(z0[1]).tobytes()
        if compress == 1:
            assert raw == np.asarray(plain.qs).tobytes()
        assert engine.stream_decompress(qs).tobytes() == raw
        assert qs.tobytes() == engine.quals_compress(_u8(raw)).tobytes() == qm.choose(raw)
        assert len(qs) <= len(z0[1])
        want = np.asarray(plain.fastq).tobytes()
        out, nr = engine.fastq_restore(z1.dna, qs, z1.hdr)
        assert nr == 3000 and out.tobytes() == want
        with pytest.raises(api.BfqError) as e:
            engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=2, quals=True)
        assert e.value.code == E_ARG
    finally:
        engine.set_params()


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, **kw)


def test_front_ends(tmp_path, shaped):
    """`bsc q` then `bsc d` round-trip a file; bfq_restore takes the `bsc q` output as its quality input."""
    bsc, restore = os.path.join(DROP, "external/libbsc/bsc"), os.path.join(DROP, "bfq_restore")
    for p in (bsc, restore):
        assert os.path.exists(p), f"{p} missing: run __graft_entry__.build()"
    qs = shaped
    dna = qs.translate(bytes(10 if b == 10 else b"ACGT"[b & 3] for b in range(256)))
    open(tmp_path / "qs", "wb").write(qs)
    open(tmp_path / "dna", "wb").write(dna)
    for k, verb in (("qs", "q"), ("dna", "e")):
        r = _run([bsc, verb, str(tmp_path / k), str(tmp_path / (k + ".bsc"))])
        assert r.returncode == 0, r.stdout
    z = open(tmp_path / "qs.bsc", "rb").read()
    assert z[:8] == b"BFQQUAL1" and z == qm.choose(qs)
    r = _run([bsc, "d", str(tmp_path / "qs.bsc"), str(tmp_path / "qs.back")])
    assert r.returncode == 0, r.stdout
    assert open(tmp_path / "qs.back", "rb").read() == qs
    r = _run([restore, "-d", str(tmp_path / "dna.bsc"), "-q", str(tmp_path / "qs.bsc"), "-o", str(tmp_path / "back.fq")])
    assert r.returncode == 0, r.stdout
    ql, dl = qs.split(b"\n")[:-1], dna.split(b"\n")[:-1]
    assert open(tmp_path / "back.fq", "rb").read() == b"".join(b"@\n" + d + b"\n+\n" + q + b"\n" for d, q in zip(dl, ql))
    _, cases = qm.refusal_cases()
    open(tmp_path / "bad.bsc", "wb").write(cases["zeroed_segment"])
    r = _run([bsc, "d", str(tmp_path / "bad.bsc"), str(tmp_path / "bad.out")])
    assert r.returncode == 1 and b"BFQQUAL1" in r.stdout, r.stdout


def test_sharded_run_with_quals(tmp_path, collection):
    """parallel.py -t 2 --compress --quals on one GPU, then bfq_restore: the merged FASTQ of the same run without --compress.
    Every block's quality share is its own member."""
    src = str(tmp_path / "in.fastq")
    open(src, "wb").write(collection)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    plain, z = str(tmp_path / "P"), str(tmp_path / "Z")
    for args in ([src, "-o", plain, "-t", "2", "-H", "--m3"], [src, "-o", z, "-t", "2", "-H", "--m3", "--compress", "--quals"]):
        r = _run([sys.executable, "-m", "bfqzip_amd.parallel"] + args, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout.decode()[-3000:]
    qz = open(z + ".fastq.qs.bsc", "rb").read()
    raw = open(plain + ".fastq.qs", "rb").read()
    first = int.from_bytes(qz[8:16], "little")
    assert 0 < first < len(raw)                                    # two members: the first is not the whole stream
    assert qz == qm.choose(raw[:first]) + qm.choose(raw[first:])
    r = _run([os.path.join(DROP, "bfq_restore"), "-d", z + ".fastq.dna.bsc", "-q", z + ".fastq.qs.bsc", "-H", z + ".h.bsc", "-o", z + ".back.fastq"])
    assert r.returncode == 0, r.stdout
    assert open(z + ".back.fastq", "rb").read() == open(plain + ".fastq", "rb").read()
