"""GPU tests of the way back (bfq_fastq_restore / bfq_fastq_restore_fd / dropin/bfq_restore): the containers a run writes
-> the FASTQ text, in one call.  Pinned to the reference through the md5s of tests/golden/index.json (files written by the
compiled bfq_int), to the forward path (the out_fastq of the same job), and to the input itself where nothing is smoothed.
Every refusal is found on the host or by the validator kernel before anything is written."""
import os, subprocess
import numpy as np
import pytest
from bfqzip_amd import api, fastq, parallel
from tests import util
from tests.test_parallel_gloo import paired_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
IDX = util.golden_index()
E_ARG, E_NOMEM = -1, -7
SENTINEL = 0xA5


def _raw(name):
    return open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read()


def _restore_of_job(engine, text, keep_headers, compress):
    z = engine.fastq_job([text], keep_headers=keep_headers, fastq=False, streams=True, hdr=keep_headers, compress=compress)
    out, nr = engine.fastq_restore(z.dna, z.qs, z.hdr if keep_headers else None)
    assert nr == z.n_reads
    return out.tobytes()


@pytest.mark.parametrize("name", list(IDX))
def test_restore_gives_the_reference_files(engine, name):
    """Every (M, B) and flag set of the golden index, -H included: compress -> restore = what the reference's bfq_int wrote."""
    text = _raw(name)
    try:
        for key, want in IDX[name]["out"].items():
            d, hdr = util.parse_case(key)
            engine.set_params(**d)
            assert util.md5(_restore_of_job(engine, text, hdr, 1)) == want, key
            if key.startswith("M2B0"):
                for mode in (2, 3):                                   # eBWT-domain containers
                    assert util.md5(_restore_of_job(engine, text, hdr, mode)) == want, (key, mode)
    finally:
        engine.set_params()


def _collection(rng, nreads, lmin, lmax, **kw):
    b, q, r = util.random_reads(rng, nreads, lmin, lmax, **kw)
    hdrs = [b"@r%d/%d len=%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), int(r[i + 1] - r[i])) for i in range(nreads)]
    return fastq.format_fastq(b, q, r, hdrs)


def test_restore_equals_the_forward_path(engine):
    """restore(compress(job)) == out_fastq of the same job run uncompressed, with and without headers, for the three kinds
    of containers: variable lengths 1..300, N's, duplicates, a single read, no read at all, and a golden input."""
    rng = np.random.default_rng(20241016)
    texts = [_collection(rng, 300, 1, 300), _collection(rng, 4000, 20, 300, p_n=0.2, dup=0.5), _collection(rng, 1, 1, 1),
             _collection(rng, 1, 300, 300), _collection(rng, 50, 1, 3), _raw("synth_var"), b""]
    engine.set_params(m=3, k=8)
    try:
        for t in texts:
            for kh in (False, True):
                plain = engine.fastq_job([t], keep_headers=kh, fastq=True)
                for mode in (1, 2, 3):
                    assert _restore_of_job(engine, t, kh, mode) == plain.fastq.tobytes(), (len(t), kh, mode)
    finally:
        engine.set_params()


@pytest.fixture(scope="module")
def big(engine):
    """2 M x 100 synthetic reads with headers, K above every LCP (nothing is smoothed), and their read-order containers:
    more than 65 536 segments and several BFQDNAC1 blocks (tests/test_gpu_codec.py)."""
    sp = api.synth_spec(2_000_000, 100, seed=3)
    text = np.empty(2_000_000 * 260, np.uint8)
    n = engine.synth_fastq(sp, text)
    text = text[:n]
    engine.set_params(k=10000)
    try:
        z = engine.fastq_job([text], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1)
    finally:
        engine.set_params()
    return text, np.array(z.dna), np.array(z.qs), np.array(z.hdr)


def test_identity_at_size(engine, big):
    text, dna, qs, hdr = big
    assert dna[:8].tobytes() == b"BFQDNAC1"
    out, nr = engine.fastq_restore(dna, qs, hdr)
    assert nr == 2_000_000 and len(out) == len(text) and np.array_equal(out, text)
    pin = api.PinnedBuffer(len(text) + 64)                             # a pinned destination: direct DMA
    try:
        out, nr = engine.fastq_restore(dna, qs, hdr, out=pin.array)
        assert len(out) == len(text) and np.array_equal(out, text)
    finally:
        pin.free()
    prof = engine.prof()
    assert prof["k_restore_index"]["launches"] >= 2 and prof["k_fq_format_lines"]["launches"] >= 2


@pytest.mark.parametrize("paired", [False, True])
def test_members_back_to_back(engine, tmp_path, paired):
    """parallel.py --compress with t = 3: one container per block (per mate) in every .bsc; each OUT / OUT_1 / OUT_2 set
    restores on its own, through the file entry point, to the .fastq of the run without step 5."""
    if paired:
        inputs = list(paired_inputs(str(tmp_path)))
    else:
        inputs = [os.path.join(util.GOLDEN, "synth_var.fastq")]
    engine.set_params(m=5)
    try:
        plain = parallel.output_names(inputs, str(tmp_path / "P"), paired)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, plain, paired=paired, headers=True, want_streams=True, want_hdr=True)
        z = parallel.output_names(inputs, str(tmp_path / "Z"), paired)
        parallel.run_files(engine, parallel.Comm(), inputs, 3, z, paired=paired, headers=True, want_streams=True, want_hdr=True, compress=True)
        for o in range(len(plain)):
            want = open(plain[o]["fastq"], "rb").read()
            for kind in ("dna", "qs", "hdr"):                          # more than one member: the first one is not the whole stream
                blob = np.fromfile(z[o][kind] + ".bsc", np.uint8)
                first = int(np.frombuffer(blob[8:16].tobytes(), np.uint64)[0])
                assert 0 < first < int(engine.L.bfq_stream_raw_len(api._ptr(blob), len(blob))), kind
            back = str(tmp_path / f"back{o}.fastq")
            ol, nr = engine.fastq_restore_files(z[o]["dna"] + ".bsc", z[o]["qs"] + ".bsc", z[o]["hdr"] + ".bsc", back)
            got = open(back, "rb").read()
            assert ol == len(want) and got == want and nr == want.count(b"\n") // 4
            # without the header stream: "@" lines
            ol, nr = engine.fastq_restore_files(z[o]["dna"] + ".bsc", z[o]["qs"] + ".bsc", None, back)
            lines = want.split(b"\n")[:-1]
            assert open(back, "rb").read() == b"".join((b"@" if i % 4 == 0 else x) + b"\n" for i, x in enumerate(lines))
    finally:
        engine.set_params()


def _refused(engine, code, dna, qs, hdr=None, size=1 << 20, match=None):
    out = np.full(size, SENTINEL, np.uint8)
    with pytest.raises(api.BfqError, match=match) as e:
        engine.fastq_restore(dna, qs, hdr, out=out)
    assert e.value.code == code, str(e.value)
    assert (out == SENTINEL).all()
    return str(e.value)


def test_refusals_leave_the_output_untouched(engine, big):
    rng = np.random.default_rng(7)
    ta, tb = _collection(rng, 500, 30, 120), _collection(rng, 500, 30, 120)
    engine.set_params(m=5)
    try:
        za = engine.fastq_job([ta], keep_headers=True, fastq=True, streams=True, hdr=True, compress=1)
        zb = engine.fastq_job([tb], keep_headers=True, fastq=False, streams=True, hdr=True, compress=1)
        ra = engine.fastq_job([ta], keep_headers=True, fastq=False, streams=True, hdr=True)
        e2 = engine.fastq_job([ta], fastq=False, streams=True, compress=2)
    finally:
        engine.set_params()
    dna, qs, hdr, text = np.array(za.dna), np.array(za.qs), np.array(za.hdr), za.fastq.tobytes()
    size = len(text) + 4096
    out, nr = engine.fastq_restore(dna, qs, hdr)
    assert out.tobytes() == text and nr == 500
    # the qualities of another collection: the first read whose lengths differ is named
    la = [len(x) for x in ta.split(b"\n")[1::4]]
    lb = [len(x) for x in tb.split(b"\n")[1::4]]
    first = next(i for i in range(500) if la[i] != lb[i])
    _refused(engine, E_ARG, dna, np.array(zb.qs), hdr, size, match=rf"read {first}\b")
    # a header stream with one line less
    hl = np.asarray(ra.hdr).tobytes().split(b"\n")[:-1]
    short = engine.stream_compress(np.frombuffer(b"".join(x + b"\n" for x in hl[:-1]), np.uint8))
    _refused(engine, E_ARG, dna, qs, np.array(short), size, match=r"read 499\b.*header")
    # a quality stream with one line less
    ql = np.asarray(ra.qs).tobytes().split(b"\n")[:-1]
    short = engine.stream_compress(np.frombuffer(b"".join(x + b"\n" for x in ql[:-1]), np.uint8))
    _refused(engine, E_ARG, dna, np.array(short), hdr, size, match=r"read 499\b")
    # a truncated member, a raw stream instead of a container, two BFQEBWT1 members
    _refused(engine, E_ARG, dna[:len(dna) // 2], qs, hdr, size)
    _refused(engine, E_ARG, dna, qs[:len(qs) - 7], hdr, size)
    _refused(engine, E_ARG, np.asarray(ra.dna), qs, hdr, size, match="not a container")
    _refused(engine, E_ARG, dna, np.asarray(ra.qs), hdr, size, match="not a container")
    two = np.concatenate([np.asarray(e2.dna), np.asarray(e2.dna)])
    _refused(engine, E_ARG, two, np.asarray(e2.qs), None, size, match="more than one BFQEBWT1")
    assert engine.L.bfq_fastq_restore_bound(api._ptr(np.asarray(ra.dna)), len(ra.dna), api._ptr(qs), len(qs), None, 0) == -1
    # an output buffer one byte short of the text
    _refused(engine, E_ARG, dna, qs, hdr, len(text) - 1, match="output buffer")
    out = np.full(len(text), SENTINEL, np.uint8)
    got, _ = engine.fastq_restore(dna, qs, hdr, out=out)
    assert got.tobytes() == text
    # a workspace cap too small for the 2 M case: BFQ_E_NOMEM before anything is written; the same engine goes on
    btext, bdna, bqs, bhdr = big
    small = api.Engine(0, ws_cap_mib=512)
    try:
        msg = _refused(small, E_NOMEM, bdna, bqs, bhdr, 1 << 20, match="GiB")
        assert "cap" in msg
        got, nr = small.fastq_restore(dna, qs, hdr)
        assert got.tobytes() == text and nr == 500
    finally:
        small.close()


def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, **kw)


def test_front_end(tmp_path):
    """The flow of tests/test_gpu_cli.py (gsufsort, bfq_int -H), the line streams cut as BFQzip.py does with sed, `bsc e`
    on each, then bfq_restore: the file bfq_int wrote.  A bad pair: exit 1 and an empty output."""
    t = {k: os.path.join(DROP, p) for k, p in dict(gsufsort="external/gsufsort/gsufsort", bfq_int="src_int_mem/bfq_int",
                                                   bsc="external/libbsc/bsc", restore="bfq_restore").items()}
    for p in t.values():
        assert os.path.exists(p), f"{p} missing: run __graft_entry__.build()"
    out = str(tmp_path / "OUT")
    for name in ("example", "synth_fix"):
        fq = os.path.join(util.GOLDEN, name + ".fastq")
        with open(out + ".h", "wb") as f:                                  # sed -n 1~4p (BFQzip.py:192-203)
            f.write(b"".join(l for i, l in enumerate(open(fq, "rb").readlines()) if i % 4 == 0))
        assert _run([t["gsufsort"], fq, "--bwt", "--qs", "-o", out]).returncode == 0
        r = _run([t["bfq_int"], "-e", out + ".bwt", "-q", out + ".bwt.qs", "-o", out + ".fq", "-m", "5", "-H", out + ".h"])
        assert r.returncode == 0, r.stdout
        lines = open(out + ".fq", "rb").readlines()
        open(out + ".fq.dna", "wb").write(b"".join(lines[1::4]))           # sed -n 2~4p / 4~4p (BFQzip.py:20-21)
        open(out + ".fq.qs", "wb").write(b"".join(lines[3::4]))
        for s in (".fq.dna", ".fq.qs", ".h"):
            r = _run([t["bsc"], "e", out + s, out + s + ".bsc", "-T"])
            assert r.returncode == 0, r.stdout
        r = _run([t["restore"], "-d", out + ".fq.dna.bsc", "-q", out + ".fq.qs.bsc", "-H", out + ".h.bsc", "-o", out + ".back.fq", "-V"])
        assert r.returncode == 0 and b"[bfq phases]" in r.stdout, r.stdout
        assert open(out + ".back.fq", "rb").read() == open(out + ".fq", "rb").read()
        r = _run([t["restore"], "-d", out + ".fq.dna.bsc", "-q", out + ".fq.qs.bsc", "-o", out + ".at.fq"])
        assert r.returncode == 0, r.stdout
        assert open(out + ".at.fq", "rb").read() == b"".join(b"@\n" if i % 4 == 0 else l for i, l in enumerate(lines))
        os.replace(out + ".fq.qs.bsc", out + "." + name + ".qs.bsc")
    # the DNA of synth_fix with the qualities of example; a raw stream
    for bad in ([t["restore"], "-d", out + ".fq.dna.bsc", "-q", out + ".example.qs.bsc", "-o", out + ".bad.fq"],
                [t["restore"], "-d", out + ".fq.dna", "-q", out + ".synth_fix.qs.bsc", "-o", out + ".bad.fq"]):
        r = _run(bad)
        assert r.returncode == 1 and b"bfq_restore:" in r.stdout, r.stdout
        assert os.path.exists(out + ".bad.fq") and os.path.getsize(out + ".bad.fq") == 0
        os.remove(out + ".bad.fq")
    assert b"read 0" in _run([t["restore"], "-d", out + ".fq.dna.bsc", "-q", out + ".example.qs.bsc", "-o", out + ".bad.fq"]).stdout
