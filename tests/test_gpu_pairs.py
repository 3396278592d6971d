"""GPU tests of the interleaved paired FASTQ calls (bfq_fastq_deinterleave* / bfq_fastq_interleave*, k_pairs.hip): the host,
device and file forms and the measuring form give the bytes, the statistics and the messages of the host form and of the
model (tests/pairs_model.py; tests/test_pairs_host.py holds the host form against it) over the model's cases, in both
directions and both modes, into guarded buffers; every refusal writes nothing and leaves the engine usable; the same on a
poisoned workspace in a child process; the tool and the multi-GPU driver.  Every refusal input has passed the host program
under sanitizers first (test_pairs_program_under_sanitizers): they test refusal, none is meant to fault."""
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import pairs_model as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
GUARD = 4096
host = api.HostText


def on_device(data, align=0):
    """(the tensor that holds it, the device address of the data `align` bytes past an aligned one)"""
    import torch
    t = torch.from_numpy(np.frombuffer(b"\0" * (16 + align) + bytes(data), np.uint8).copy()).cuda()
    return t, t.data_ptr() + 16 + align


def split_device(engine, text, lens, align=0, short=None, **opts):
    """the device form of the split: the text in a torch buffer, the three texts into guarded ones of exactly lens[k] bytes
    (short = k: one byte less for output k)"""
    import torch
    hold, addr = on_device(text, align)
    caps = [n - (k == short) for k, n in enumerate(lens)]
    outs = [torch.full((c + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
    try:
        ol, nr, st = engine.fastq_deinterleave_device(addr, len(text), [o.data_ptr() + GUARD for o in outs], caps, **opts)
    except api.BfqError:
        assert all(bool((o == 0xA5).all()) for o in outs), "a refusal wrote into an output buffer"
        raise
    got = []
    for o, n in zip(outs, ol):
        h = o.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
        got.append(h[GUARD:GUARD + n].tobytes())
    return got, nr, st


def merge_device(engine, texts, cap, align=0, **opts):
    import torch
    texts = list(texts) + [None] * (3 - len(texts))
    held = [None if t is None else on_device(t, align) for t in texts]
    out = torch.full((cap + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    try:
        n, st = engine.fastq_interleave_device([None if h is None else h[1] for h in held], [0 if t is None else len(t) for t in texts],
                                               out.data_ptr() + GUARD, cap, **opts)
    except api.BfqError:
        assert bool((out == 0xA5).all()), "a refusal wrote into the output buffer"
        raise
    h = out.cpu().numpy()
    assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
    return h[GUARD:GUARD + n].tobytes(), st


def put(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def check_split(engine, tmp_path, name, aligns=(0, 5)):
    """every form of the split on one case against the model"""
    text, opts = P.split_cases()[name]
    want, wst = P.expect_split(name)
    n_reads = [wst["singles"], wst["pairs"], wst["pairs"]]
    ol, nr, st = engine.fastq_deinterleave_measure(text, **opts)
    assert ol == wst["out_len"] and nr == n_reads and st.as_dict() == wst, name
    bufs = [np.full(len(w) + 2 * GUARD, 0xA5, np.uint8) for w in want]       # host buffers of the exact size, guarded
    got, st = engine.fastq_deinterleave(text, outs=[b[GUARD:GUARD + len(w)] for b, w in zip(bufs, want)], **opts)
    assert [g.tobytes() for g in got] == want and st.as_dict() == wst and st.n_reads == n_reads, name
    assert all((b[:GUARD] == 0xA5).all() and (b[GUARD + len(w):] == 0xA5).all() for b, w in zip(bufs, want)), name
    for align in aligns:
        got, nr, st = split_device(engine, text, wst["out_len"], align=align, **opts)
        assert got == want and nr == n_reads and st.as_dict() == wst, (name, align)
    dsts = [str(tmp_path / ("o%d.fq" % k)) for k in range(3)]
    ol, nr, st = engine.fastq_deinterleave_files(put(tmp_path, "in.fq", text), dsts, **opts)
    assert [open(d, "rb").read() for d in dsts] == want and ol == wst["out_len"] and nr == n_reads and st.as_dict() == wst, name


def check_merge(engine, tmp_path, name, aligns=(0, 3)):
    texts, opts = P.merge_cases()[name]
    want, wst = P.expect_merge(name)
    n, nr, st = engine.fastq_interleave_measure(texts, **opts)
    assert n == len(want) and nr == [wst["singles"], wst["pairs"], wst["pairs"]] and st.as_dict() == wst, name
    buf = np.full(len(want) + 2 * GUARD, 0xA5, np.uint8)
    got, st = engine.fastq_interleave(texts, out=buf[GUARD:GUARD + len(want)], **opts)
    assert got.tobytes() == want and st.as_dict() == wst and (buf[:GUARD] == 0xA5).all() and (buf[GUARD + len(want):] == 0xA5).all(), name
    for align in aligns:
        got, st = merge_device(engine, texts, len(want), align=align, **opts)
        assert got == want and st.as_dict() == wst, (name, align)
    paths = [None if t is None else put(tmp_path, "t%d.fq" % k, t) for k, t in enumerate(texts)]
    n, st = engine.fastq_interleave_files(paths, str(tmp_path / "m.fq"), **opts)
    assert open(str(tmp_path / "m.fq"), "rb").read() == want and n == len(want) and st.as_dict() == wst, name


@pytest.mark.parametrize("name", P.SPLIT_NAMES)
def test_split_forms_equal_the_model(engine, tmp_path, name):
    check_split(engine, tmp_path, name, aligns=(0, 5) if name in P.SMALL_SPLIT else (0,))
    want, wst = P.expect_split(name)
    got, st = host.fastq_deinterleave_host(*P.split_cases()[name][:1], **P.split_cases()[name][1])
    assert [g.tobytes() for g in got] == want and st.as_dict() == wst          # ... and the host form


@pytest.mark.parametrize("name", P.MERGE_NAMES)
def test_merge_forms_equal_the_model(engine, tmp_path, name):
    check_merge(engine, tmp_path, name, aligns=(0, 3) if name != "wide" else (0,))
    texts, opts = P.merge_cases()[name]
    got, st = host.fastq_interleave_host(texts, **opts)
    assert got.tobytes() == P.expect_merge(name)[0] and st.as_dict() == P.expect_merge(name)[1]


def test_text_sized_by_the_call(engine):
    text, opts = P.split_cases()["edges-orphans"]
    got, st = engine.fastq_deinterleave(text, **opts)
    assert [g.tobytes() for g in got] == P.expect_split("edges-orphans")[0]
    texts, opts = P.merge_cases()["with-singles-nolf"]
    assert engine.fastq_interleave(texts, **opts)[0].tobytes() == P.expect_merge("with-singles-nolf")[0]


def test_refusals(engine, tmp_path):
    good, gopts = P.split_cases()["orphans-singles-first"]
    gwant, gst = P.expect_split("orphans-singles-first")
    for name, (text, opts, code, msg) in P.split_refusals().items():
        with pytest.raises(api.BfqError) as h:
            host.fastq_deinterleave_host(text, **opts)
        assert (h.value.code, str(h.value).split(": ", 1)[1]) == (code, msg), name
        cap = len(text) + 1
        buf = np.full(3 * cap, 0xA5, np.uint8)
        with pytest.raises(api.BfqError) as e:
            engine.fastq_deinterleave(text, outs=[buf[k * cap:(k + 1) * cap] for k in range(3)], **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and e.value.needed == [0, 0, 0], (name, str(e.value), msg)
        assert (buf == 0xA5).all(), name
        with pytest.raises(api.BfqError) as e:
            split_device(engine, text, [cap] * 3, align=3, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.fastq_deinterleave_measure(text, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        dsts = [str(tmp_path / ("r%d.fq" % k)) for k in range(3)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_deinterleave_files(put(tmp_path, "bad.fq", text), dsts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and [os.path.getsize(d) for d in dsts] == [0, 0, 0], (name, str(e.value))
        got, nr, st = split_device(engine, good, gst["out_len"], **gopts)       # the same Engine is usable afterwards
        assert got == gwant and st.as_dict() == gst, name
    mgood, mopts = P.merge_cases()["with-singles"]
    mwant, mst = P.expect_merge("with-singles")
    for name, (texts, opts, code, msg) in P.merge_refusals().items():
        with pytest.raises(api.BfqError) as h:
            host.fastq_interleave_host(texts, **opts)
        assert (h.value.code, str(h.value).split(": ", 1)[1]) == (code, msg), name
        cap = sum(len(t) + 1 for t in texts if t is not None)
        buf = np.full(cap, 0xA5, np.uint8)
        with pytest.raises(api.BfqError) as e:
            engine.fastq_interleave(texts, out=buf, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and e.value.needed == 0 and (buf == 0xA5).all(), (name, str(e.value), msg)
        with pytest.raises(api.BfqError) as e:
            merge_device(engine, texts, cap, align=1, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.fastq_interleave_measure(texts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        paths = [None if t is None else put(tmp_path, "b%d.fq" % k, t) for k, t in enumerate(texts)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_interleave_files(paths, str(tmp_path / "bm.fq"), **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and os.path.getsize(str(tmp_path / "bm.fq")) == 0, (name, str(e.value))
        got, st = merge_device(engine, mgood, len(mwant), **mopts)
        assert got == mwant and st.as_dict() == mst, name


def test_registered_outputs_of_a_refused_split_end_empty(engine, tmp_path):
    """outputs a tool registered (bfq_output_prefault) before a call that is refused before their lengths are known: the
    mappings go with the call, the files end empty and not at the registered 8192 bytes; registered again, a good call
    picks the mappings up and cuts the files to their lengths"""
    import ctypes as C
    from bfqzip_amd import _lib
    L = _lib.lib()
    recs = [P.rec(b"@r%d/%d" % (k // 2, k % 2 + 1), b"ACGT"[:k % 3 + 2]) for k in range(4)]
    fds = [os.open(str(tmp_path / ("g%d.fq" % k)), os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o644) for k in range(3)]
    try:
        def call(text):
            for fd in fds:
                assert L.bfq_output_prefault(fd, 8192, 4096) == 0 and os.fstat(fd).st_size == 8192
            src = os.open(put(tmp_path, "gin.fq", text), os.O_RDONLY)
            try:
                O, st, ol, nr = api.pairs_opts(), _lib.PairsStats(), (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
                rc = L.bfq_fastq_deinterleave_fd(engine.h, src, len(text), C.byref(O), (C.c_int * 3)(*fds), ol, nr, C.byref(st))
            finally:
                os.close(src)
            return rc, [os.pread(fd, 8192, 0) for fd in fds]
        with pytest.raises(P.Refused) as want:
            P.split(b"".join(recs[:3]))
        rc, got = call(b"".join(recs[:3]))
        assert rc == want.value.code and L.bfq_last_error(engine.h).decode().endswith(want.value.msg) and "odd" in want.value.msg
        assert got == [b"", b"", b""]
        rc, got = call(b"".join(recs))
        assert rc == 0 and got == P.split(b"".join(recs))[0] == [b"", recs[0] + recs[2], recs[1] + recs[3]]
    finally:
        for fd in fds:
            os.close(fd)


@pytest.mark.parametrize("name", ("lanes", "orphans-singles-first"))
def test_capacity_one_byte_short(engine, name):
    text, opts = P.split_cases()[name]
    want, wst = P.expect_split(name)
    for short in range(3):
        if not wst["out_len"][short]:
            continue
        bufs = [np.full(n - (k == short), 0xA5, np.uint8) for k, n in enumerate(wst["out_len"])]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_deinterleave(text, outs=bufs, **opts)
        assert e.value.code == -1 and e.value.needed == wst["out_len"] and all((b == 0xA5).all() for b in bufs), (name, short)
        with pytest.raises(api.BfqError) as e:
            split_device(engine, text, wst["out_len"], short=short, **opts)
        assert e.value.code == -1 and e.value.needed == wst["out_len"], (name, short)
    texts, mo = P.merge_cases()["with-singles"]
    mw, _ = P.expect_merge("with-singles")
    buf = np.full(len(mw) - 1, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        engine.fastq_interleave(texts, out=buf, **mo)
    assert e.value.code == -1 and e.value.needed == len(mw) and (buf == 0xA5).all()
    with pytest.raises(api.BfqError) as e:
        merge_device(engine, texts, len(mw) - 1, **mo)
    assert e.value.code == -1 and e.value.needed == len(mw)
    assert merge_device(engine, texts, len(mw), **mo)[0] == mw


def test_workspace_cap_too_small():
    e = api.Engine(0, ws_cap_mib=2)
    try:
        text, opts = P.split_cases()["wide"]
        with pytest.raises(api.BfqError) as x:
            e.fastq_deinterleave(text, **opts)
        assert x.value.code == P.E_NOMEM and "GiB of device memory" in str(x.value)
        texts, opts = P.merge_cases()["wide"]
        with pytest.raises(api.BfqError) as x:
            e.fastq_interleave(texts, **opts)
        assert x.value.code == P.E_NOMEM and "GiB of device memory" in str(x.value)
        e.set_params(ws_cap_mib=0)                                  # the context stays usable
        got, st = e.fastq_deinterleave(*P.split_cases()["edges"][:1])
        assert [g.tobytes() for g in got] == P.expect_split("edges")[0]
    finally:
        e.close()


def test_compressed_text_is_refused(engine):
    import gzip
    z = gzip.compress(P.split_cases()["one-pair"][0])
    with pytest.raises(api.BfqError) as e:
        engine.fastq_deinterleave(z, outs=[np.empty(1000, np.uint8)] * 3)
    assert e.value.code == -1 and "inflate the text first" in str(e.value)
    with pytest.raises(api.BfqError) as e:
        split_device(engine, z, [1000] * 3)
    assert e.value.code == -1 and "inflate the text first" in str(e.value)
    with pytest.raises(api.BfqError) as e:
        engine.fastq_interleave([None, z, z], out=np.empty(1000, np.uint8))
    assert e.value.code == -1 and "text 1 is compressed" in str(e.value) and "inflate the text first" in str(e.value)


CHILD = """
import sys, pathlib
sys.path.insert(0, %r)
from bfqzip_amd import api
from tests import pairs_model as P
from tests import test_gpu_pairs as T
assert api._lib.os.environ["BFQ_POISON"] == "0x41"
e = api.Engine(0)
tmp = pathlib.Path(sys.argv[1])
for name in ("lanes", "lanes-orphans", "orphans-runs", "orphans-singles-first", "orphans-empty-keys", "wide", "wide-orphans"):
    T.check_split(e, tmp, name, aligns=(0,))
for name in ("lanes", "with-singles", "lanes-with-singles", "wide"):
    T.check_merge(e, tmp, name, aligns=(0,))
e.close()
print("poisoned pairs ok")
"""


def test_forms_on_a_poisoned_workspace(tmp_path):
    """the three forms on lanes, orphans and wide in a fresh process whose arena and text buffer hold 0x41 before every call"""
    script = put(tmp_path, "child.py", (CHILD % ROOT).encode())
    r = subprocess.run([sys.executable, script, str(tmp_path)], env=dict(os.environ, BFQ_POISON="0x41"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    assert r.returncode == 0 and b"poisoned pairs ok" in r.stdout, r.stdout.decode()[-4000:]


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _golden_pair(tmp_path):
    """(the paths of the two mates of the paired golden input, their texts, the model's interleaved text)"""
    from tests.test_parallel_gloo import paired_inputs
    f1, f2 = paired_inputs(str(tmp_path))
    a, b = open(f1, "rb").read(), open(f2, "rb").read()
    return (f1, f2), (a, b), P.merge([None, a, b])[0]


def test_tool(engine, tmp_path):
    import gzip
    tool = os.path.join(DROP, "bfq_pairs")
    path = lambda n: str(tmp_path / n)
    (f1, f2), (a, b), both = _golden_pair(tmp_path)
    il = put(tmp_path, "il.fq", both)
    r = _run([tool, "-s", il, "-1", path("a.fq"), "-2", path("b.fq")])          # the round trip
    assert r.returncode == 0 and b"200 records: 100 pairs, 0 singles" in r.stdout, (r.stdout, r.stderr)
    assert (open(path("a.fq"), "rb").read(), open(path("b.fq"), "rb").read()) == (a, b)
    r = _run([tool, "-m", "-1", path("a.fq"), "-2", path("b.fq"), "-o", path("back.fq")])
    assert r.returncode == 0 and open(path("back.fq"), "rb").read() == both and b"100 pairs" in r.stdout, (r.stdout, r.stderr)
    r = _run([tool, "-t", il])
    assert r.returncode == 0 and b"200 records: 100 pairs, 0 singles" in r.stdout, (r.stdout, r.stderr)
    # compressed inputs are inflated first: BGZF, and plain gzip with -g
    put(tmp_path, "il.fq.gz", engine.bgzf_deflate(both).tobytes())
    r = _run([tool, "-s", path("il.fq.gz"), "-1", path("za.fq"), "-2", path("zb.fq")])
    assert r.returncode == 0 and (open(path("za.fq"), "rb").read(), open(path("zb.fq"), "rb").read()) == (a, b), (r.stdout, r.stderr)
    put(tmp_path, "a.gz", gzip.compress(a))
    r = _run([tool, "-g", "-m", "-1", path("a.gz"), "-2", f2, "-o", path("zback.fq")])
    assert r.returncode == 0 and open(path("zback.fq"), "rb").read() == both, (r.stdout, r.stderr)
    # orphan mode, with and without -0; a merge with singles behind the pairs
    text, _ = P.split_cases()["orphans-singles-first"]
    want, wst = P.expect_split("orphans-singles-first")
    r = _run([tool, "-s", put(tmp_path, "o.fq", text), "-O", "-0", path("s0.fq"), "-1", path("s1.fq"), "-2", path("s2.fq")])
    assert r.returncode == 0 and [open(path("s%d.fq" % k), "rb").read() for k in range(3)] == want, (r.stdout, r.stderr)
    assert ("%d records: %d pairs, %d singles" % (wst["records"], wst["pairs"], wst["singles"])).encode() in r.stdout
    r = _run([tool, "-t", path("o.fq"), "-O"])
    assert r.returncode == 0 and ("%d pairs, %d singles" % (wst["pairs"], wst["singles"])).encode() in r.stdout
    r = _run([tool, "-m", "-0", path("s0.fq"), "-1", path("s1.fq"), "-2", path("s2.fq"), "-o", path("sm.fq")])
    assert r.returncode == 0 and open(path("sm.fq"), "rb").read() == P.merge(want)[0], (r.stdout, r.stderr)
    # refusals: exit status 1, the library's message, empty outputs
    btext, _, _, msg = P.split_refusals()["middle"]
    bad = put(tmp_path, "bad.fq", btext)
    r = _run([tool, "-s", bad, "-1", path("x1.fq"), "-2", path("x2.fq")])
    assert r.returncode == 1 and msg.encode() in r.stderr and os.path.getsize(path("x1.fq")) == os.path.getsize(path("x2.fq")) == 0, r.stderr
    r = _run([tool, "-t", bad])
    assert r.returncode == 1 and msg.encode() in r.stderr
    assert _run([tool, "-t", bad, "-n"]).returncode == 0 and _run([tool, "-t", path("o.fq")]).returncode == 1
    mtexts, _, _, msg = P.merge_refusals()["counts"]
    r = _run([tool, "-m", "-1", put(tmp_path, "m1.fq", mtexts[1]), "-2", put(tmp_path, "m2.fq", mtexts[2]), "-o", path("xm.fq")])
    assert r.returncode == 1 and msg.encode() in r.stderr and os.path.getsize(path("xm.fq")) == 0, r.stderr
    for args in (["-s", il], ["-s", il, "-1", path("u.fq")], ["-m", "-1", f1, "-2", f2], ["-t", il, "-1", path("u.fq")], ["-s", il, "-m"],
                 ["-m", "-O", "-1", f1, "-2", f2, "-o", path("u.fq")]):
        assert _run([tool] + args).returncode == 1, args


def test_parallel_interleaved(engine, tmp_path):
    for d in "ab":
        os.mkdir(str(tmp_path / d))
    out = lambda d, n: str(tmp_path / d / n)
    (f1, f2), (a, b), both = _golden_pair(tmp_path)
    il = put(tmp_path, "il.fq", both)
    assert parallel.main([f1, f2, "-p", "-o", out("a", "OUT"), "-t", "2", "-0", "-H"]) == 0
    assert parallel.main([il, "--interleaved", "-o", out("b", "OUT"), "-t", "2", "-0", "-H", "--interleaved-out", out("b", "il.fq")]) == 0
    want = [open(out("a", "OUT_%d.fastq" % k), "rb").read() for k in (1, 2)]
    assert [open(out("b", "OUT_%d.fastq" % k), "rb").read() for k in (1, 2)] == want
    assert open(out("b", "il.fq"), "rb").read() == P.merge([None] + want)[0]
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["OUT_1.fastq", "OUT_2.fastq", "il.fq"]       # the intermediates are gone
    bad = put(tmp_path, "bad.fq", P.split_refusals()["middle"][0])
    assert parallel.main([bad, "--interleaved", "-o", out("b", "BAD"), "-t", "2", "-0"]) == 1
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["OUT_1.fastq", "OUT_2.fastq", "il.fq"]
