"""GPU tests of the repair of paired FASTQ (bfq_fastq_repair*, the repair section of k_pairs.hip): the measuring form, the
host, device and file forms give the bytes, the statistics and the messages of the host form and of the model
(tests/pairs_repair_model.py; tests/test_pairs_repair_host.py holds the host form against it) over the model's cases, into
guarded buffers; every refusal writes nothing and leaves the engine usable; the small cases again on a poisoned workspace
in a child process.  Every refusal input has passed the host program under sanitizers first
(test_repair_program_under_sanitizers): they test refusal, none is meant to fault."""
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import api
from tests import pairs_repair_model as R
from tests.test_gpu_pairs import on_device, put, GUARD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


def repair_device(engine, texts, lens, align=0, short=None, **opts):
    """the device form: the texts in torch buffers `align` bytes past an aligned address, the three outputs into guarded ones
    of exactly lens[k] bytes (short = k: one byte less for output k)"""
    import torch
    texts = list(texts) + [None] * (3 - len(texts))
    held = [None if t is None else on_device(t, align) for t in texts]
    caps = [n - (k == short) for k, n in enumerate(lens)]
    outs = [torch.full((c + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
    try:
        ol, nr, st = engine.fastq_repair_device([None if h is None else h[1] for h in held], [0 if t is None else len(t) for t in texts],
                                                [o.data_ptr() + GUARD for o in outs], caps, **opts)
    except api.BfqError:
        assert all(bool((o == 0xA5).all()) for o in outs), "a refusal wrote into an output buffer"
        raise
    got = []
    for o, n in zip(outs, ol):
        h = o.cpu().numpy()
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
        got.append(h[GUARD:GUARD + n].tobytes())
    return got, nr, st


def check_repair(engine, tmp_path, name, aligns=(0, 5)):
    """every form of the repair on one case against the model"""
    texts, opts = R.all_cases()[name]
    want, wst = R.expect(name)
    n_reads = [wst["singles"], wst["pairs"], wst["pairs"]]
    ol, nr, st = engine.fastq_repair_measure(texts, **opts)
    assert ol == wst["out_len"] and nr == n_reads and st.as_dict() == wst, (name, st, wst)
    bufs = [np.full(len(w) + 2 * GUARD, 0xA5, np.uint8) for w in want]       # host buffers of the exact size, guarded
    got, st = engine.fastq_repair(texts, outs=[b[GUARD:GUARD + len(w)] for b, w in zip(bufs, want)], **opts)
    assert [g.tobytes() for g in got] == want and st.as_dict() == wst and st.n_reads == n_reads, name
    assert all((b[:GUARD] == 0xA5).all() and (b[GUARD + len(w):] == 0xA5).all() for b, w in zip(bufs, want)), name
    for align in aligns:
        got, nr, st = repair_device(engine, texts, wst["out_len"], align=align, **opts)
        assert got == want and nr == n_reads and st.as_dict() == wst, (name, align)
    paths = [None if t is None else put(tmp_path, "t%d.fq" % k, t) for k, t in enumerate(texts)]
    dsts = [str(tmp_path / ("o%d.fq" % k)) for k in range(3)]
    ol, nr, st = engine.fastq_repair_files(paths, dsts, **opts)
    assert [open(d, "rb").read() for d in dsts] == want and ol == wst["out_len"] and nr == n_reads and st.as_dict() == wst, name


@pytest.mark.parametrize("name", R.NAMES)
def test_repair_forms_equal_the_model(engine, tmp_path, name):
    check_repair(engine, tmp_path, name, aligns=(0, 5) if name not in R.LARGE else (0,))
    texts, opts = R.all_cases()[name]
    got, st = host.fastq_repair_host(texts, **opts)
    assert [g.tobytes() for g in got] == R.expect(name)[0] and st.as_dict() == R.expect(name)[1]      # ... and the host form


def test_text_sized_by_the_call(engine):
    texts, opts = R.cases()["all-three"]
    got, st = engine.fastq_repair(texts, **opts)
    assert [g.tobytes() for g in got] == R.expect("all-three")[0]


def test_refusals(engine, tmp_path):
    good, gopts = R.cases()["all-three"]
    gwant, gst = R.expect("all-three")
    for name, (texts, opts, code, msg) in R.refusals().items():
        with pytest.raises(api.BfqError) as h:
            host.fastq_repair_host(texts, **opts)
        assert (h.value.code, str(h.value).split(": ", 1)[1]) == (code, msg), name
        cap = sum(len(t) + 1 for t in texts if t is not None)
        buf = np.full(3 * cap, 0xA5, np.uint8)
        with pytest.raises(api.BfqError) as e:
            engine.fastq_repair(texts, outs=[buf[k * cap:(k + 1) * cap] for k in range(3)], **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and e.value.needed == [0, 0, 0], (name, str(e.value), msg)
        assert (buf == 0xA5).all(), name
        with pytest.raises(api.BfqError) as e:
            repair_device(engine, texts, [cap] * 3, align=3, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.fastq_repair_measure(texts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        paths = [None if t is None else put(tmp_path, "b%d.fq" % k, t) for k, t in enumerate(texts)]
        dsts = [str(tmp_path / ("r%d.fq" % k)) for k in range(3)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_repair_files(paths, dsts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and [os.path.getsize(d) for d in dsts] == [0, 0, 0], (name, str(e.value))
        got, nr, st = repair_device(engine, good, gst["out_len"], **gopts)       # the same Engine is usable afterwards
        assert got == gwant and st.as_dict() == gst, name


@pytest.mark.parametrize("name", ("filtered-300", "all-three"))
def test_capacity_one_byte_short(engine, name):
    texts, opts = R.cases()[name]
    want, wst = R.expect(name)
    for short in range(3):
        assert wst["out_len"][short]
        bufs = [np.full(n - (k == short), 0xA5, np.uint8) for k, n in enumerate(wst["out_len"])]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_repair(texts, outs=bufs, **opts)
        assert e.value.code == -1 and e.value.needed == wst["out_len"] and all((b == 0xA5).all() for b in bufs), (name, short)
        with pytest.raises(api.BfqError) as e:
            repair_device(engine, texts, wst["out_len"], short=short, **opts)
        assert e.value.code == -1 and e.value.needed == wst["out_len"], (name, short)
    assert repair_device(engine, texts, wst["out_len"], **opts)[0] == want


def test_workspace_cap_too_small():
    e = api.Engine(0, ws_cap_mib=2)
    try:
        texts, opts = R.cases()["wide"]
        with pytest.raises(api.BfqError) as x:
            e.fastq_repair(texts, **opts)
        assert x.value.code == R.P.E_NOMEM and "GiB of device memory" in str(x.value)
        e.set_params(ws_cap_mib=0)                                  # the context stays usable
        got, st = e.fastq_repair(R.cases()["filtered-65"][0])
        assert [g.tobytes() for g in got] == R.expect("filtered-65")[0]
    finally:
        e.close()


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_tool(engine, tmp_path):
    import gzip
    tool = os.path.join(ROOT, "dropin", "bfq_pairs")
    path = lambda n: str(tmp_path / n)
    (_, t1, t2), _ = R.cases()["filtered-300"]
    want, wst = R.expect("filtered-300")
    f1, f2 = put(tmp_path, "r1.fq", t1), put(tmp_path, "r2.fq", t2)
    counts = ("%d records: %d pairs, %d singles" % (wst["records"], wst["pairs"], wst["singles"])).encode()
    r = _run([tool, "-r", "-1", f1, "-2", f2, "-A", path("a.fq"), "-B", path("b.fq"), "-S", path("s.fq")])
    assert r.returncode == 0 and counts in r.stdout, (r.stdout, r.stderr)
    assert [open(path(n), "rb").read() for n in ("s.fq", "a.fq", "b.fq")] == want
    r = _run([tool, "-r", "-t", "-1", f1, "-2", f2])               # count only: status 1, there are singletons
    assert r.returncode == 1 and counts in r.stdout, (r.stdout, r.stderr)
    # singletons without -S: refused before anything is written
    r = _run([tool, "-r", "-1", f1, "-2", f2, "-A", path("x1.fq"), "-B", path("x2.fq")])
    assert r.returncode == 1 and ("FASTQ repair: %d singletons and no -S file" % wst["singles"]).encode() in r.stderr, r.stderr
    assert not os.path.exists(path("x1.fq")) and not os.path.exists(path("x2.fq"))
    # the repaired mates are proper: nothing left over, -S not needed, and -r -t exits with 0
    r = _run([tool, "-r", "-1", path("a.fq"), "-2", path("b.fq"), "-A", path("a2.fq"), "-B", path("b2.fq")])
    assert r.returncode == 0 and [open(path(n), "rb").read() for n in ("a2.fq", "b2.fq")] == want[1:], (r.stdout, r.stderr)
    assert _run([tool, "-r", "-t", "-1", path("a.fq"), "-2", path("b.fq")]).returncode == 0
    # one mixed file, plain gzip, inflated first; -k keeps the suffixes in the names
    (m0, _, _), _ = R.cases()["mixed-suffix"]
    mwant, mst = R.expect("mixed-suffix")
    put(tmp_path, "m.fq.gz", gzip.compress(m0))
    r = _run([tool, "-r", "-g", "-0", path("m.fq.gz"), "-A", path("ma.fq"), "-B", path("mb.fq"), "-S", path("ms.fq")])
    assert r.returncode == 0 and [open(path(n), "rb").read() for n in ("ms.fq", "ma.fq", "mb.fq")] == mwant, (r.stdout, r.stderr)
    r = _run([tool, "-r", "-k", "-t", "-0", put(tmp_path, "m.fq", m0)])
    kst = R.expect("mixed-suffix-kept")[1]
    assert r.returncode == 1 and ("%d pairs, %d singles" % (kst["pairs"], kst["singles"])).encode() in r.stdout, (r.stdout, r.stderr)
    # a refusal: exit status 1, the library's message, empty outputs
    btexts, _, _, msg = R.refusals()["1025-equal"]
    r = _run([tool, "-r", "-0", put(tmp_path, "bad.fq", btexts[0]), "-A", path("y1.fq"), "-B", path("y2.fq"), "-S", path("y0.fq")])
    assert r.returncode == 1 and msg.encode() in r.stderr and all(os.path.getsize(path(n)) == 0 for n in ("y0.fq", "y1.fq", "y2.fq")), r.stderr
    for args in (["-r"], ["-r", "-1", f1, "-2", f2], ["-r", "-1", f1, "-A", path("u.fq")], ["-r", "-t", "-1", f1, "-A", path("u.fq")], ["-r", "-A", path("u.fq"), "-B", path("v.fq")]):
        assert _run([tool] + args).returncode == 1, args


def test_parallel_repair(engine, tmp_path):
    from bfqzip_amd import parallel
    from tests.test_pairs_repair_host import filtered_golden
    for d in "ab":
        os.mkdir(str(tmp_path / d))
    out = lambda d, n: str(tmp_path / d / n)
    (g1, g2), want = filtered_golden(str(tmp_path))
    assert parallel.main([g1, g2, "-p", "--repair", "-o", out("a", "OUT"), "-t", "2", "-0", "-H", "--keep-inflated"]) == 0
    mids = [out("a", "thin_R1_1.fastq"), out("a", "thin_R1_2.fastq")]
    assert [open(m, "rb").read() for m in mids] == want[1:]         # the run's inputs are the repaired files ...
    assert open(out("a", "thin_R1_singles.fastq"), "rb").read() == want[0]      # ... and the singles file is the model's
    assert parallel.main(mids + ["-p", "-o", out("b", "OUT"), "-t", "2", "-0", "-H"]) == 0
    assert [open(out("a", "OUT_%d.fastq" % k), "rb").read() for k in (1, 2)] == [open(out("b", "OUT_%d.fastq" % k), "rb").read() for k in (1, 2)]
    bad = put(tmp_path, "bad.fq", R.refusals()["1025-equal"][0][0])
    assert parallel.main([bad, "--repair", "-o", out("b", "BAD"), "-t", "2", "-0"]) == 1
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["OUT_1.fastq", "OUT_2.fastq"]


CHILD = """
import sys, pathlib
sys.path.insert(0, %r)
from bfqzip_amd import api
from tests import pairs_repair_model as R
from tests import test_gpu_pairs_repair as T
assert api._lib.os.environ["BFQ_POISON"] == "0x41"
e = api.Engine(0)
tmp = pathlib.Path(sys.argv[1])
for name in R.SMALL_NAMES + ("bound-1024",):
    T.check_repair(e, tmp, name, aligns=(0,))
e.close()
print("poisoned repair ok")
"""


def test_forms_on_a_poisoned_workspace(tmp_path):
    """the forms on the small cases in a fresh process whose arena and text buffer hold 0x41 before every call"""
    script = put(tmp_path, "child.py", (CHILD % ROOT).encode())
    r = subprocess.run([sys.executable, script, str(tmp_path)], env=dict(os.environ, BFQ_POISON="0x41"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    assert r.returncode == 0 and b"poisoned repair ok" in r.stdout, r.stdout.decode()[-4000:]
