"""GPU tests of the exact duplicate removal (bfq_fastq_dedup*, k_dedup.hip): the measuring, host, device and file forms give the
bytes, every statistic and the messages of the model (tests/dedup_model.py) and of the host form (tests/test_dedup_host.py
holds that against the model) over the model's cases, into guarded buffers; every refusal writes nothing and leaves the engine
usable; all of it once more on a poisoned workspace in child processes; the tool and the multi-GPU driver.  The refusal inputs
are those of the host program under sanitizers (test_dedup_program_under_sanitizers)."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import dedup_model as M

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


def dedup_device(engine, texts, lens, align=0, short=None, dups=True, **opts):
    """the device form: the texts in torch buffers, the four outputs into guarded ones of exactly lens[k] bytes (short = k: one
    byte less for output k); dups=False: the removed records are not written"""
    import torch
    held = [None if t is None else on_device(t, align) for t in texts]
    caps = [n - (k == short) for k, n in enumerate(lens)]
    outs = [torch.full((c + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for c in caps]
    ptr = [o.data_ptr() + GUARD for o in outs]
    try:
        ol, dl, st = engine.fastq_dedup_device([None if h is None else h[1] for h in held], [0 if t is None else len(t) for t in texts], ptr[:2], caps[:2],
                                               ptr[2:] if dups else None, caps[2:] if dups else None, **opts)
    except api.BfqError:
        assert all(bool((o == 0xA5).all()) for o in outs), "a refusal wrote into an output buffer"
        raise
    got = []
    for k, (o, n) in enumerate(zip(outs, ol + dl)):
        h = o.cpu().numpy()
        if k >= 2 and not dups:
            assert (h == 0xA5).all()
            n = 0
        assert (h[:GUARD] == 0xA5).all() and (h[GUARD + n:] == 0xA5).all()
        got.append(h[GUARD:GUARD + n].tobytes())
    return got, ol, dl, st


def put(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def check(engine, tmp_path, name, aligns=(0, 5)):
    """every form on one case against the model"""
    texts, opts = M.all_cases()[name]
    kept, removed, wst = M.expect(name)
    want, lens = kept + removed, [len(w) for w in kept + removed]
    ol, dl, st = engine.fastq_dedup_measure(texts, **opts)
    assert ol + dl == lens and st.as_dict() == wst, name
    bufs = [np.full(n + 2 * GUARD, 0xA5, np.uint8) for n in lens]              # host buffers of the exact size, guarded
    wins = [b[GUARD:GUARD + n] for b, n in zip(bufs, lens)]
    outs, dups, st = engine.fastq_dedup(texts, outs=wins[:2], dups=wins[2:], **opts)
    assert [o.tobytes() for o in outs] + [d.tobytes() for d in dups] == want and st.as_dict() == wst, name
    assert all((b[:GUARD] == 0xA5).all() and (b[GUARD + n:] == 0xA5).all() for b, n in zip(bufs, lens)), name
    for align in aligns:
        got, ol, dl, st = dedup_device(engine, texts, lens, align=align, **opts)
        assert got == want and ol + dl == lens and st.as_dict() == wst, (name, align)
    got, ol, dl, st = dedup_device(engine, texts, lens, dups=False, **opts)   # the removed records counted, not written
    assert got[:2] == kept and ol + dl == lens and st.as_dict() == wst, name
    paths = [None if t is None else put(tmp_path, "t%d.fq" % k, t) for k, t in enumerate(texts)]
    dsts = [str(tmp_path / ("o%d.fq" % k)) for k in range(4)]
    if texts[1] is None:
        dsts[1] = dsts[3] = None
    ol, dl, st = engine.fastq_dedup_files(paths, dsts[:2], dsts[2:], **opts)
    assert [open(d, "rb").read() if d else b"" for d in dsts] == want and ol + dl == lens and st.as_dict() == wst, name


@pytest.mark.parametrize("name", M.NAMES)
def test_forms_equal_the_model(engine, tmp_path, name):
    check(engine, tmp_path, name, aligns=(0, 5) if name in M.SMALL_NAMES else (0,))
    texts, opts = M.all_cases()[name]
    outs, dups, st = host.fastq_dedup_host(texts, dups=True, **opts)           # ... and the host form
    assert ([o.tobytes() for o in outs], [d.tobytes() for d in dups], st.as_dict()) == M.expect(name)


def test_text_sized_by_the_call(engine):
    for name in ("lines-paired-nolf", "keep-middle"):
        texts, opts = M.all_cases()[name]
        outs, dups, st = engine.fastq_dedup(texts, dups=True, **opts)
        assert ([o.tobytes() for o in outs], [d.tobytes() for d in dups], st.as_dict()) == M.expect(name)
        outs, dups, st = engine.fastq_dedup(texts, **opts)
        assert [o.tobytes() for o in outs] == M.expect(name)[0] and dups is None


def refusals_hold(engine, tmp_path):
    """every refusal in every form: the model's message, nothing written, and a good call on the same Engine afterwards"""
    good, gopts = M.all_cases()["pairs-mix-best"]
    gk, gr, gst = M.expect("pairs-mix-best")
    glens = [len(w) for w in gk + gr]
    for name, (texts, opts, code, msg) in M.refusals().items():
        with pytest.raises(api.BfqError) as h:
            host.fastq_dedup_host(texts, **opts)
        assert (h.value.code, str(h.value).split(": ", 1)[1]) == (code, msg), name
        cap = max(len(t) + 1 for t in texts if t is not None)
        buf = np.full(4 * cap, 0xA5, np.uint8)
        wins = [buf[k * cap:(k + 1) * cap] for k in range(4)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_dedup(texts, outs=wins[:2], dups=wins[2:], **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and e.value.needed == [0, 0, 0, 0], (name, str(e.value), msg)
        assert (buf == 0xA5).all(), name
        with pytest.raises(api.BfqError) as e:
            dedup_device(engine, texts, [cap] * 4, align=3, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.fastq_dedup_measure(texts, **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg), (name, str(e.value))
        paths = [None if t is None else put(tmp_path, "b%d.fq" % k, t) for k, t in enumerate(texts)]
        dsts = [str(tmp_path / ("r%d.fq" % k)) for k in range(4)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_dedup_files(paths, dsts[:2], dsts[2:], **opts)
        assert e.value.code == code and str(e.value).endswith(": " + msg) and [os.path.getsize(d) for d in dsts] == [0, 0, 0, 0], (name, str(e.value))
        got, ol, dl, st = dedup_device(engine, good, glens, **gopts)           # the same Engine is usable afterwards
        assert got == gk + gr and st.as_dict() == gst, name


def test_refusals(engine, tmp_path):
    refusals_hold(engine, tmp_path)


SHORT = ("lengths", "pairs-mix", "keep-middle-paired", "collide-mate-2")


def short_caps_hold(engine, name):
    """each of the four outputs one byte short: refused with the lengths needed, nothing written; then the exact sizes"""
    texts, opts = M.all_cases()[name]
    kept, removed, wst = M.expect(name)
    lens = [len(w) for w in kept + removed]
    for short in range(4):
        if not lens[short]:
            continue
        bufs = [np.full(n - (k == short), 0xA5, np.uint8) for k, n in enumerate(lens)]
        with pytest.raises(api.BfqError) as e:
            engine.fastq_dedup(texts, outs=bufs[:2], dups=bufs[2:], **opts)
        assert e.value.code == -1 and e.value.needed == lens and all((b == 0xA5).all() for b in bufs), (name, short)
        with pytest.raises(api.BfqError) as e:
            dedup_device(engine, texts, lens, short=short, **opts)
        assert e.value.code == -1 and e.value.needed == lens, (name, short)
    got, ol, dl, st = dedup_device(engine, texts, lens, **opts)
    assert got == kept + removed and st.as_dict() == wst


@pytest.mark.parametrize("name", SHORT)
def test_capacity_one_byte_short(engine, name):
    short_caps_hold(engine, name)


def test_file_form_needs_a_place_for_the_kept_records(engine, tmp_path):
    (t1, t2), opts = M.all_cases()["pairs-mix"]
    kept, removed, wst = M.expect("pairs-mix")
    a, b = put(tmp_path, "a.fq", t1), put(tmp_path, "b.fq", t2)
    d = [str(tmp_path / ("w%d.fq" % k)) for k in range(4)]
    for outs in ([d[0], None], [None, d[1]], [None, None]):       # paired without a descriptor for a mate's kept records
        with pytest.raises(api.BfqError) as e:
            engine.fastq_dedup_files([a, b], outs, d[2:], **opts)
        assert e.value.code == -1 and "bad file descriptor" in str(e.value) and all(os.path.getsize(p) == 0 for p in d if os.path.exists(p)), outs
    with pytest.raises(api.BfqError) as e:
        engine.fastq_dedup_files([a, None], [None, None], None, **opts)
    assert e.value.code == -1 and "bad file descriptor" in str(e.value)
    ol, dl, st = engine.fastq_dedup_files([a, b], d[:2], [d[2], None], **opts)         # a removed text may go unwritten
    assert [open(p, "rb").read() for p in d[:3]] == kept + removed[:1] and os.path.getsize(d[3]) == 0 and st.as_dict() == wst


def test_workspace_cap_too_small():
    e = api.Engine(0, ws_cap_mib=2)
    try:
        texts, opts = M.all_cases()["wide"]
        with pytest.raises(api.BfqError) as x:
            e.fastq_dedup(texts, **opts)
        assert x.value.code == M.P.E_NOMEM and "removing duplicates needs" in str(x.value) and "GiB of device memory" in str(x.value)
        e.set_params(ws_cap_mib=0)                                  # the context stays usable
        outs, _, st = e.fastq_dedup(*M.all_cases()["lines"][:1])
        assert [o.tobytes() for o in outs] == M.expect("lines")[0]
    finally:
        e.close()


CHILD = """
import sys, pathlib
sys.path.insert(0, %r)
from bfqzip_amd import api
from tests import dedup_model as M
from tests import test_gpu_dedup as T
assert api._lib.os.environ["BFQ_POISON"] == "0x41"
e = api.Engine(0)
tmp = pathlib.Path(sys.argv[1])
T.POISONED[sys.argv[2]](e, tmp)
e.close()
print("poisoned dedup ok")
"""


def _all_small(e, tmp):
    for name in M.SMALL_NAMES:
        check(e, tmp, name, aligns=(0, 3))


def _all_large(e, tmp):
    for name in M.NAMES:
        if name not in M.SMALL_NAMES:
            check(e, tmp, name, aligns=(0,))


def _all_refused(e, tmp):
    refusals_hold(e, tmp)
    for name in SHORT:
        short_caps_hold(e, name)


POISONED = {"small": _all_small, "large": _all_large, "refused": _all_refused}


@pytest.mark.parametrize("part", sorted(POISONED))
def test_forms_on_a_poisoned_workspace(tmp_path, part):
    """the file once more -- every case and variant in every form, the refusals, the short capacities -- in fresh processes whose
    arena and text buffer hold 0x41 before every call"""
    script = put(tmp_path, "child.py", (CHILD % ROOT).encode())
    r = subprocess.run([sys.executable, script, str(tmp_path), part], env=dict(os.environ, BFQ_POISON="0x41"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"poisoned dedup ok" in r.stdout, r.stdout.decode()[-4000:]


def _run(args):
    return subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_tool(engine, tmp_path):
    import gzip
    tool = os.path.join(DROP, "bfq_dedup")
    path = lambda n: str(tmp_path / n)
    read = lambda n: open(path(n), "rb").read()
    (t1, t2), _ = M.all_cases()["pairs-mix"]
    kept, removed, st = M.expect("pairs-mix")
    a, b = put(tmp_path, "a.fq", t1), put(tmp_path, "b.fq", t2)
    r = _run([tool, "-i", a, "-j", b, "-o", path("k1.fq"), "-p", path("k2.fq"), "-D", path("d1.fq"), "-E", path("d2.fq"), "-r", path("rep.json")])
    assert r.returncode == 1 and b"11 pairs: 10 kept, 1 removed" in r.stdout, (r.stdout, r.stderr)     # duplicates were found: 1
    assert [read("k1.fq"), read("k2.fq")] == kept and [read("d1.fq"), read("d2.fq")] == removed
    rep = json.load(open(path("rep.json")))
    assert {k: rep[k] for k in st} == st and rep["paired"] == 1 and rep["keep"] == 0
    r = _run([tool, "-i", path("k1.fq"), "-j", path("k2.fq"), "-o", path("kk1.fq"), "-p", path("kk2.fq")])
    assert r.returncode == 0 and [read("kk1.fq"), read("kk2.fq")] == kept, (r.stdout, r.stderr)          # nothing left to remove: 0
    # single-end, the best qualities, the count alone
    (text, _), _ = M.all_cases()["keep-middle"]
    bk, br, bst = M.expect("keep-middle")
    s = put(tmp_path, "s.fq", text)
    r = _run([tool, "-i", s, "-o", path("sk.fq"), "-q", "-D", path("sd.fq")])
    assert r.returncode == 1 and read("sk.fq") == bk[0] and read("sd.fq") == br[0] and b"400 reads: 101 kept, 299 removed" in r.stdout, (r.stdout, r.stderr)
    r = _run([tool, "-i", s, "-o", path("s0.fq")])
    assert r.returncode == 1 and read("s0.fq") == M.expect("keep-middle-rule-0")[0][0]
    r = _run([tool, "-t", "-i", s, "-r", path("t.json")])
    assert r.returncode == 1 and b"the largest of 300 at record" in r.stdout and json.load(open(path("t.json")))["max_group"] == 300, (r.stdout, r.stderr)
    # compressed inputs are inflated first: BGZF, and plain gzip with -g
    put(tmp_path, "s.fq.gz", engine.bgzf_deflate(text).tobytes())
    r = _run([tool, "-i", path("s.fq.gz"), "-o", path("z.fq"), "-q"])
    assert r.returncode == 1 and read("z.fq") == bk[0], (r.stdout, r.stderr)
    put(tmp_path, "s.gz", gzip.compress(text))
    r = _run([tool, "-g", "-i", path("s.gz"), "-o", path("zz.fq"), "-q"])
    assert r.returncode == 1 and read("zz.fq") == bk[0], (r.stdout, r.stderr)
    # refusals: exit status 2, the library's message, empty outputs
    btexts, _, _, msg = M.refusals()["counts"]
    r = _run([tool, "-i", put(tmp_path, "c1.fq", btexts[0]), "-j", put(tmp_path, "c2.fq", btexts[1]), "-o", path("x1.fq"), "-p", path("x2.fq")])
    assert r.returncode == 2 and msg.encode() in r.stderr and os.path.getsize(path("x1.fq")) == os.path.getsize(path("x2.fq")) == 0, r.stderr
    for args in (["-i", s], ["-i", s, "-o", path("u.fq"), "-p", path("u2.fq")], ["-i", a, "-j", b, "-o", path("u.fq")], ["-t", "-i", s, "-o", path("u.fq")],
                 ["-i", a, "-j", b, "-o", path("u.fq"), "-p", path("u2.fq"), "-D", path("u3.fq")], ["-o", path("u.fq")]):
        assert _run([tool] + args).returncode == 2, args


def test_parallel_dedup(engine, tmp_path):
    """parallel.py --dedup / --dedup-best with the real Engine: the run on the inputs with duplicates equals the run on the
    model's kept texts; the removed records stay beside the outputs, the kept files are intermediates"""
    from tests.test_dedup_parallel import _with_duplicates
    for d in "cd":
        os.mkdir(str(tmp_path / d))
    out = lambda d, n: str(tmp_path / d / n)
    ins = _with_duplicates(str(tmp_path))
    texts = [open(p, "rb").read() for p in ins]
    for best, (want_dir, got_dir) in ((True, "cd"),):               # paired, the best qualities
        kept, removed, st = M.dedup(texts, keep=int(best))
        assert st["removed"] == 3
        k = [put(tmp_path, "kept%d_%d.fastq" % (best, m + 1), t) for m, t in enumerate(kept)]
        assert parallel.main(k + ["-p", "-o", out(want_dir, "OUT"), "-t", "2", "-0", "-H"]) == 0
        assert parallel.main(ins + ["-p", "--dedup-best" if best else "--dedup", "-o", out(got_dir, "OUT"), "-t", "2", "-0", "-H"]) == 0
        assert [open(out(got_dir, "OUT_%d.fastq" % m), "rb").read() for m in (1, 2)] == [open(out(want_dir, "OUT_%d.fastq" % m), "rb").read() for m in (1, 2)]
        assert [open(out(got_dir, "dup_1.dups_%d.fastq" % m), "rb").read() for m in (1, 2)] == removed
        assert sorted(os.listdir(str(tmp_path / got_dir))) == ["OUT_1.fastq", "OUT_2.fastq", "dup_1.dups_1.fastq", "dup_1.dups_2.fastq"]
    kept, removed, st = M.dedup(texts[:1])                          # single-end
    k = put(tmp_path, "kept_s.fastq", kept[0])
    os.mkdir(str(tmp_path / "e")); os.mkdir(str(tmp_path / "f"))
    assert parallel.main([k, "-o", out("e", "OUT"), "-t", "2", "-0", "-H"]) == 0
    assert parallel.main(ins[:1] + ["--dedup", "-o", out("f", "OUT"), "-t", "2", "-0", "-H"]) == 0
    assert open(out("f", "OUT.fastq"), "rb").read() == open(out("e", "OUT.fastq"), "rb").read() and open(out("f", "dup_1.dups.fastq"), "rb").read() == removed[0]
    bad = put(tmp_path, "short.fq", b"".join(b for _, b in M.P.records(texts[1])[:-1]))
    assert parallel.main([ins[0], bad, "-p", "--dedup", "-o", out("f", "BAD"), "-t", "2", "-0"]) == 1
    assert sorted(os.listdir(str(tmp_path / "f"))) == ["OUT.fastq", "dup_1.dups.fastq"]
