"""GPU tests of the fidelity report (bfq_fastq_compare / _fd, dropin/bfq_compare, parallel.py --report): in every case the
report and the diff list equal tests/compare_model.py, with ==; the diff buffer is filled with a sentinel beforehand and must
be untouched beyond what was asked for."""
import ctypes as C
import json
import os
import struct
import subprocess
import numpy as np
import pytest
from bfqzip_amd import _lib, api, parallel
from tests import compare_model as cm, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dropin", "bfq_compare")
NAMES = ("example", "paired", "synth_fix", "synth_var")
E_ARG, E_NOMEM = -1, -7
SENT = 0xA5


def _raw(name, ext=".fastq"):
    return open(os.path.join(util.GOLDEN, name + ext), "rb").read()


def sentinel(n):
    buf = np.zeros(n, api.DIFF_DTYPE)
    buf.view(np.uint8)[:] = SENT
    return buf


def intact(buf, start=0):
    return bool((buf[start:].view(np.uint8) == SENT).all())


def assert_report(rep, M, max_diffs):
    """rep (api.CompareReport) == M (the model's dict, whose diff list may be longer than what was asked for)."""
    for k in cm.SCALARS:
        assert getattr(rep, k) == M[k], k
    for k in cm.ARRAYS:
        assert np.array_equal(np.asarray(getattr(rep, k)).reshape(-1), M[k]), k
    want = M["diffs"][:max_diffs]
    assert len(want) == min(M["n_diffs"], max_diffs)         # (the model was asked for enough)
    assert len(rep.diffs) == len(want) and np.array_equal(rep.diffs, want)
    assert rep.identical == (M["n_diffs"] == 0)


def check(engine, a_parts, b_parts, M, max_diffs=0, permz=None):
    buf = sentinel(max_diffs + 3)
    rep = engine.fastq_compare(a_parts, b_parts, perm=permz, max_diffs=max_diffs, diffs_out=buf)
    assert_report(rep, M, max_diffs)
    assert intact(buf, min(M["n_diffs"], max_diffs))
    return rep


def raw_compare(engine, a_parts, b_parts, permz=None, cap=4):
    """The C call itself, for the refusals: (code, message, the report as bytes, the sentinel buffer)."""
    def parts(texts):
        arrs = [np.frombuffer(t, np.uint8) for t in texts]
        tp = (_lib.TextPart * len(arrs))()
        for i, x in enumerate(arrs):
            tp[i].data, tp[i].len = (x.ctypes.data if len(x) else None), len(x)
        return arrs, tp
    ka, ta = parts(a_parts)
    kb, tb = parts(b_parts)
    z = np.frombuffer(bytes(permz), np.uint8) if permz is not None else None
    rep = _lib.CompareReport()
    C.memset(C.byref(rep), 0xFF, C.sizeof(rep))
    buf = sentinel(cap)
    rc = engine.L.bfq_fastq_compare(engine.h, ta, len(ka), tb, len(kb), C.c_void_p(z.ctypes.data) if z is not None else None,
                                    len(z) if z is not None else 0, C.byref(rep), C.c_void_p(buf.ctypes.data), cap)
    return rc, engine.L.bfq_last_error(engine.h).decode(), bytes(rep), buf


def refused(engine, a_parts, b_parts, code=E_ARG, **kw):
    rc, msg, rep, buf = raw_compare(engine, a_parts, b_parts, **kw)
    assert rc == code, (rc, msg)
    assert rep == bytes(len(rep)) and intact(buf), msg       # the report zeroed, the diff buffer untouched
    return msg


# ---- texts ------------------------------------------------------------------------------------------------------------------
def fq_text(b, q, r, hdrs=None, eol=b"\n"):
    out = []
    for i in range(len(r) - 1):
        s, e = int(r[i]), int(r[i + 1])
        out += [hdrs[i] if hdrs is not None else b"@", eol, b[s:e].tobytes(), eol, b"+", eol, q[s:e].tobytes(), eol]
    return b"".join(out)


def record_list(text):
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
    ends = nl[3::4] + 1
    starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
    return [text[int(s):int(e)] for s, e in zip(starts, ends)]


OTHER = np.frombuffer(b"ACGTNaR", np.uint8)                  # a and R: class 5


def mutate(rng, b, q, qvals=None):
    """B from A: 2 % of the bases replaced by another of ACGTN or by a / R, 30 % of the qualities moved by +-1..40 within
    33..126 (qvals given: redrawn from those values instead)."""
    b2, q2 = b.copy(), q.copy()
    at = np.flatnonzero(rng.random(len(b)) < 0.02)
    pick = rng.integers(0, len(OTHER), len(at))
    pick = np.where(OTHER[pick] == b[at], (pick + 1) % len(OTHER), pick)
    b2[at] = OTHER[pick]
    at = np.flatnonzero(rng.random(len(q)) < 0.30)
    if qvals is None:
        d = rng.integers(1, 41, len(at)) * rng.choice([-1, 1], len(at))
        q2[at] = np.clip(q[at].astype(np.int64) + d, 33, 126).astype(np.uint8)
    else:
        q2[at] = qvals[rng.integers(0, len(qvals), len(at))]
    return b2, q2


EDGE_LENS = (1, 63, 64, 65, 128, 129, 511, 512, 513, 700)


def edge_collection(rng, qvals=None):
    """300 random reads with the edge lengths among them; B made as mutate() says, the 700-base read differing in its first and
    its last 64-position step only, the last read's last position differing."""
    b, q, r = util.random_reads(rng, 300, 20, 150, qhi=126)
    lens = list(np.diff(r.astype(np.int64)))
    reads = [(b[int(r[i]):int(r[i + 1])], q[int(r[i]):int(r[i + 1])]) for i in range(300)]
    for k, L in enumerate(EDGE_LENS):
        s = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, L)]
        reads.insert(7 + 29 * k, (s, rng.integers(33, 127, L).astype(np.uint8)))
    b = np.concatenate([x for x, _ in reads]); q = np.concatenate([y for _, y in reads])
    if qvals is not None:
        q = qvals[rng.integers(0, len(qvals), len(q))]
    r = np.concatenate([[0], np.cumsum([len(x) for x, _ in reads])]).astype(np.uint64)
    b2, q2 = mutate(rng, b, q, qvals)
    i700 = [len(x) for x, _ in reads].index(700)
    s = int(r[i700])
    b2[s:s + 700], q2[s:s + 700] = b[s:s + 700], q[s:s + 700]
    ok = set(int(v) for v in qvals) if qvals is not None else set(range(33, 127))
    other = lambda v: next(c for c in (int(v) + 1, int(v) + 2, int(v) + 3, int(v) - 1, int(v) - 2) if c in ok)
    b2[s + 3] = ord("a"); q2[s + 650] = other(q[s + 650]); b2[s + 650] = ord("R"); q2[s + 699] = other(q[s + 699])
    q2[-1] = other(q[-1])
    return (b, q, r), (b2, q2, r)


@pytest.fixture(scope="module")
def golden_models():
    out = {}
    for name in NAMES:
        a, b = _raw(name), _raw(name, ".M2B0.fq")
        M = cm.compare([a], [b])
        out[name] = (a, b, cm.compare([a], [b], max_diffs=M["n_diffs"] + 5))
    return out


@pytest.fixture(scope="module")
def big():
    """40 000 x 100: A, B and the model's compare with 1000 diffs."""
    rng = np.random.default_rng(40000)
    N, L = 40000, 100
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N * L)]
    q = rng.integers(33, 75, N * L).astype(np.uint8)
    b2, q2 = mutate(rng, b, q)

    def text(b, q):
        m = np.empty((N, 2 * L + 6), np.uint8)
        m[:, 0], m[:, 1] = ord("@"), 10
        m[:, 2:2 + L] = b.reshape(N, L)
        m[:, 2 + L:5 + L] = np.frombuffer(b"\n+\n", np.uint8)
        m[:, 5 + L:5 + 2 * L] = q.reshape(N, L)
        m[:, 5 + 2 * L] = 10
        return m.tobytes()
    A, B = text(b, q), text(b2, q2)
    return A, B, cm.compare([A], [B], max_diffs=1000)


# ---- 1, 2: the goldens, a text against itself ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_golden_pairs(engine, golden_models, name):
    a, b, M = golden_models[name]
    assert (M["n_reads"], M["total_bases"]) == {"example": (100, 10100), "paired": (200, 20200), "synth_fix": (1500, 90000), "synth_var": (2000, 89495)}[name]
    for md in (0, 7, M["n_diffs"] + 5):
        check(engine, [a], [b], M, md)


def test_text_against_itself(engine):
    a = _raw("synth_var")
    M = cm.compare([a], [a])
    rep = check(engine, [a], [a], M, 16)
    assert rep.identical and rep.first_changed_read == api.NO_READ == (1 << 64) - 1 and rep.headers_same == rep.n_reads == 2000 and len(rep.diffs) == 0


# ---- 3: edge lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw_quals", (False, True))
def test_edge_lengths(engine, raw_quals):
    rng = np.random.default_rng(3 + raw_quals)
    qvals = np.array([v for v in range(1, 256) if v not in (10, 13)], np.uint8) if raw_quals else None
    (b, q, r), (b2, q2, _) = edge_collection(rng, qvals)
    A, B = fq_text(b, q, r, eol=b"\r\n"), fq_text(b2, q2, r)         # A has CRLF line ends, B LF
    M = cm.compare([A], [B], max_diffs=10 ** 6)
    assert M["n_diffs"] > 1000 and int(M["diffs"]["read"][-1]) == len(r) - 2 and int(M["pos_len"][511]) == 1 + 2 + 189
    i700 = list(np.diff(r.astype(np.int64))).index(700)
    assert [int(p) for p in M["diffs"]["pos"][M["diffs"]["read"] == i700]] == [3, 650, 699]
    if raw_quals:
        assert M["qual_abs_max"] > 200 and np.count_nonzero(M["qual_hist_a"]) == 253
    for md in (0, 50, M["n_diffs"], M["n_diffs"] + 9):
        check(engine, [A], [B], M, md)
    # the cap inside the 700-base read's differences: the read straddles it
    upto = int(np.flatnonzero(M["diffs"]["read"] == i700)[0])
    for md in (upto + 1, upto + 2):
        check(engine, [A], [B], M, md)


# ---- 4: headers ----------------------------------------------------------------------------------------------------------------
def test_header_classes(engine):
    rng = np.random.default_rng(4)
    b, q, r = util.random_reads(rng, 120, 10, 80)
    N = len(r) - 1
    ha = [b"@read.%d some text/1" % i for i in range(N)]
    ha[5] = b"@"
    A = fq_text(b, q, r, ha, eol=b"\r\n")
    alt = [h + b"x" if i % 7 == 0 else h for i, h in enumerate(ha)]
    for hb, want in ((None, (1, N - 1, 0)), (ha, (N, 0, 0)), (alt, (N - (N + 6) // 7, 0, (N + 6) // 7))):
        B = fq_text(b, q, r, hb)
        M = cm.compare([A], [B])
        assert (M["headers_same"], M["headers_dropped"], M["headers_changed"]) == want
        rep = check(engine, [A], [B], M, 4)
        assert rep.identical                                 # headers are no payload


# ---- 5: parts ------------------------------------------------------------------------------------------------------------------
def test_parts(engine, golden_models):
    a, b, M = golden_models["synth_var"]
    ra, rb = record_list(a), record_list(b)
    ca = (len(b"".join(ra[:300])), len(b"".join(ra[:1201])))
    cb = len(b"".join(rb[:777]))
    a_parts = [a[:ca[0] - 1], a[ca[0]:ca[1]], a[ca[1]:]]     # the first part without its final newline
    b_parts = [b[:cb], b[cb:-1]]                             # ... and the last one of B
    for md in (0, 33):
        check(engine, a_parts, b_parts, M, md)
    rep = check(engine, [b""], [b""], cm.compare([b""], [b""]), 5)
    assert rep.n_reads == 0 and rep.total_bases == 0 and rep.identical and rep.as_dict()["pos_len"] == []
    assert all(getattr(rep, k) == 0 for k in cm.SCALARS if k != "first_changed_read")


# ---- 6: permutation --------------------------------------------------------------------------------------------------------------
def raw_container(perm):
    """The BFQPERM1 bytes of any entries, valid or not (api.perm_encode refuses what is no permutation)."""
    N = len(perm)
    w = 1 if N <= 2 else (N - 1).bit_length()
    bits = 0
    for j, v in enumerate(perm):
        bits |= int(v) << (j * w)
    return b"BFQPERM1" + struct.pack("<QIIIIQ", N, w, 0, 0, 0, 0) + bits.to_bytes(8 * ((N * w + 63) // 64), "little")


def test_permutation(engine):
    rng = np.random.default_rng(6)
    (b, q, r), (b2, q2, _) = edge_collection(rng)
    N = len(r) - 1
    A, B0 = fq_text(b, q, r), fq_text(b2, q2, r)             # B0: B before the reordering
    (reordered,), permz = engine.fastq_reorder([A], keep=True)
    perm, _ = api.perm_decode(permz)
    assert sorted(int(v) for v in perm) == list(range(N)) and not np.array_equal(perm, np.arange(N))
    ra, rb0 = record_list(A), record_list(B0)
    assert reordered.tobytes() == b"".join(ra[int(v)] for v in perm)
    B = b"".join(rb0[int(v)] for v in perm)                  # the reordered text, mutated
    M = cm.compare([A], [B0], max_diffs=10 ** 6)
    Mp = cm.compare([A], [B], perm=perm, max_diffs=10 ** 6)
    assert all(M[k] == Mp[k] for k in cm.SCALARS) and np.array_equal(M["diffs"], Mp["diffs"])
    for md in (0, 100, M["n_diffs"] + 1):
        check(engine, [A], [B], M, md, permz=permz)
    assert raw_container(perm)[:20] == bytes(permz[:20]) and raw_container(perm)[40:] == bytes(permz[40:])
    check(engine, [A], [B], M, 10, permz=np.frombuffer(raw_container(perm), np.uint8))
    # a permutation of N + 1 reads: both numbers are named
    msg = refused(engine, [A], [B], permz=api.perm_encode(np.arange(N + 1)))
    assert str(N + 1) in msg and str(N) in msg.replace(str(N + 1), "")
    # a value twice: the first offending position is named
    twice = [int(v) for v in perm]
    twice[211] = twice[40]
    msg = refused(engine, [A], [B], permz=raw_container(twice))
    assert "211" in msg
    assert "BFQPERM1" in refused(engine, [A], [B], permz=b"BFQPERM2" + raw_container(perm)[8:])


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(engine, big):
    rec = lambda i, L: b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT" * (L // 4), b"I" * L)
    a = b"".join(rec(i, 40) for i in range(100))
    msg = refused(engine, [a], [b"".join(rec(i, 40) for i in range(99))])
    assert "100" in msg and "99" in msg
    msg = refused(engine, [a], [b"".join(rec(i, 44 if i in (37, 12) else 40) for i in range(100))])
    assert "read 12" in msg and "40" in msg and "44" in msg and "37" not in msg
    msg = refused(engine, [a], [a[:a.rindex(b"\n", 0, len(a) - 1) + 1]])          # B loses its last line
    assert msg.startswith("B: ") and "multiple of 4" in msg
    msg = refused(engine, [a.replace(b"IIII\n", b"III\n", 1)], [a])
    assert msg.startswith("A: ") and "len(DNA) != len(QS)" in msg
    A, B, M = big
    small = api.Engine(0, ws_cap_mib=1)
    try:
        msg = refused(small, [A], [B], code=E_NOMEM)
        assert "GiB" in msg
    finally:
        small.close()
    check(engine, [a], [a], cm.compare([a], [a]), 2)         # the engine goes on


# ---- 8: many workgroups ------------------------------------------------------------------------------------------------------------
def test_many_workgroups(engine, big):
    A, B, M = big
    assert M["n_reads"] == 40000 and M["total_bases"] == 4000000 and M["n_diffs"] > 10 ** 6 and M["qual_sq_sum"] > 1 << 28
    check(engine, [A], [B], M, 1000)
    os.environ["BFQ_CMP_HIST"] = "runs"                      # the histogram adds by run heads count the same
    try:
        check(engine, [A], [B], M, 0)
    finally:
        del os.environ["BFQ_CMP_HIST"]


# ---- 9: end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end(golden_models):
    eng = api.Engine(0, m=5, M=2, B=0)
    try:
        for name in NAMES:
            a = golden_models[name][0]
            out, st = eng.fastq_run(a, keep_headers=True)
            rep = eng.fastq_compare([a], [out])
            assert rep.bases_changed == st["modified"] and rep.quals_changed <= st["qs_smoothed"] and rep.headers_same == rep.n_reads
            assert_report(rep, cm.compare([a], [out]), 0)
        eng.set_params(m=5, M=2, B=1)
        out, st = eng.fastq_run(golden_models["example"][0], keep_headers=True)
        rep = eng.fastq_compare([golden_models["example"][0]], [out])
        assert 1 <= np.count_nonzero(rep.qual_hist_b) <= 8 < np.count_nonzero(rep.qual_hist_a)
    finally:
        eng.close()


# ---- 10: files and the tool ----------------------------------------------------------------------------------------------------------
def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


def test_files_and_tool(engine, golden_models, tmp_path):
    assert os.path.exists(TOOL), f"{TOOL} missing: run __graft_entry__.build()"
    a, b, M = golden_models["example"]
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a); open(fb, "wb").write(b[:-1])    # (no final newline in the file)
    rep = engine.fastq_compare_files(fa, fb, max_diffs=7)
    assert_report(rep, M, 7)
    assert rep.as_dict() == engine.fastq_compare([a], [b], max_diffs=7).as_dict()
    r = _run([TOOL, "-a", fa, "-b", fa])
    assert r.returncode == 0 and json.loads(r.stdout)["identical"] is True, r.stderr
    r = _run([TOOL, "-a", fa, "-b", fb, "-n", "7", "-V"])
    assert r.returncode == 1 and b"[bfq phases]" in r.stderr, r.stderr
    js = json.loads(r.stdout)
    assert js.pop("diffs") == [[int(v) for v in d] for d in rep.diffs.tolist()] and len(rep.diffs) == 7
    assert js == rep.as_dict() and js["first_changed_read"] == M["first_changed_read"] and len(js["pos_len"]) == 101
    out = str(tmp_path / "rep.json")
    r = _run([TOOL, "-a", fa, "-b", fb, "-o", out])
    assert r.returncode == 1 and r.stdout == b"" and json.load(open(out)) == rep.as_dict()
    # the reordered file with its permutation: the same report; a permutation of another collection: exit 2
    fr, fp = str(tmp_path / "r.fq"), str(tmp_path / "r.perm")
    engine.fastq_reorder_files([fb], [fr], perm_path=fp)
    r = _run([TOOL, "-a", fa, "-b", fr, "-P", fp])
    assert r.returncode == 1 and json.loads(r.stdout) == rep.as_dict(), r.stderr
    assert engine.fastq_compare_files(fa, fr, perm_path=fp, max_diffs=7).as_dict() == rep.as_dict()
    other = str(tmp_path / "o.perm")
    open(other, "wb").write(api.perm_encode(np.arange(99)).tobytes())
    for cmd in ([TOOL, "-a", fa, "-b", str(tmp_path / "missing.fq")], [TOOL, "-a", fa, "-b", fr, "-P", other], [TOOL, "-a", fa, "-b", fr, "-P", fa],
                [TOOL, "-a", fa]):
        r = _run(cmd)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr, cmd
    assert b"99" in _run([TOOL, "-a", fa, "-b", fr, "-P", other]).stderr


# ---- 11: the driver ------------------------------------------------------------------------------------------------------------------
def test_parallel_report(engine, tmp_path):
    src = str(tmp_path / "in.fastq")
    open(src, "wb").write(_raw("synth_var"))
    out = str(tmp_path / "R")
    assert parallel.main([src, "-t", "4", "-o", out, "--report"]) == 0
    js = json.load(open(out + ".fastq.report.json"))
    assert js == engine.fastq_compare_files(src, out + ".fastq").as_dict() and js["n_reads"] == 2000 and js["n_diffs"] > 0
    # nothing to compare with when the merged text is not written: refused at argument checking, nothing written
    before = sorted(os.listdir(str(tmp_path)))
    assert parallel.main([src, "-t", "4", "-o", str(tmp_path / "C"), "--compress", "--report"]) != 0
    assert parallel.main([src, "-t", "4", "-o", str(tmp_path / "S"), "--m2", "--streams-only", "--report"]) != 0
    assert sorted(os.listdir(str(tmp_path))) == before
