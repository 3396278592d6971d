"""GPU tests of the k-mer spectrum report (bfq_fastq_kmers / _fd, dropin/bfq_kmers, parallel.py --report-kmers): in every case
the report and the list equal tests/kmers_model.py, with ==; the list buffer is filled with a sentinel beforehand and must be
untouched beyond what was asked for.  The shapes are the smallest at which each kernel can still go wrong: the key widths on
both sides of the one-round / two-round step, the window borders, runs that end and start at a chunk's border, value ranges
of one bin."""
import ctypes as C
import json
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import _lib, api, parallel
from tests import bgzf_model as BG
from tests import kmers_model as km, util
from tests import test_kmers_host as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dropin", "bfq_kmers")
E_ARG, E_NOMEM = -1, -7
NL_CHUNK = 4096                                              # BFQ_NL_CHUNK: text bytes per workgroup of the line kernels


class poisoned:
    """BFQ_POISON=<byte> in the environment for the time of the block (as tests/test_gpu_poison.py sets it); what stood there
    before comes back."""

    def __init__(self, byte):
        self.value = "0x%02X" % byte

    def __enter__(self):
        self.old = os.environ.get("BFQ_POISON")
        os.environ["BFQ_POISON"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("BFQ_POISON", None)
        else:
            os.environ["BFQ_POISON"] = self.old


def geometry():
    seg, run, starts = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().bfq_kmers_geometry(C.byref(seg), C.byref(run), C.byref(starts)) == 0
    return int(seg.value), int(run.value), int(starts.value)


def check(engine, a_parts, b_parts, max_list=8, M=None, **kw):
    M = M or km.kmers(a_parts, b_parts, **kw)
    buf = H.sentinel(max_list + 3)
    rep = engine.fastq_kmers(a_parts, b_parts, max_list=max_list, list_out=buf, **kw)
    H.assert_report(rep, M, max_list)
    assert H.intact(buf, min(M["n_listed"], max_list))
    return rep, M


# ---- 1: the goldens --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.NAMES)
@pytest.mark.parametrize("k", (8, 20, 21, 31))
def test_goldens(engine, name, k):
    a, b = H.golden(name), H.golden(name, ".M2B0.fq")
    for solid in (2, 3):
        for canonical in (False, True):
            check(engine, [a], [b], 37, M=H.golden_model(name, k, solid, canonical), k=k, solid=solid, canonical=canonical)
    check(engine, [a], None, 0, M=H.golden_model(name, k, single=True), k=k)
    if (name, k) in H.RECORDED:                              # the numbers a user reads: the recorded table
        rep = engine.fastq_kmers([a], [b], k=k)
        assert (rep.windows_a, rep.windows_b, rep.distinct_a, rep.distinct_b, rep.only_a, rep.solid_lost, rep.only_b, rep.distinct_changed) == H.RECORDED[(name, k)]


# ---- 2: key widths and window borders ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 9, 20, 21, 31))
def test_borders(engine, k):
    """k = 20: 40 bits, one sort round; 21: the first two-round k; 31: 62 bits.  The texts hold T x 31, A x 31, two k-mers that
    differ in the lowest base only, reads of 0, k - 1, k, k + 1 bases, N first, last, in the middle, twice k and k - 1 apart,
    lower case, CRLF, no final newline, an empty text."""
    rng = np.random.default_rng(100 + k)
    for a, b in H.border_texts(k, rng):
        for canonical in (True, False):
            check(engine, [a], [b], k=k, solid=2, canonical=canonical)
        check(engine, [a], None, k=k)


def test_parts_long_reads_and_chunk_borders(engine):
    rng = np.random.default_rng(11)
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n, p=[.245, .245, .245, .245, .02]))
    _, _, starts = geometry()
    step = 16 * starts                                       # start positions of one step of a group of lanes
    long_read = rnd(5000)                                    # many steps of one group
    reads = [rnd(int(n)) for n in rng.integers(15, 120, 40)]
    a = H.fq(reads + [rnd(300), long_read, rnd(step + 20), rnd(step + 21), rnd(step + 19), rnd(2 * step + 20)])
    b = H.fq([long_read[:2500] + b"A" + long_read[2501:]] + reads[::-1])
    for k in (8, 21, 31):
        check(engine, [a], [b], k=k)
    # three parts each.  A part without its final newline gets one, so a cut in the middle of a sequence line makes another
    # text, one that the parser refuses: the model and the library agree on that ...
    cut = lambda t: [t[:len(t) // 3 + 5], t[len(t) // 3 + 5:2 * len(t) // 3 + 7], t[2 * len(t) // 3 + 7:]]
    pa, pb = cut(a), cut(b)
    assert all(not p.endswith(b"\n") for p in pa[:2] + pb[:2])
    with pytest.raises(km.Malformed):
        km.kmers(pa, pb, k=21)
    assert refused(engine, pa, pb).startswith("A: ")
    # ... and cuts behind a record's sequence line (the part ends with that line's newline) give the one text back
    nla = [i + 1 for i in range(len(a)) if a[i:i + 1] == b"\n"]
    nlb = [i + 1 for i in range(len(b)) if b[i:i + 1] == b"\n"]
    pa = [a[:nla[5]], a[nla[5]:nla[len(nla) // 2 + 1]], a[nla[len(nla) // 2 + 1]:]]
    pb = [b[:nlb[1]], b[nlb[1]:nlb[6]], b[nlb[6]:]]
    check(engine, pa, pb, M=km.kmers([a], [b], k=21), k=21)
    # a sequence line across the border of the line kernels' chunk: a first record sized so that the second's line straddles it
    half = (NL_CHUNK - 60 - 7) // 2
    first = b"@x\n" + b"C" * half + b"\n+\n" + b"I" * half + b"\n"
    t = first + H.fq([rnd(200), rnd(90)])
    assert len(first) + 4 < NL_CHUNK < len(first) + 4 + 200
    check(engine, [t], [t[:-1]], k=21)


# ---- 3: strand -----------------------------------------------------------------------------------------------------------------
def test_strand_and_palindromes(engine, tmp_path):
    rng = np.random.default_rng(7)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n))) for n in rng.integers(25, 90, 60)]
    a = H.fq(reads)
    b = H.fq([H.rc(reads[i]) for i in rng.permutation(len(reads))])
    rep, _ = check(engine, [a], [b], k=21)
    assert rep.unchanged and rep.distinct_a == rep.distinct_both
    rep, _ = check(engine, [a], [b], k=21, canonical=False)
    assert not rep.unchanged
    rep, _ = check(engine, [H.fq([b"ACGTACGT"])], None, k=8)
    assert (rep.windows_a, rep.distinct_a, int(rep.hist_a[1])) == (1, 1, 1)
    check(engine, [H.fq([b"ACGTACGTACGT", b"TTTTAAAA", b"AATT" * 5])], [H.fq([b"ACGTACGT"])], k=8)
    fa, fb = str(tmp_path / "a.fq"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a); open(fb, "wb").write(b)
    assert _run([TOOL, "-a", fa, "-b", fb]).returncode == 0
    assert _run([TOOL, "-a", fa, "-b", fb, "-f"]).returncode == 1


# ---- 4: long runs ---------------------------------------------------------------------------------------------------------------
def test_long_runs(engine):
    seg, run, _ = geometry()
    read = b"ACGGTCATTGCAAGCTTAGGCTAACGTTAGCCATGCAATGC"[:40]
    a = H.fq([read] * 20000)                                 # 20 runs of 20 000 rows: several chunks and radix tiles each
    rep, M = check(engine, [a], [H.fq([read] * 9 + [read[:30]] * 20)], k=21, solid=3)
    assert int(rep.hist_a[255]) == rep.distinct_a == 20 and int(rep.joint[15, 9]) == 10 and int(rep.joint[15, 15]) == 10
    rep, M = check(engine, [H.fq([b"A" * 5000])], None, k=21)
    assert (rep.distinct_a, rep.windows_a, int(rep.hist_a[255])) == (1, 4980, 1)
    check(engine, [H.fq([b"A" * 5000, b"T" * 4000])], [H.fq([b"A" * 30 + b"C"])], k=21, solid=2)
    # forward 8-mers in sorted order: AAAAAAAA (value 0) first.  With n of them its run ends at row n - 1 and the next run starts at
    # row n: n = the chunk's rows puts the end on a chunk's last row and the start on the next one's first
    for n in (seg - 1, seg, seg + 1, 2 * seg):
        a = H.fq([b"A" * 8] * (n - 3) + [b"C" * 8] * 5)
        b = H.fq([b"A" * 8] * 3 + [b"G" * 8] * (seg - 5) + [b"T" * 8])
        rep, M = check(engine, [a], [b], k=8, canonical=False, solid=2)
        assert M["windows_a"] + M["windows_b"] == n + seg + 1
    # exactly one chunk of runs, one less and one more: every k-mer once
    rng = np.random.default_rng(3)
    for n in (run - 1, run, run + 1):
        vals = rng.choice(4 ** 8, n, replace=False)
        strs = [km.kmer_string(int(v), 8).encode() for v in vals]
        rep, M = check(engine, [H.fq(strs)], [H.fq(strs[:n // 2] * 2)], max_list=5, k=8, canonical=False, solid=2)
        assert rep.distinct_a == n


# ---- 5: value ranges -----------------------------------------------------------------------------------------------------------
def test_partitions(engine):
    a, b = H.golden("synth_fix"), H.golden("synth_fix", ".M2B0.fq")
    M0 = H.golden_model("synth_fix", 21, 2, True)
    ca, cb = M0["counts"]
    one = engine.fastq_kmers([a], [b], k=21, solid=2)
    H.assert_report(one, M0, 0)
    assert one.n_partitions == 1
    _, bins = km.ranges(ca, cb, 21, 0)
    largest = max(bins.values())
    for pr in (40000, largest - 1):                          # >= 3 ranges; a bound below the largest bin's count: that bin still runs
        rng_, _ = km.ranges(ca, cb, 21, pr)
        assert len(rng_) >= 3
        M = dict(M0, n_partitions=len(rng_))
        check(engine, [a], [b], 50, M=M, k=21, solid=2, part_records=pr)
        # the list's cap inside a range and exactly at a range's end
        part_of = {bn: i for i, r in enumerate(rng_) for bn in r}
        ends = [0] * len(rng_)
        for v, _, _ in M0["list"]:
            ends[part_of[v >> (42 - km.TOP_BITS)]] += 1
        cum = np.cumsum(ends)
        two = [int(c) for c, e in zip(cum, ends) if e >= 2][:-1]   # the list's length at the end of a range that lists two or more
        assert two or pr != 40000
        for cap in ([two[0], two[0] - 1, two[-1]] if two else []) + [int(cum[np.flatnonzero(ends)[0]]), int(cum[-1]), int(cum[-1]) + 1]:
            check(engine, [a], [b], cap, M=M, k=21, solid=2, part_records=pr)
    # every non-empty bin a range of its own
    a, b = H.golden("example"), H.golden("example", ".M2B0.fq")
    M0 = H.golden_model("example", 21, 3, True)
    rng_, bins = km.ranges(*M0["counts"], 21, 1)
    assert len(rng_) == len(bins) > 100
    check(engine, [a], [b], 10 ** 4, M=dict(M0, n_partitions=len(bins)), k=21, solid=3, part_records=1)


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------
def raw_kmers(engine, a_parts, b_parts, k=21, solid=3, reserved=0, cap=4):
    def parts(texts):
        arrs = [np.frombuffer(t, np.uint8) for t in texts]
        tp = (_lib.TextPart * max(len(arrs), 1))()
        for i, x in enumerate(arrs):
            tp[i].data, tp[i].len = (x.ctypes.data if len(x) else None), len(x)
        return arrs, tp
    ka, ta = parts(a_parts)
    kb, tb = parts(b_parts)
    rep = _lib.KmerReport()
    C.memset(C.byref(rep), 0xFF, C.sizeof(rep))
    buf = H.sentinel(cap)
    O = _lib.KmerOpts(k=k, solid=solid, canonical=1, reserved=reserved, part_records=0)
    rc = engine.L.bfq_fastq_kmers(engine.h, ta, len(ka), tb, len(kb), C.byref(O), C.byref(rep), C.c_void_p(buf.ctypes.data), cap)
    return rc, engine.L.bfq_last_error(engine.h).decode(), bytes(rep), buf


def refused(engine, a_parts, b_parts, code=E_ARG, **kw):
    rc, msg, rep, buf = raw_kmers(engine, a_parts, b_parts, **kw)
    assert rc == code, (rc, msg)
    assert rep == bytes(len(rep)) and H.intact(buf), msg     # the report zeroed, the list untouched
    return msg


def test_refusals(engine):
    a = H.fq([b"ACGTACGTACGTACGTACGTACGTACGTAAAC"] * 5)
    for kw in (dict(k=7), dict(k=32), dict(solid=1), dict(solid=16), dict(reserved=1)):
        refused(engine, [a], [a], **kw)
    msg = refused(engine, [a[:a.rindex(b"\n", 0, len(a) - 1) + 1]], [a])
    assert msg.startswith("A: ") and "multiple of 4" in msg
    msg = refused(engine, [a], [a.replace(b"IIII\n", b"III\n", 1)])
    assert msg.startswith("B: ") and "len(DNA) != len(QS)" in msg
    big = H.golden("synth_fix")
    small = api.Engine(0, ws_cap_mib=1)
    try:
        msg = refused(small, [big], [big], code=E_NOMEM)
        assert "GiB" in msg
    finally:
        small.close()
    check(engine, [a], [a], k=21)                            # the engine goes on


# ---- 7: the other forms --------------------------------------------------------------------------------------------------------
def _run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


def test_files_bgzf_and_tool(engine, tmp_path):
    assert os.path.exists(TOOL), f"{TOOL} missing: run __graft_entry__.build()"
    a, b = H.golden("example"), H.golden("example", ".M2B0.fq")
    M = H.golden_model("example", 21)
    fa, fz, fb = str(tmp_path / "a.fq"), str(tmp_path / "a.fq.gz"), str(tmp_path / "b.fq")
    open(fa, "wb").write(a); open(fz, "wb").write(BG.bgzf(a)); open(fb, "wb").write(b[:-1])   # (B: no final newline in the file)
    buf = H.sentinel(12)
    rep = engine.fastq_kmers_files(fz, fb, max_list=9, list_out=buf)                          # A is BGZF
    H.assert_report(rep, M, 9)
    assert H.intact(buf, min(M["n_listed"], 9))
    H.assert_report(engine.fastq_kmers_files(fa), H.golden_model("example", 21, single=True), 0)
    r = _run([TOOL, "-a", fa, "-b", fa])
    assert r.returncode == 0 and json.loads(r.stdout)["distinct_changed"] == 0, r.stderr
    r = _run([TOOL, "-a", fz, "-b", fb, "-n", "9", "-V"])
    assert r.returncode == 1 and b"[bfq phases]" in r.stderr, r.stderr
    js = json.loads(r.stdout)
    assert js == rep.as_dict() and js["list"] == [[km.kmer_string(v, 21), x, y] for v, x, y in M["list"][:9]]
    for key in km.SCALARS + km.ARRAYS:
        assert js[key] == M[key], key
    out = str(tmp_path / "rep.json")
    r = _run([TOOL, "-a", fa, "-b", fb, "-k", "8", "-s", "2", "-f", "-o", out])
    M8 = H.golden_model("example", 8, 2, False)
    assert r.returncode == 1 and r.stdout == b"" and all(json.load(open(out))[key] == M8[key] for key in km.SCALARS + km.ARRAYS)
    r = _run([TOOL, "-a", fa])                               # one file: its spectrum, exit 0
    assert r.returncode == 0 and json.loads(r.stdout)["distinct_a"] == M["distinct_a"]
    for cmd in ([TOOL, "-a", fa, "-b", str(tmp_path / "missing.fq")], [TOOL, "-a", fa, "-k", "32"], [TOOL, "-b", fb], [TOOL, "-a", fb + "x"]):
        r = _run(cmd)
        assert r.returncode == 2 and r.stdout == b"" and r.stderr, cmd


def test_parallel_report_kmers(engine, tmp_path):
    src = str(tmp_path / "in.fastq")
    open(src, "wb").write(H.golden("example"))
    out = str(tmp_path / "R")
    assert parallel.main([src, "-t", "2", "-o", out, "--report-kmers", "21"]) == 0
    js = json.load(open(out + ".fastq.kmers.json"))
    M = km.kmers([H.golden("example")], [open(out + ".fastq", "rb").read()], k=21)
    assert all(js[key] == M[key] for key in km.SCALARS + km.ARRAYS) and js["n_reads_a"] == js["n_reads_b"] > 0
    before = sorted(os.listdir(str(tmp_path)))
    assert parallel.main([src, "-t", "2", "-o", str(tmp_path / "C"), "--compress", "--report-kmers", "21"]) != 0
    assert parallel.main([src, "-t", "2", "-o", str(tmp_path / "S"), "--report-kmers", "32"]) != 0
    assert sorted(os.listdir(str(tmp_path))) == before


@pytest.mark.parametrize("byte", (0x41, 0xFF))
def test_poisoned_workspace(byte):
    a, b = H.golden("synth_var"), H.golden("synth_var", ".M2B0.fq")
    with poisoned(byte):
        e = api.Engine(0)
        try:
            e.stream_reserve(1 << 16)
            assert (e.workspace_read(0, 1 << 16) == byte).all()
            for k in (20, 21):
                check(e, [a], [b], 20, M=H.golden_model("synth_var", k), k=k)
            check(e, [a], [b], 20, M=dict(H.golden_model("synth_var", 21), n_partitions=len(km.ranges(*H.golden_model("synth_var", 21)["counts"], 21, 5000)[0])),
                  k=21, part_records=5000)
        finally:
            e.close()
