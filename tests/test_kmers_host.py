"""The k-mer spectrum report on the host: bfq_fastq_kmers_host == tests/kmers_model.py, with ==, on the goldens and on every
edge the definition has; the model reproduces the counts recorded for the goldens (made independently of the library); the
structures of _lib.py have the sizes the header states.  No GPU."""
import ctypes as C
import functools
import os
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import kmers_model as km, util

NAMES = ("example", "paired", "synth_fix", "synth_var")
E_ARG, E_TOO_LONG = -1, -5
SENT = 0xA5

# recorded for NAME.fastq against NAME.M2B0.fq, canonical k-mers: (name, k): windows A / B, distinct A / B, only in A, of those
# with count >= 3, only in B, distinct with cA != cB
RECORDED = {
    ("example", 21): (8058, 8079, 2566, 2458, 127, 0, 19, 235),
    ("synth_fix", 8): (78993, 79289, 7737, 5688, 2089, 4, 40, 4247),
    ("synth_fix", 21): (59024, 59641, 13828, 8313, 5884, 0, 369, 9029),
    ("synth_fix", 31): (43956, 44619, 14334, 8505, 6633, 0, 804, 10242),
    ("synth_var", 21): (35802, 39461, 15982, 13756, 3243, 0, 1017, 6926),
    ("synth_var", 31): (18435, 21317, 12265, 11041, 2767, 0, 1543, 6456),
}


def golden(name, ext=".fastq"):
    return open(os.path.join(util.GOLDEN, name + ext), "rb").read()


@functools.lru_cache(maxsize=None)
def golden_model(name, k, solid=3, canonical=True, single=False):
    return km.kmers([golden(name)], None if single else [golden(name, ".M2B0.fq")], k=k, solid=solid, canonical=canonical)


def sentinel(n):
    buf = np.zeros(n, api.KMER_DTYPE)
    buf.view(np.uint8)[:] = SENT
    return buf


def intact(buf, start=0):
    return bool((buf[start:].view(np.uint8) == SENT).all())


def assert_report(rep, M, max_list, n_partitions=None):
    """rep (api.KmerReport) == M (the model's dict, whose list is uncut)"""
    for k in km.SCALARS:
        want = M[k] if k != "n_partitions" or n_partitions is None else n_partitions
        assert getattr(rep, k) == want, k
    for k in km.ARRAYS:
        assert [int(v) for v in np.asarray(getattr(rep, k)).reshape(-1)] == M[k], k
    want = M["list"][:max_list]
    assert [(int(e["kmer"]), int(e["count_a"]), int(e["count_b"])) for e in rep.listed] == want
    assert rep.solid_lost == M["trans"][6] and rep.unchanged == (M["distinct_changed"] == 0)


def check_host(a, b, max_list=8, **kw):
    M = km.kmers([a], [b] if b is not None else None, **kw)
    buf = sentinel(max_list + 3)
    rep = api.fastq_kmers_host(a, b, max_list=max_list, list_out=buf, **kw)
    assert_report(rep, M, max_list)
    assert intact(buf, min(M["n_listed"], max_list))
    return rep, M


def test_struct_sizes():
    assert C.sizeof(_lib.KmerOpts) == 24 and C.sizeof(_lib.KmerEntry) == 16 and api.KMER_DTYPE.itemsize == 16
    assert C.sizeof(_lib.KmerReport) == 8 * (21 + 256 + 256 + 256 + 9 + 8)
    assert [k for k, _ in _lib.KmerReport._fields_][:21] == list(km.SCALARS)
    seg, run, starts = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    assert _lib.lib().bfq_kmers_geometry(C.byref(seg), C.byref(run), C.byref(starts)) == 0
    assert seg.value >= 256 and run.value >= 256 and starts.value >= 1


@pytest.mark.parametrize("name,k", sorted(RECORDED))
def test_model_reproduces_the_recorded_counts(name, k):
    M = golden_model(name, k)
    only_a_solid = sum(1 for v, x, y in M["list"] if y == 0)     # solid (>= 3) in A, absent from B
    got = (M["windows_a"], M["windows_b"], M["distinct_a"], M["distinct_b"], M["only_a"], only_a_solid, M["only_b"], M["distinct_changed"])
    assert got == RECORDED[(name, k)]
    assert only_a_solid == M["trans"][6]


@pytest.mark.parametrize("k", (8, 21, 31))
def test_model_paired_golden_is_unchanged(k):
    M = golden_model("paired", k)
    assert M["windows_a"] == M["windows_b"] and M["distinct_a"] == M["distinct_b"]
    assert (M["only_a"], M["trans"][6], M["only_b"], M["distinct_changed"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", (8, 20, 21, 31))
def test_host_goldens(name, k):
    a, b = golden(name), golden(name, ".M2B0.fq")
    for solid, canonical in ((3, True), (2, False)):
        M = golden_model(name, k, solid, canonical)
        buf = sentinel(40)
        rep = api.fastq_kmers_host(a, b, k=k, solid=solid, canonical=canonical, max_list=37, list_out=buf)
        assert_report(rep, M, 37)
        assert intact(buf, min(M["n_listed"], 37))
    assert_report(api.fastq_kmers_host(a, None, k=k), golden_model(name, k, single=True), 0)


def fq(seqs, eol=b"\n", last=True):
    t = b"".join(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * len(s) + eol for i, s in enumerate(seqs))
    return t if last else t[:-len(eol)]


def rc(s):
    return s.translate(km.COMP)[::-1]


def border_texts(k, rng):
    """(A, B) pairs at the borders of the definition for this k"""
    rnd = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    base = rnd(k + 40)
    lens = [rnd(n) for n in (0, k - 1, k, k + 1)]
    ns = [b"N" + rnd(k + 5), rnd(k + 5) + b"N", rnd(k) + b"N" + rnd(k), rnd(3) + b"N" + rnd(k) + b"N" + rnd(3), rnd(3) + b"N" + rnd(k - 1) + b"N" + rnd(k + 2)]
    lower = [base[:k + 3] + b"a" + base[k + 4:], base.lower(), rnd(k + 9) + b"R" + rnd(k)]
    diff = rnd(k - 1)
    strand = [diff + b"A", rc(diff + b"A"), diff + b"C", b"T" * 31, b"A" * 31, b"T" * k, b"A" * k]
    A = lens + ns + lower + strand + [base] * 3
    B = [base] * 3 + [rc(base), base[:-1] + (b"A" if base[-1:] != b"A" else b"C")] + ns[:2] + lens
    return [(fq(A), fq(B)), (fq(A, b"\r\n"), fq(B, b"\n", last=False)), (fq(A, last=False), fq([])), (fq([]), fq(B)), (b"", fq(B))]


@pytest.mark.parametrize("k", (8, 9, 20, 21, 31))
def test_host_borders(k):
    rng = np.random.default_rng(100 + k)
    for a, b in border_texts(k, rng):
        for canonical in (True, False):
            check_host(a, b, k=k, solid=2, canonical=canonical)
        check_host(a, None, k=k, solid=3)


def test_host_strand_and_palindrome():
    rng = np.random.default_rng(7)
    reads = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), int(n))) for n in rng.integers(25, 90, 60)]
    a = fq(reads)
    b = fq([rc(reads[i]) for i in rng.permutation(len(reads))])
    rep, _ = check_host(a, b, k=21)
    assert rep.unchanged and rep.distinct_a == rep.distinct_both
    rep, _ = check_host(a, b, k=21, canonical=False)
    assert not rep.unchanged
    rep, M = check_host(fq([b"ACGTACGT"]), None, k=8)
    assert (rep.windows_a, rep.distinct_a, int(rep.hist_a[1])) == (1, 1, 1)
    rep, M = check_host(fq([b"ACGTACGTACGT"]), None, k=8)        # ACGTACGT twice, and its two rotations, each its own reverse complement or not
    assert rep.windows_a == 5 and M["list"] == []


def test_host_long_runs_saturate_the_bins():
    read = b"ACGGTCATTGCAAGCTTAGGCTAACGTTAGCCATGCAATGC"[:40]
    a = fq([read] * 300)
    rep, M = check_host(a, fq([read] * 9), k=21, solid=3)
    assert int(rep.hist_a[255]) == rep.distinct_a > 0 and int(rep.joint[15, 9]) == rep.distinct_a
    rep, M = check_host(fq([b"A" * 5000]), None, k=21)
    assert (rep.distinct_a, rep.windows_a, int(rep.hist_a[255])) == (1, 4980, 1)


def test_host_partitions_are_reported():
    a, b = golden("synth_fix"), golden("synth_fix", ".M2B0.fq")
    for pr in (1, 1000, 30000):
        M = km.kmers([a], [b], k=21, part_records=pr)
        rep = api.fastq_kmers_host(a, b, k=21, part_records=pr)
        assert rep.n_partitions == M["n_partitions"] >= 3
        assert_report(rep, M, 0)


def raw_host(a, b, k=21, solid=3, reserved=0, cap=4):
    rep = _lib.KmerReport()
    C.memset(C.byref(rep), 0xFF, C.sizeof(rep))
    buf = sentinel(cap)
    O = _lib.KmerOpts(k=k, solid=solid, canonical=1, reserved=reserved, part_records=0)
    L = _lib.lib()
    rc_ = L.bfq_fastq_kmers_host(a, len(a), b, len(b) if b is not None else 0, C.byref(O), C.byref(rep), C.c_void_p(buf.ctypes.data), cap)
    return rc_, L.bfq_kmers_host_error().decode(), bytes(rep), buf


def test_host_refusals():
    a = fq([b"ACGTACGTACGTACGTACGTACGTACGTAAAC"] * 5)
    for kw in (dict(k=7), dict(k=32), dict(solid=1), dict(solid=16), dict(reserved=1)):
        rc_, msg, rep, buf = raw_host(a, a, **kw)
        assert rc_ == E_ARG and rep == bytes(len(rep)) and intact(buf), msg
    cases = ((a[:a.rindex(b"\n", 0, len(a) - 1) + 1], a, "A: ", "multiple of 4", E_ARG), (a, a.replace(b"IIII\n", b"III\n", 1), "B: ", "len(DNA) != len(QS)", E_ARG),
             (fq([b"A" * 65001]), a, "A: ", "BFQ_MAX_READ_LEN", E_TOO_LONG))
    for x, y, pre, words, code in cases:
        rc_, msg, rep, buf = raw_host(x, y)
        assert rc_ == code and msg.startswith(pre) and words in msg
        assert rep == bytes(len(rep)) and intact(buf)
        with pytest.raises(km.Malformed):
            km.kmers([x], [y])
    rc_, msg, rep, buf = raw_host(a, a)
    assert rc_ == 0 and msg == ""
