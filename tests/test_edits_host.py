"""The BFQEDIT1 container on the host (include/bfqzip_hip.h: bfq_edits_* and the two one-thread text forms) against the Python
model (tests/edits_model.py) and the reference-made goldens.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, _lib
from tests import edits_model as em, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("example", "paired", "synth_fix", "synth_var")
GOLDEN_EDITS = {"example": 10, "paired": 0, "synth_fix": 429, "synth_var": 598}   # changed bases against the reference's X.M2B0.fq


def golden_pair(name):
    rd = lambda f: open(os.path.join(util.GOLDEN, f), "rb").read()
    return rd(name + ".fastq"), rd(name + ".M2B0.fq")


def edits(E, bits, seed):
    """E ascending positions with gaps below 2^bits, their bytes, and a T above them"""
    rng = np.random.default_rng(seed)
    gaps = [int(x) >> (64 - bits) if bits else 0 for x in rng.integers(0, 1 << 63, E, dtype=np.uint64) * 2]
    pos, g = [], int(rng.integers(0, 3))
    for k in range(E):
        if k:
            g += 1 + gaps[k]
        pos.append(g)
    byt = [int(x) for x in rng.integers(33, 127, E)]
    return pos, byt, (pos[-1] + 1 + int(rng.integers(0, 3))) if E else 4


CASES = [(0, 5), (1, 5), (2, 0), (1023, 9), (1024, 9), (1025, 9), (2049, 3), (2049, 0), (1025, 33), (300, 44)]


@pytest.mark.parametrize("E,bits", CASES)
def test_host_encode_is_the_model_byte_for_byte(E, bits):
    pos, byt, T = edits(E, bits, 17 * E + bits)
    z = api.edits_encode(pos, byt, 12, T, 0x1234567890ABCDEF, 0xFEDCBA0987654321)
    assert z.tobytes() == em.encode(pos, byt, 12, T, 0x1234567890ABCDEF, 0xFEDCBA0987654321)
    assert len(z) <= api.edits_bound(E, T)
    d = api.edits_decode(z)
    assert list(d["pos"]) == pos and list(d["byte"]) == byt
    assert (d["n_reads"], d["total_bases"], d["n_edits"], d["shape"], d["target_sum"]) == (12, T, E, 0x1234567890ABCDEF, 0xFEDCBA0987654321)
    m = em.decode(z.tobytes())
    assert m["pos"] == pos and m["byte"] == byt
    assert api.edits_info(z) == dict(n_reads=12, total_bases=T, n_edits=E, members=1)


def test_the_empty_container_is_64_bytes_and_all_consecutive_edits_need_no_gap_words():
    z = api.edits_encode([], [], 0, 0, 0, 0)
    assert len(z) == 64 and z.tobytes() == em.encode([], [], 0, 0, 0, 0)
    pos = list(range(7, 7 + 2049))
    z = api.edits_encode(pos, [65] * 2049, 1, 4000, 0, 0)
    assert len(z) == 64 + 8 * 3 + 8 + 0 + 2056 and bytes(z[64 + 24:64 + 27]) == b"\0\0\0"      # w = 0 three times
    # a segment of one edit: its `first` alone
    z = api.edits_encode(pos[:1025], [65] * 1025, 1, 4000, 0, 0)
    assert len(z) == 64 + 16 + 8 + 0 + 1032 and struct.unpack_from("<Q", z.tobytes(), 72)[0] == 7 + 1024


def test_gaps_up_to_two_to_the_55_take_the_widest_entries():
    pos = [3, 3 + (1 << 55) + 1, 3 + (1 << 55) + 2, (1 << 56) - 1]
    z = api.edits_encode(pos, [65, 67, 71, 84], 1, 1 << 56, 0, 0)
    assert z.tobytes() == em.encode(pos, [65, 67, 71, 84], 1, 1 << 56, 0, 0) and z[64 + 8] == 56
    assert [int(v) for v in api.edits_decode(z)["pos"]] == pos
    with pytest.raises(api.EditsError):
        api.edits_encode([0], [65], 1, (1 << 56) + 1, 0, 0)


def test_encode_refuses_what_is_no_edit_list_and_writes_nothing():
    L = _lib.lib()
    for pos, byt, T in (([5, 5], [65, 65], 10), ([5, 4], [65, 65], 10), ([5, 10], [65, 65], 10), ([5, 6], [65, 32], 10), ([5, 6], [127, 65], 10)):
        p, b = np.array(pos, np.uint64), np.array(byt, np.uint8)
        out = np.full(256, 0xEE, np.uint8)
        ol = C.c_uint64(3)
        assert L.bfq_edits_encode(api._ptr(p), api._ptr(b), 2, 1, T, 0, 0, api._ptr(out), 256, C.byref(ol)) == -1 and ol.value == 0 and (out == 0xEE).all()
    p, b = np.array([1, 2, 3], np.uint64), np.array([65, 65, 65], np.uint8)
    out = np.full(256, 0xEE, np.uint8)
    assert L.bfq_edits_encode(api._ptr(p), api._ptr(b), 3, 1, 9, 0, 0, api._ptr(out), 64 + 8 + 8 + 8 - 1, None) == -1 and (out == 0xEE).all()
    assert L.bfq_edits_encode(api._ptr(p), api._ptr(b), 3, 1, 9, 0, 0, api._ptr(out), 64 + 8 + 8 + 8, None) == 0


def malformed():
    """(name, bytes, first_bad or None) -- every way the header says a member can be wrong"""
    pos, byt, T = edits(2500, 9, 99)
    good = em.encode(pos, byt, 3, T, 5, 6)
    nseg, off_w = 3, 64 + 24
    off_g = off_w + 8
    off_b = len(good) - em.pad8(2500)
    put = lambda z, at, b: z[:at] + b + z[at + len(b):]
    yield "magic", put(good, 0, b"X"), None
    yield "S", put(good, 32, struct.pack("<I", 512)), None
    yield "flags", put(good, 36, b"\1"), None
    yield "more edits than bases", put(good, 16, struct.pack("<Q", 2499)), None
    yield "T above 2^56", put(good, 16, struct.pack("<Q", (1 << 56) + 1)), None
    yield "a byte too many", good + b"\0", None
    yield "a byte too few", good[:-1], None
    yield "payload stated too small", put(good, 56, struct.pack("<Q", len(good) - 64 - 8)), None
    yield "cut in the header", good[:40], None
    yield "table padding", put(good, off_w + nseg, b"\1"), None
    yield "bytes padding", put(good, off_b + 2500, b"\1"), None
    yield "width above 56", put(good, off_w + 2, bytes([57])), 2048
    yield "byte 32", put(good, off_b + 1500, b" "), 1500
    yield "byte 127", put(good, off_b + 7, b"\x7f"), 7
    yield "two bad bytes", put(put(good, off_b + 2499, b"\n"), off_b + 30, b"\n"), 30
    yield "position >= T", put(good, 16, struct.pack("<Q", pos[2000])), 2000
    yield "first[1] not above the edit before it", put(good, 64 + 8, struct.pack("<Q", pos[1023])), 1024
    yield "first[2] far below", put(good, 64 + 16, struct.pack("<Q", 0)), 2048
    yield "first[0] at T", put(good, 64, struct.pack("<Q", T)), 0
    # a width that is not canonical (every gap written a bit wider), and set padding bits in a segment's last word
    p2, b2 = pos[:100], byt[:100]
    w = max(p2[j + 1] - p2[j] - 1 for j in range(99)).bit_length()
    yield "a width that is not canonical", em.encode(p2, b2, 3, T, 5, 6, widths={0: w + 1}), 0
    g2 = em.encode(p2, b2, 3, T, 5, 6)
    assert (99 * w) % 64
    yield "gap padding bits", put(g2, len(g2) - 104 - 1, bytes([g2[len(g2) - 104 - 1] | 0x80])), 0
    p3 = pos[:1100]
    z3 = em.encode(p3, byt[:1100], 3, T, 5, 6, widths={1: 12})
    yield "a later segment's width", z3, 1024


@pytest.mark.parametrize("name,z,want", list(malformed()), ids=[m[0].replace(" ", "_") for m in malformed()])
def test_every_malformation_is_refused_with_its_first_offending_edit(name, z, want):
    with pytest.raises(em.Malformed) as m:
        em.decode(z)
    assert m.value.first_bad == (em.NOPOS if want is None else want)
    L = _lib.lib()
    a = np.frombuffer(z, np.uint8)
    p, b = np.full(4096, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(4096, 0xA5, np.uint8)
    v = [C.c_uint64(77) for _ in range(5)]
    bad = C.c_uint64(5)
    rc = L.bfq_edits_decode(api._ptr(a), len(a), api._ptr(p), api._ptr(b), 4096, *[C.byref(x) for x in v], C.byref(bad))
    assert rc == -1 and bad.value == (em.NOPOS if want is None else want)
    assert (p == 0xA5A5A5A5A5A5A5A5).all() and (b == 0xA5).all() and all(x.value == 77 for x in v)
    with pytest.raises(api.EditsError) as e:
        api.edits_decode(a)
    assert e.value.first_bad == want


def seq_lines(text):
    return bytes(text).split(b"\n")[1::4]


@pytest.mark.parametrize("name", NAMES)
def test_the_goldens_edits_and_the_way_back(name):
    """The expectation comes from the reference-made fixtures: X.M2B0.fq differs from X.fastq in 10 / 0 / 429 / 598 bases;
    with the edits applied it has X.fastq's sequence lines and every other byte of its own."""
    a, b = golden_pair(name)
    z, st = api.fastq_edits_host(a, b)
    assert st.edits == GOLDEN_EDITS[name] == api.edits_info(z)["n_edits"]
    assert z.tobytes() == em.container(a, b)
    d = api.edits_decode(z)
    la, lb = seq_lines(a), seq_lines(b)
    assert sum(x != y for s, t in zip(la, lb) for x, y in zip(s, t)) == GOLDEN_EDITS[name]
    assert st.reads == len(la) == d["n_reads"] and st.bases == sum(map(len, la)) == d["total_bases"] and st.bytes == len(z)
    assert st.reads_touched == sum(s != t for s, t in zip(la, lb))
    back, st2 = api.fastq_unedit_host(b, z)
    back = back.tobytes()
    assert st2.edits == st.edits and st2.reads_touched == st.reads_touched
    lines, want = back.split(b"\n"), b.split(b"\n")
    assert lines[1::4] == la
    want[1::4] = la
    assert lines == want
    assert back == em.apply(b, z.tobytes())


def test_members_back_to_back_accumulate():
    a1, b1 = golden_pair("example")
    a2, b2 = golden_pair("synth_var")
    z1, z2 = api.fastq_edits_host(a1, b1)[0], api.fastq_edits_host(a2, b2)[0]
    zz = np.concatenate([z1, z2, z1])
    info = api.edits_info(zz)
    assert info == dict(n_reads=100 + 2000 + 100, total_bases=10100 + 89495 + 10100, n_edits=10 + 598 + 10, members=3)
    assert [len(m) for m in api.edits_members(zz)] == [len(z1), len(z2), len(z1)]
    back, st = api.fastq_unedit_host(b1 + b2 + b1, zz)
    assert seq_lines(back.tobytes()) == seq_lines(a1 + a2 + a1) and st.edits == 618
    assert back.tobytes() == em.apply(b1 + b2 + b1, zz.tobytes())
    with pytest.raises(api.EditsError):                              # a member is missing
        api.fastq_unedit_host(b1 + b2 + b1, zz[:len(z1) + len(z2)])
    with pytest.raises(api.EditsError):                              # the blocks in another order: shape
        api.fastq_unedit_host(b2 + b1 + b1, zz)
    with pytest.raises(api.EditsError) as e:
        api.edits_info(np.concatenate([z1, z2[:-8]]))
    assert "member 1" in str(e.value)


def test_the_host_text_forms_refuse_and_write_nothing():
    rec = lambda i, s: b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s))
    a = b"".join(rec(i, b"ACGT" * 5) for i in range(12))
    b = b"".join(rec(i, b"ACGT" * 4 + (b"AAGT" if i % 3 == 0 else b"ACGT")) for i in range(12))
    z, st = api.fastq_edits_host(a, b)
    assert st.edits == 4 and st.reads_touched == 4
    out = np.full(len(a) + 8, 0xEE, np.uint8)

    def refused(call, *words):
        with pytest.raises(api.EditsError) as e:
            call()
        assert (out == 0xEE).all()
        for w in words:
            assert w in str(e.value), str(e.value)
    refused(lambda: api.fastq_edits_host(a, b[:len(b) - len(rec(11, b"ACGT" * 5))], out=out), "12 in A", "11 in B")
    longer = b"".join(rec(i, b"ACGT" * 5 + (b"A" if i in (5, 9) else b"")) for i in range(12))
    refused(lambda: api.fastq_edits_host(a, longer, out=out), "read 5", "20 bases in A and 21 in B")
    refused(lambda: api.fastq_edits_host(a, b, out=out[:len(z) - 1]), "needs")
    refused(lambda: api.fastq_unedit_host(a, z, out=out), "not the output these edits were made from")          # applied to the INPUT
    other = b"".join(rec(i, b"ACGT" * 4 + b"AAGT") for i in range(12))[:-1]
    z2 = api.fastq_edits_host(longer, longer)[0]
    refused(lambda: api.fastq_unedit_host(b, z2, out=out), "bases")                                                # another collection
    shuffled = b"".join(rec(i, b"ACGT" * (4 if i == 0 else 6 if i == 1 else 5)) for i in range(12))
    z3 = api.fastq_edits_host(shuffled, shuffled)[0]
    refused(lambda: api.fastq_unedit_host(b, z3, out=out), "shape")                                                # same N and T, other lengths
    bad = z.copy(); bad[len(bad) - 8 + 2] = 10
    refused(lambda: api.fastq_unedit_host(b, bad, out=out), "edit 2")
    refused(lambda: api.fastq_unedit_host(b, z, out=out[:len(b) - 1]), "needs")
    del other
    tab = a.replace(b"ACGTACGTACGTACGTACGT\n+\nI", b"ACGTACGTACGTACGTAC\tT\n+\nI", 1)
    refused(lambda: api.fastq_edits_host(tab, a, out=out), "outside 33..126")


def test_member_counts_that_wrap_are_refused_before_they_size_anything():
    """N is bounded by nothing in a member: two members whose read counts add up to the text's only mod 2^64 (and one that
    alone claims more reads than there are) are refused, nothing is written, and info's sums saturate"""
    rec = lambda i, s: b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s))
    empty = b"".join(rec(i, b"") for i in range(6))                       # six empty reads: T = 0, so only N can tell
    M = (1 << 64) - 1
    out = np.full(len(empty) + 8, 0xEE, np.uint8)
    for ns in ((M, 7), (M - 1, 8), (7,), (M,), (3, M, 4)):
        z = b"".join(em.encode([], [], n, 0, em.shape_of([0] * min(n, 6)), 0) for n in ns)
        with pytest.raises(api.EditsError) as e:
            api.fastq_unedit_host(empty, z, out=out)
        assert e.value.code == -1 and (out == 0xEE).all(), ns
    assert api.edits_info(em.encode([], [], M, 0, 0, 0) + em.encode([], [], 7, 0, 0, 0))["n_reads"] == M
    z = em.encode([], [], 2, 0, em.shape_of([0, 0]), 0) + em.encode([], [], 4, 0, em.shape_of([0] * 4), 0)
    assert api.fastq_unedit_host(empty, z, out=out)[0].tobytes() == empty  # the honest split of the same six reads


def test_library_declares_and_exports_the_edits_calls():
    header = open(os.path.join(ROOT, "include", "bfqzip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(bfq_(?:edits_\w+|fastq_(?:un)?edit\w*))\s*\(", header))
    assert declared == {"bfq_edits_bound", "bfq_edits_member_len", "bfq_edits_info", "bfq_edits_encode", "bfq_edits_decode", "bfq_edits_host_error",
                        "bfq_fastq_edits_host", "bfq_fastq_unedit_host", "bfq_edits_make_device", "bfq_edits_apply_device", "bfq_fastq_edits",
                        "bfq_fastq_edits_device", "bfq_fastq_edits_fd", "bfq_fastq_unedit", "bfq_fastq_unedit_fd"}
    L = _lib.lib()
    for s in declared:
        assert s in _lib.SYMBOLS and getattr(L, s) is not None
    assert C.sizeof(_lib.EditStats) == 40
    # the job keeps its size: what the edits need travels beside it
    assert C.sizeof(_lib.FastqJob) == _lib.FastqJob.reserved1.offset + 4 and C.sizeof(_lib.JobEdits) == 24
    assert "bfq_fastq_run_job_edits" in _lib.SYMBOLS and L.bfq_fastq_run_job_edits is not None


def test_host_forms_as_a_program_under_sanitizers(tmp_path):
    """tests/cxx/test_edits.cpp: bfq_edits.h and bfq_edits_host.cpp compiled for the host with -fsanitize=address,undefined and
    run as a program of its own -- exact-size heap buffers, so a byte read or written beside a member, an edit list or a
    text ends the run."""
    exe = str(tmp_path / "test_edits")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_edits.cpp"), os.path.join(ROOT, "bfqzip_amd", "csrc", "bfq_edits_host.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
