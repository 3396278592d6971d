"""Host side of the unaligned BAM output (csrc/bfq_ubam.h): the host form (HostText.fastq_to_bam_host) against the
plain-Python statement of the definition (tests/ubam_model.py) -- stream, statistics and every refusal's message --, the
size arithmetic, the way back through the host form of the BAM input, and the same code compiled for the host with
sanitizers and run as a program of its own."""
import os
import struct
import subprocess
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import bam_model as M
from tests import ubam_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


@pytest.mark.parametrize("name", U.NAMES)
def test_host_form_equals_the_model(name):
    texts, opts = U.cases()[name]
    want, wst = U.expect(name)
    got, st = host.fastq_to_bam_host(texts, **opts)
    assert got.tobytes() == want, name
    assert st.as_dict() == wst, name
    buf = np.full(len(want) + 64, 0xA5, np.uint8)                  # into a guarded buffer of the exact size
    got, st = host.fastq_to_bam_host(texts, out=buf[32:32 + len(want)], **opts)
    assert got.tobytes() == want and (buf[:32] == 0xA5).all() and (buf[32 + len(want):] == 0xA5).all(), name


def records(stream):
    """(name, flag, l_seq, the record's size) of every record of a stream without references"""
    l_text = struct.unpack_from("<i", stream, 4)[0]
    assert stream[:4] == b"BAM\1" and struct.unpack_from("<i", stream, 8 + l_text)[0] == 0
    o, out = 12 + l_text, []
    while o < len(stream):
        bs, ref, pos, ln, mapq, bin_, nc, flag, lseq, nref, npos, tlen = struct.unpack_from("<IiiBBHHHIiii", stream, o)
        assert (ref, pos, mapq, bin_, nc, nref, npos, tlen) == (-1, -1, 0, 4680, 0, -1, -1, 0)
        out.append((stream[o + 36:o + 36 + ln - 1], flag, lseq, bs + 4))
        o += 4 + bs
    assert o == len(stream)
    return out


@pytest.mark.parametrize("name", ("edges", "edges-rg", "lanes", "pairs+0-rg", "pairs-header", "unnamed", "long"))
def test_measure_arithmetic(name):
    """a record is 36 + (l_name + 1) + ceil(l_seq / 2) + l_seq bytes, + 4 + len(rg_id); the header as stated; members"""
    texts, opts = U.cases()[name]
    got, st = host.fastq_to_bam_host(texts, **opts)
    s = got.tobytes()
    rg = opts.get("rg_id")
    text = opts["header_text"] if "header_text" in opts else U.DEFAULT_HEADER + (b"@RG\tID:" + rg + b"\n" if rg else b"")
    assert s.startswith(M.header(text))
    recs = records(s)
    for nm, flag, lseq, size in recs:
        assert size == 36 + len(nm) + 1 + (lseq + 1) // 2 + lseq + (4 + len(rg) if rg else 0)
    n = [len(U.lines_of(t)) // 4 if t is not None else 0 for t in texts]
    assert [f for _, f, _, _ in recs] == [77, 141] * n[1] + [4] * n[0]
    assert st.raw_len == len(s) == len(M.header(text)) + sum(r[3] for r in recs) and st.members == -(-len(s) // 65280) + 1
    assert st.records == len(recs) and list(st.written) == n


def test_names():
    texts, _ = U.cases()["edges-as-mates"]
    names = [r[0] for r in records(host.fastq_to_bam_host(texts)[0].tobytes())]
    want = [h for h, *_ in U.edge_reads()]
    at = lambda h: 2 * want.index(h)
    assert names[at(b"/1")] == b"/1" and names[at(b"/1") + 1] == b"/1"               # exactly the suffix: it stays
    assert names[at(b"a/1")] == b"a" and names[at(b"a/1") + 1] == b"a/1"             # only the matching suffix goes
    assert names[at(b"a/2")] == b"a/2" and names[at(b"a/2") + 1] == b"a"
    assert names[at(b"a/1/1")] == b"a/1" and names[at(b"b/3")] == b"b/3"
    i = want.index(b"")
    assert names[2 * i] == names[2 * i + 1] == b"%d" % (i + 1)                       # both mates share their number
    assert names[at(b"n" * 254)] == b"n" * 254 and names[at(b"blank 1:N:0:ACGT")] == b"blank" and names[at(b"tab\tBC:Z:AC GT")] == b"tab"
    kept = [r[0] for r in records(host.fastq_to_bam_host(texts, mate_suffix=0)[0].tobytes())]
    assert kept[at(b"a/1")] == b"a/1" and kept[at(b"a/2") + 1] == b"a/2"
    texts, opts = U.cases()["unnamed"]
    names = [r[0] for r in records(host.fastq_to_bam_host(texts, **opts)[0].tobytes())]
    assert names == [b"%d" % (i // 2 + 1) for i in range(80)] + [b"%d" % (41 + i) for i in range(7)]
    st = host.fastq_to_bam_host(texts, **opts)[1]
    assert st.named == 87 and st.comments_dropped == 0
    st = host.fastq_to_bam_host(*U.cases()["pairs+0"][:1])[1]
    assert st.comments_dropped == 607 and st.named == 0


@pytest.mark.parametrize("name", ("edges", "lanes", "pairs+0", "many"))
def test_back_through_the_bam_input(name):
    """bam_to_fastq of the stream gives the normalised texts back: the first word of the name, upper-case bases, a bare '+'"""
    texts, opts = U.cases()[name]
    got, st = host.fastq_to_bam_host(texts, **opts)
    back = host.bam_to_fastq_host(got, split=1)[0]
    for k in range(3):
        assert back[k].tobytes() == (U.normalised(texts[k], k, pairs=st.written[1]) if texts[k] is not None else b""), (name, k)


def test_ubam_of_the_bam_model_comes_back():
    """fastq_to_bam of the texts bam_to_fastq wrote from bam_model's a-ubam case equals that case's stream in every field
    but the tags (its records carry RG and XB tags, which no text holds; its qualities are <= 93 and present)"""
    c = M.good()["a-ubam"]
    recs = [r for r in c.recs if not r.flag & 0x900]
    texts = host.bam_to_fastq_host(c.stream, exclude_flags=0x900)[0]
    got, st = host.fastq_to_bam_host([texts[0].tobytes()], header_text=b"")
    # every kept record went to text 0 with its mate suffix; as text 0 it keeps the suffix and gets flag 4: compare SEQ and QUAL
    want = M.header(b"") + b"".join(M.encode(M.rec(r.name + ((b"/1", b"/2")[M.mate(r.flag) - 1] if M.mate(r.flag) else b""), 4,
                                                         r.seq if not r.flag & 16 else bytes(M.COMP[M.SEQ.index(ch)] for ch in reversed(r.seq)),
                                                         r.qual if not r.flag & 16 else r.qual[::-1])) for r in recs)
    assert got.tobytes() == want and st.records == len(recs) and st.unknown_bases == 0
    # split into mates, forward records only, without tags: the stream itself
    plain = [r._replace(aux=b"") for r in M.paired(60)]
    case = M.Case(plain, text=b"@HD\tVN:1.6\tSO:unsorted\n")
    t = host.bam_to_fastq_host(case.stream, split=1)[0]
    got, _ = host.fastq_to_bam_host([None, t[1].tobytes(), t[2].tobytes()], paired_check=1)
    assert got.tobytes() == case.stream


def test_refusals_carry_the_models_message_and_write_nothing():
    for name, (texts, opts, code, msg) in U.refusals().items():
        buf = np.full(1 << 18, 0xA5, np.uint8)
        with pytest.raises(api.BfqError) as e:
            host.fastq_to_bam_host(texts, out=buf[32:-32], **opts)
        assert e.value.code == code and str(e.value).endswith(msg), (name, str(e.value), msg)
        assert (buf == 0xA5).all(), name
    assert U.refusals()["first-of-three"][3] == "FASTQ to BAM: text 2 read 9: the third line does not begin with '+'"
    assert U.refusals()["name-255"][3] == "FASTQ to BAM: text 0 read 40: name longer than 254 bytes"
    assert U.refusals()["too-long"][2] == -5 and U.refusals()["qual-32"][3].endswith("a quality byte outside [33, 126]")
    texts, opts = U.cases()["pairs"]
    want = U.expect("pairs")[0]
    buf = np.full(len(want) + 63, 0xA5, np.uint8)                  # one byte short
    with pytest.raises(api.BfqError) as e:
        host.fastq_to_bam_host(texts, out=buf[32:32 + len(want) - 1], **opts)
    assert e.value.code == -1 and e.value.needed == len(want) and (buf == 0xA5).all()


def test_ubam_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_ubam")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_ubam.cpp")])
    lines, n = [], [0]

    def put(data):
        n[0] += 1
        p = str(tmp_path / ("f%d" % n[0]))
        with open(p, "wb") as f:
            f.write(data if data is not None else b"")
        return p if data is not None else "-"

    def words(texts, o):
        return "%s %s %s %d %d %d %s %s" % (put(texts[0]), put(texts[1]), put(texts[2]), o.get("mate_suffix", 1), o.get("paired_check", 0), o.get("level", 1),
                                            put(o.get("header_text")), put(o.get("rg_id")))

    for name in U.NAMES:
        texts, opts = U.cases()[name]
        want, st = U.expect(name)
        lines.append("good %s %s %d %d %d" % (words(texts, opts), put(want), st["named"], st["comments_dropped"], st["unknown_bases"]))
    for name, (texts, opts, code, msg) in U.refusals().items():
        lines.append("bad %s %s %d" % (words(texts, opts), put(msg.encode()), code))
    man = put(("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert b"%d cases, 0 failures" % len(lines) in r.stdout


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_ubam_default_opts", "bfq_fastq_to_bam_measure", "bfq_fastq_to_bam_host", "bfq_ubam_host_error", "bfq_fastq_to_bam_device",
              "bfq_fastq_to_bam", "bfq_fastq_to_bam_fd", "bfq_fastq_restore_bam_fd"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.UbamOpts) == 40 and C.sizeof(_lib.UbamStats) == 72
    o = _lib.UbamOpts()
    L.bfq_ubam_default_opts(C.byref(o))
    assert (o.mate_suffix, o.paired_check, o.level, o.reserved, o.header_text, o.header_len, o.rg_id) == (1, 0, 1, 0, None, 0, None)


def test_driver_and_api_refuse_before_any_work(tmp_path):
    """--ubam-out together with --bam-out: exit status 1 before an engine exists, nothing written"""
    from bfqzip_amd import parallel
    fq, out = str(tmp_path / "in.fastq"), str(tmp_path / "o" / "OUT")
    os.mkdir(str(tmp_path / "o"))
    with open(fq, "wb") as f:
        f.write(U.cases()["lanes"][0][0])
    assert parallel.main([fq, "-o", out, "-t", "2", "--ubam-out", str(tmp_path / "o" / "u.bam"), "--bam-out", str(tmp_path / "o" / "o.bam")]) == 1
    assert parallel.main([fq, "-o", out, "-t", "2", "--ubam-out", str(tmp_path / "o" / "u.bam"), "--streams-only", "--m2"]) == 1
    assert os.listdir(str(tmp_path / "o")) == []
