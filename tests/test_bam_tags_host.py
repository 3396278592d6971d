"""Host side of the aux tags in FASTQ header lines (csrc/bfq_bam.h, csrc/bfq_ubam.h): the host forms with the tag
extension (bfq_bam_tag_opts, bfq_ubam_tag_opts) against the plain-Python statement of the definition
(tests/bam_tags_model.py) -- texts, stream, statistics, tag counts and every refusal's message --, the measure arithmetic,
the identity BAM -> text -> BAM, the untouched structures and defaults, and the same code compiled for the host with
sanitizers and run as a program of its own."""
import os
import struct
import subprocess
import ctypes as C
import numpy as np
import pytest
from bfqzip_amd import _lib, api, parallel
from tests import bam_model as M
from tests import bam_tags_model as T
from tests import ubam_model as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


def split_opts(o):
    """(the keywords of the host form, those of the model) of an option set of the way in"""
    kw = {k: v for k, v in o.items() if k not in ("tags", "strict")}
    return dict(kw, tags=o["tags"], strict_tags=o.get("strict", 0)), kw


@pytest.mark.parametrize("opts", T.WAY_IN_OPTS, ids=[str(i) for i in range(len(T.WAY_IN_OPTS))])
def test_way_in_equals_the_model(opts):
    recs = T.way_in_recs()
    stream = M.Case(recs, raw=True).stream
    call, model = split_opts(opts)
    want, wst, wts = T.expected(recs, opts["tags"], **model)
    for piece in T.PIECES:
        got, st = host.bam_to_fastq_host(stream, piece=piece, **call)
        assert [g.tobytes() for g in got] == want, (opts, piece)
        assert st.tags.as_dict() == wts and {k: st.as_dict()[k] for k in wst} == wst, (opts, piece)
    plain, pst = host.bam_to_fastq_host(stream, **model)              # reserved 0: the untagged model's bytes
    assert [g.tobytes() for g in plain] == M.expected(recs, **model)[0] and pst.tags is None
    bufs = [np.full(len(w) + 64, 0xA5, np.uint8) for w in want]     # into guarded buffers of the exact size
    got, _ = host.bam_to_fastq_host(stream, outs=[b[32:32 + len(w)] for b, w in zip(bufs, want)], **call)
    assert [g.tobytes() for g in got] == want and all((b[:32] == 0xA5).all() and (b[32 + len(w):] == 0xA5).all() for b, w in zip(bufs, want))


@pytest.mark.parametrize("name", T.REPAIRED)
def test_way_in_on_a_repaired_chain(name):
    """a carrier whose B array holds well-formed records at a piece boundary: a walker starts inside the tag area, the chain
    walks the piece again, and the tag counts are those of the chain's pieces alone"""
    c = M.good()[name]
    want, _, wts = T.expected(c.recs, "*")
    repaired = 0
    for piece in T.PIECES:
        got, st = host.bam_to_fastq_host(c.stream, piece=piece, tags="*")
        assert [g.tobytes() for g in got] == want and st.tags.as_dict() == wts, (name, piece)
        repaired += st.repaired
    assert repaired == 2 and wts["tags_dropped"] > 0


def test_way_in_measure_arithmetic():
    """a kept record is l_read_name + 2 l_seq + 5 bytes of text, + 2 with a suffix, + tag_bytes; a tag is 6 bytes and its value"""
    recs = T.way_in_recs()
    stream = M.Case(recs, raw=True).stream
    (plain, _, _), pst = host.bam_to_fastq_host(stream)
    (text, _, _), st = host.bam_to_fastq_host(stream, tags="*")
    assert len(text) == len(plain) + st.tags.tag_bytes and st.as_dict() == pst.as_dict()
    fields = [f for line in text.tobytes().split(b"\n")[0::4] for f in line.split(b"\t")[1:]]
    assert len(fields) == st.tags.tags_written and sum(len(f) + 1 for f in fields) == st.tags.tag_bytes
    assert b"\tI0:i:-128\tJ0:i:127\n" in text.tobytes() and b"\tI5:i:0\tJ5:i:4294967295\n" in text.tobytes()
    assert b"\tI4:i:-2147483648\tJ4:i:2147483647\n" in text.tobytes() and b"\tXA:A:q\tXH:H:0aF9\tXS:A: \tXE:H:\n" in text.tobytes()
    # the reservation: no tag is more than 5/2 of its stored bytes as text
    for aux, n in ((T.aux_int(b"XC", b"c", -128), 10), (T.aux_int(b"XC", b"s", -32768), 12), (T.aux_int(b"XC", b"i", -(1 << 31)), 17), (M.aux_z(b"XZ", b""), 6)):
        assert len(T.tag_text(*T.parse_tags(aux)[0])) == n and 2 * n <= 5 * len(aux)


def test_way_in_refusals_write_nothing():
    cases = dict((k, (v, 0)) for k, v in T.bad_tag_recs().items())
    cases["strict"] = (T.strict_recs(), 1)
    for name, (recs, strict) in cases.items():
        stream = M.Case(recs, raw=True).stream
        with pytest.raises(T.Refused) as w:
            T.expected(recs, "*", strict=strict)
        for piece in T.PIECES:
            bufs = [np.full(1 << 17, 0xA5, np.uint8) for _ in range(3)]
            with pytest.raises(api.BfqError) as e:
                host.bam_to_fastq_host(stream, outs=bufs, piece=piece, tags="*", strict_tags=strict)
            assert e.value.code == w.value.code and str(e.value).endswith(w.value.msg), (name, piece, str(e.value), w.value.msg)
            assert all((b == 0xA5).all() for b in bufs), name
        host.bam_to_fastq_host(stream, strict_tags=1)               # with tags off nothing new is checked
        if not strict:
            host.bam_to_fastq_host(stream, tags="*", exclude_flags=0x940)       # ... and an excluded record is not looked at
    at = 12 + sum(len(M.encode(r)) for r in T.way_in_recs()[:T.BAD_AT])
    assert w.value.msg == "BAM tags: record 150 at byte %d: tag XF of type f cannot be carried" % at
    with pytest.raises(T.Refused) as w:
        T.expected(T.bad_tag_recs()["z-without-nul"], "*")
    assert w.value.msg == "damaged BAM input: record 150 at byte %d: malformed tag area" % at


@pytest.mark.parametrize("name", T.WAY_OUT_NAMES)
def test_way_out_equals_the_model(name):
    texts, opts = T.way_out_cases()[name]
    want, wst, wts = T.expect_out(name)
    got, st = host.fastq_to_bam_host(texts, **opts)
    assert got.tobytes() == want and st.as_dict() == wst and st.tags.as_dict() == wts, name
    buf = np.full(len(want) + 64, 0xA5, np.uint8)
    got, st = host.fastq_to_bam_host(texts, out=buf[32:32 + len(want)], **opts)
    assert got.tobytes() == want and (buf[:32] == 0xA5).all() and (buf[32 + len(want):] == 0xA5).all(), name
    plain = {k: v for k, v in opts.items() if k != "tags"}          # reserved 0: the untagged model's bytes
    got, st = host.fastq_to_bam_host(texts, **plain)
    assert got.tobytes() == U.convert(texts, **plain)[0] and st.tags is None, name
    short = np.full(len(want) + 63, 0xA5, np.uint8)
    if len(want) > len(M.header(U.DEFAULT_HEADER)) + 64:
        with pytest.raises(api.BfqError) as e:
            host.fastq_to_bam_host(texts, out=short[32:32 + len(want) - 1], **opts)
        assert e.value.needed == len(want) and (short == 0xA5).all()


def tags_of(stream):
    """the tag areas of the records of a stream without references"""
    o, out = 12 + struct.unpack_from("<i", stream, 4)[0], []
    while o < len(stream):
        bs, ln, lseq = struct.unpack_from("<I", stream, o)[0], stream[o + 12], struct.unpack_from("<I", stream, o + 20)[0]
        out.append(stream[o + 36 + ln + (lseq + 1) // 2 + lseq:o + 4 + bs])
        o += 4 + bs
    return out


def test_way_out_measure_arithmetic():
    """an integer is stored at the smallest width; no field is longer stored than written; the stream grows by tag_bytes"""
    texts, opts = T.way_out_cases()["shapes"]
    got, st = host.fastq_to_bam_host(texts, **opts)
    plain, pst = host.fastq_to_bam_host(texts)
    assert st.raw_len == pst.raw_len + st.tags.tag_bytes
    areas = tags_of(got.tobytes())
    ints = next(a for a in areas if a.startswith(b"I0C"))
    want = b"".join(T.aux_int(b"I%d" % (j % 10) if j < 10 else b"J%d" % (j - 10), ty, v) for j, (ty, v) in enumerate(zip(
        (b"C", b"C", b"S", b"S", b"I", b"I", b"c", b"c", b"s", b"s", b"i", b"i"), T.INTS)))
    assert ints == want
    over = next(a for a in areas if a.startswith(b"OK"))
    assert over == T.aux_int(b"OK", b"C", 0) + T.aux_int(b"OL", b"C", 7)           # both out of range dropped; "-0" and "007" taken
    assert next(a for a in areas if b"fine" in a) == M.aux_z(b"OK", b"fine")      # every malformed field dropped
    for field in (b"XX:A:c", b"XX:i:0", b"XX:i:256", b"XX:i:65536", b"XX:i:-1", b"XX:i:-129", b"XX:i:-32769", b"XX:Z:", b"XX:H:00"):
        assert len(T.field_tag(field, [], False)) <= len(field) + 1
    rg, _ = host.fastq_to_bam_host(texts, tags="*", rg_id="given")
    assert all(a.endswith(M.aux_z(b"RG", b"given")) and a.count(b"RGZ") == 1 for a in tags_of(rg.tobytes()))
    assert any(M.aux_z(b"RG", b"fromtext") in a for a in areas)


@pytest.mark.parametrize("paired", (0, 1))
def test_identity_bam_text_bam(paired):
    recs = T.identity_recs(paired)
    case = M.Case(recs, text=T.IDENTITY_HEADER, raw=True)
    t, st = host.bam_to_fastq_host(case.stream, tags="*", split=1)
    texts = [None, t[1].tobytes(), t[2].tobytes()] if paired else [t[0].tobytes()]
    back, st2 = host.fastq_to_bam_host(texts, tags="*", header_text=T.IDENTITY_HEADER, paired_check=paired)
    assert back.tobytes() == case.stream
    assert st.tags.tags_dropped == 0 and st2.tags.fields_dropped == 0 and st2.comments_dropped == 0 and st.tags.tags_written == st2.tags.tags_written
    again, _ = host.bam_to_fastq_host(back, tags="*", split=1)       # text -> BAM -> text
    assert [a.tobytes() for a in again] == [a.tobytes() for a in t]
    # the same through the patch with the names compared: the tagged header lines meet their records
    patched, pst = host.bam_patch_host(case.stream, texts, split=1, check_names=1, tags="*")
    assert patched.tobytes() == case.stream and pst.reads_changed == 0


def test_refused_lists_and_untouched_structures():
    L = _lib.lib()
    stream = M.Case(T.way_in_recs()[:4], raw=True).stream
    for make, call in ((_lib.BamTagOpts, lambda x: L.bfq_bam_to_fastq_host(stream, len(stream), C.byref(x), None, None, (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), None)),
                       (_lib.UbamTagOpts, lambda x: L.bfq_fastq_to_bam_host((C.c_void_p * 3)(), (C.c_uint64 * 3)(), C.byref(x), None, 0, C.byref(C.c_uint64()), None))):
        way_in = make is _lib.BamTagOpts
        err = L.bfq_bam_host_error if way_in else L.bfq_ubam_host_error
        for n, key in ((33, b"BC"), (1, b"1C"), (1, b"B-"), (2, b"\0\0")):
            x = make()
            (L.bfq_bam_default_opts if way_in else L.bfq_ubam_default_opts)(C.byref(x.o))
            x.o.reserved = _lib.BAM_OPTS_TAGS if way_in else _lib.UBAM_OPTS_TAGS
            x.n_tags = n
            x.tag[min(n, 32) - 1][0], x.tag[min(n, 32) - 1][1] = key[0], key[1]
            x.tag[0][0], x.tag[0][1] = (key[0], key[1]) if n == 1 else (66, 67)
            assert call(x) == -1 and b"tags" in err(), (n, key)
            x.o.reserved = 7                                         # any other value: ignored, as before
            assert call(x) == (0 if way_in else -1) and b"tags" not in err()      # (the way out without a buffer: only its length)
    with pytest.raises(ValueError):
        api.bam_opts(tags="BCX")
    with pytest.raises(ValueError):
        api.ubam_opts(tags=",".join(["BC"] * 33))
    assert C.sizeof(_lib.BamOpts) == 32 and C.sizeof(_lib.BamStats) == 120 and C.sizeof(_lib.UbamOpts) == 40 and C.sizeof(_lib.UbamStats) == 72
    assert _lib.BamOpts.reserved.offset == 28 and _lib.UbamOpts.reserved.offset == 12 and _lib.UbamOpts.rg_id.offset == 32
    assert C.sizeof(_lib.BamTagOpts) == 32 + 8 + 64 + 8 and _lib.BamTagOpts.tag.offset == 40 and _lib.BamTagOpts.stats.offset == 104
    assert C.sizeof(_lib.UbamTagOpts) == 40 + 8 + 64 + 8 and _lib.UbamTagOpts.tag.offset == 48 and _lib.UbamTagOpts.stats.offset == 112
    assert C.sizeof(_lib.BamTagStats) == 24 and C.sizeof(_lib.UbamTagStats) == 24
    o = _lib.BamOpts()
    L.bfq_bam_default_opts(C.byref(o))
    assert (o.exclude_flags, o.mate_suffix, o.default_qual, o.split, o.paired_check, o.piece, o.check_names, o.reserved) == (0x900, 1, 1, 0, 0, 0, 0, 0)
    u = _lib.UbamOpts()
    L.bfq_ubam_default_opts(C.byref(u))
    assert (u.mate_suffix, u.paired_check, u.level, u.reserved, u.header_text, u.header_len, u.rg_id) == (1, 0, 1, 0, None, 0, None)
    assert api.bam_opts().reserved == 0 and api.ubam_opts()[0].reserved == 0 and isinstance(api.bam_opts(), _lib.BamOpts)
    assert api.bam_opts(tags="*").o.reserved == 0x31474154 and api.ubam_opts(tags="BC")[0].o.reserved == 0x32474154


def test_driver_refuses_before_any_work(tmp_path):
    """--bam-tags without kept headers, with a list that is none, or with nothing it applies to: exit status 1 before an
    engine exists, nothing written"""
    fq, out = str(tmp_path / "in.fastq"), str(tmp_path / "o" / "OUT")
    os.mkdir(str(tmp_path / "o"))
    with open(fq, "wb") as f:
        f.write(U.cases()["lanes"][0][0])
    ubam = str(tmp_path / "o" / "u.bam")
    assert parallel.main([fq, "-o", out, "-t", "2", "--ubam-out", ubam, "--bam-tags", "*"]) == 1
    assert parallel.main([fq, "-o", out, "-t", "2", "--bam", "--bam-tags", "BC,RX"]) == 1
    assert parallel.main([fq, "-o", out, "-t", "2", "-H", "--ubam-out", ubam, "--bam-tags", "BCD"]) == 1
    assert parallel.main([fq, "-o", out, "-t", "2", "-H", "--bam-tags", "BC"]) == 1
    assert os.listdir(str(tmp_path / "o")) == []


def test_bam_tags_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bam_tags")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_bam_tags.cpp")])
    lines, n = [], [0]

    def put(data):
        n[0] += 1
        p = str(tmp_path / ("f%d" % n[0]))
        with open(p, "wb") as f:
            f.write(data if data is not None else b"")
        return p if data is not None else "-"

    def sel(tags):
        return "*" if tags == "*" else tags

    for opts in T.WAY_IN_OPTS:
        call, model = split_opts(opts)
        want, _, wts = T.expected(T.way_in_recs(), opts["tags"], **model)
        stream = put(M.Case(T.way_in_recs(), raw=True).stream)
        for piece in T.PIECES:
            lines.append("in %s %s 0 %d %d %d %s %s %s %d %d %d" % (stream, sel(opts["tags"]), piece, model.get("split", 0), model.get("mate_suffix", 1),
                                                                    put(want[0]), put(want[1]), put(want[2]), wts["tags_written"], wts["tags_dropped"], wts["tag_bytes"]))
    bad = dict((k, (v, 0)) for k, v in T.bad_tag_recs().items())
    bad["strict"] = (T.strict_recs(), 1)
    for name, (recs, strict) in bad.items():
        with pytest.raises(T.Refused) as w:
            T.expected(recs, "*", strict=strict)
        stream = put(M.Case(recs, raw=True).stream)
        for piece in T.PIECES:
            lines.append("inbad %s * %d %d %s" % (stream, strict, piece, put(w.value.msg.encode())))
    for name in T.WAY_OUT_NAMES:
        texts, opts = T.way_out_cases()[name]
        want, wst, wts = T.expect_out(name)
        lines.append("out %s %s %s %s %d %s %s %d %d %d %d" % (put(texts[0]), put(texts[1]), put(texts[2]), sel(opts["tags"]), opts.get("paired_check", 0),
                                                               put(opts.get("rg_id")), put(want), wst["comments_dropped"], wts["tags_written"], wts["fields_dropped"],
                                                               wts["tag_bytes"]))
    man = put(("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert b"%d cases, 0 failures" % len(lines) in r.stdout
