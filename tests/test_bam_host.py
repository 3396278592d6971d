"""Host side of the BAM input (csrc/bfq_bam.h): the host form of the conversion (HostText.bam_to_fastq_host) against the
texts and the statistics the model computes from its own record lists (tests/bam_model.py), every refusal's message, the
probe, and the same code compiled for the host with sanitizers and run as a program of its own."""
import os
import subprocess
import ctypes as C
import gzip
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import bam_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


def test_model_files_are_bam():
    """the model's files are BGZF around the stream the record lists encode; the golden input comes back as its FASTQ"""
    g = M.good()
    for name in M.GOOD_NAMES:
        c = g[name]
        assert (c.blob if name == "j-raw" else gzip.decompress(c.blob)) == c.stream and c.stream[:4] == b"BAM\1", name
        assert len(c.blob) < 1_000_000
    assert M.expect(g["i-golden"])[0][0] == M.B.golden_text(M.GOLDEN + ".fastq")
    assert g["f-header-big"].hdr_end > 100_000 and len(M.B.directory(g["f-header-big"].blob)) > 3      # the header spans BGZF members
    assert len(g["k-level0"].blob) > len(g["k-level0"].stream)     # stored members
    assert sum(len(r.seq) == 60000 for r in g["c-long"].recs) == 1
    st = M.expect(g["b-edges"])[1]
    assert st["clamped_quals"] > 0 and st["no_qual"] > 0 and st["reversed"] > 0 and st["skipped"] > 0


@pytest.mark.parametrize("name", M.GOOD_NAMES)
def test_host_form_gives_the_models_texts_and_stats(name):
    c = M.good()[name]
    for opts in M.OPTION_SETS:
        want = M.expect(c, **opts)[0]
        for piece in M.PIECES:
            texts, st = host.bam_to_fastq_host(c.stream, piece=piece, **opts)
            assert [t.tobytes() for t in texts] == want, (name, piece, opts)
            assert st.as_dict() == M.stats(c, piece, **opts), (name, piece, opts)


def test_chain_is_parallel():
    """the suite does not pass on a serial or lucky run"""
    g = M.good()
    st = host.bam_to_fastq_host(g["a-ubam"].stream, piece=1024)[1]
    print("a-ubam @1024:", st)
    assert st.walkers >= st.pieces - 1 and st.pieces >= 900 and st.repaired == 0 and st.dead == 0
    st = host.bam_to_fastq_host(g["c-long"].stream, piece=256)[1]
    print("c-long @256:", st)
    assert st.pieces - st.walkers >= 100 and M.chain(g["c-long"], 256)[1] >= 100
    for piece in M.PIECES:
        st = host.bam_to_fastq_host(g["d-false"].stream, piece=piece)[1]
        assert st.dead >= 1 and st.repaired >= 1 and st.rounds == 1 + st.repaired, (piece, st)
        st = host.bam_to_fastq_host(g["e-resync"].stream, piece=piece)[1]
        assert st.dead == 0 and st.repaired >= 1, (piece, st)


def test_buffer_rules():
    c = M.good()["h-paired"]
    want = M.expect(c, split=1)[0]
    assert len(want[0]) == 0 and len(want[1]) and len(want[2])
    bufs = [np.full(len(w) + 64, 0xA5, np.uint8) for w in want]
    texts, st = host.bam_to_fastq_host(c.stream, outs=[b[32:32 + len(w)] for b, w in zip(bufs, want)], split=1, paired_check=1)
    assert [t.tobytes() for t in texts] == want and list(st.written) == [0, 500, 500]
    for b, w in zip(bufs, want):
        assert (b[:32] == 0xA5).all() and (b[32 + len(w):] == 0xA5).all()
    for k in (1, 2):                                               # one byte short in one output: nothing is written anywhere
        outs = [np.full(len(w) - (1 if i == k else 0), 0xA5, np.uint8) for i, w in enumerate(want)]
        with pytest.raises(api.BfqError) as e:
            host.bam_to_fastq_host(c.stream, outs=outs, split=1)
        assert e.value.code == -1 and e.value.needed == [len(w) for w in want] and all((o == 0xA5).all() for o in outs)
    for bad in (dict(piece=63), dict(piece=(1 << 30) + 1), dict(default_qual=94), dict(paired_check=1)):
        with pytest.raises(api.BfqError) as e:
            host.bam_to_fastq_host(c.stream, **bad)
        assert e.value.code == -1, bad


def test_refusals_carry_their_message():
    bad = M.refusals()
    seen = set()
    for name, (blob, stream, code, msg) in bad.items():
        if stream is None:
            continue
        for piece in (256, 4096, 0):
            with pytest.raises(api.BfqError) as e:
                host.bam_to_fastq_host(stream, piece=piece)
            assert e.value.code == code and str(e.value).endswith(msg), (name, piece, str(e.value))
        seen.add(msg.split(": ")[-1])
    assert seen == set(M.REASON_TEXT[1:])                            # one input per reason at least


def test_pairing_check():
    c = M.good()["h-paired"]
    assert host.bam_to_fastq_host(c.stream, split=1, paired_check=1)[1].written[1] == 500
    for name, (case, msg) in M.pair_refusals().items():
        for piece in (256, 0):
            with pytest.raises(api.BfqError) as e:
                host.bam_to_fastq_host(case.stream, split=1, paired_check=1, piece=piece)
            assert e.value.code == -1 and str(e.value).endswith(msg), (name, str(e.value))
        assert host.bam_to_fastq_host(case.stream, split=1)[1].records == len(case.recs)     # without the check it converts


def test_probe():
    g = M.good()
    for name in M.GOOD_NAMES:
        assert host.bam_probe(g[name].blob), name
    fq = M.B.golden_text("example.fastq")
    assert not host.bam_probe(fq) and not host.bam_probe(M.B.bgzf(fq)) and not host.bam_probe(gzip.compress(fq)) and not host.bam_probe(b"")
    assert not host.bam_probe(M.B.EOF) and not host.bam_probe(b"BAM") and host.bam_probe(b"BAM\1")
    assert not host.bam_probe(M.refusals()["bad-magic"][0])


def test_bam_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bam")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_bam.cpp")])
    lines = []

    def put(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        return p

    g = M.good()
    for name in M.GOOD_NAMES:
        if name == "j-raw":
            continue
        for split in (0, 1):
            want = M.expect(g[name], split=split)[0]
            lines.append("good %s %d %s %s %s" % (put(name + ".bam.raw", g[name].stream), split, put("%s.%d.0.fq" % (name, split), want[0]),
                                                  put("%s.%d.1.fq" % (name, split), want[1]), put("%s.%d.2.fq" % (name, split), want[2])))
    for name, (blob, stream, code, msg) in M.refusals().items():
        if stream is not None:
            lines.append("bad %s %s" % (put(name + ".bam.raw", stream), put(name + ".msg", msg.encode())))
    sweep = M.Case(M.ubam(12, seed=31))
    lines.append("sweep %s %s" % (put("sweep.bam.raw", sweep.stream), put("sweep.fq", M.expect(sweep)[0][0])))
    man = put("manifest", ("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_bam_default_opts", "bfq_bam_probe", "bfq_bam_measure", "bfq_bam_to_fastq", "bfq_bam_to_fastq_device", "bfq_bam_to_fastq_fd",
              "bfq_bam_to_fastq_host", "bfq_bam_host_error"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.BamOpts) == 32 and C.sizeof(_lib.BamStats) == 120
    o = _lib.BamOpts()
    L.bfq_bam_default_opts(C.byref(o))
    assert (o.exclude_flags, o.mate_suffix, o.default_qual, o.split, o.paired_check, o.piece) == (0x900, 1, 1, 0, 0, 0)
