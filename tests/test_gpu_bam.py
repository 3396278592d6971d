"""GPU tests of the BAM input (bfq_bam_*, k_bam.hip): the texts and the statistics equal the host form's -- which
tests/test_bam_host.py holds against the model's record lists -- over the model's inputs (tests/bam_model.py), at several
piece sizes and option sets, into host buffers, device buffers with guard bands and files; every refusal gives the model's
message and leaves the engine usable; the tool and the multi-GPU driver's --bam.  The refusal inputs have passed the host
program under sanitizers first: they test refusal, none is meant to fault."""
import json
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import api, parallel
from tests import bam_model as M
from tests import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = os.path.join(ROOT, "dropin")
GUARD = 4096
PIECES = (256, 1024, 0)
host = api.HostText


def texts_of(arrs):
    return [a.tobytes() for a in arrs]


@pytest.mark.parametrize("name", M.GOOD_NAMES)
def test_engine_equals_the_host_form(engine, name):
    c = M.good()[name]
    for opts in M.OPTION_SETS:
        first = None
        for piece in PIECES:
            want, wst = host.bam_to_fastq_host(c.stream, piece=piece, **opts)
            got, st = engine.bam_to_fastq(c.blob, piece=piece, **opts)
            assert texts_of(got) == texts_of(want), (name, piece, opts)
            assert st.as_dict() == wst.as_dict(), (name, piece, opts)
            first = first or texts_of(got)
            assert texts_of(got) == first, (name, piece, opts)
        assert first == M.expect(c, **opts)[0], (name, opts)


@pytest.mark.parametrize("name", ("a-ubam", "b-edges", "d-false", "g-empty", "h-paired", "j-raw"))
def test_forms_agree(engine, tmp_path, name):
    import torch
    c = M.good()[name]
    for opts in (dict(), dict(split=1, piece=1024)):
        want, wst = host.bam_to_fastq_host(c.stream, **opts)
        want = texts_of(want)
        lens, reads, st = engine.bam_measure(c.blob, **opts)
        assert lens == [len(w) for w in want] and reads == list(wst.written) and st.as_dict() == wst.as_dict(), (name, opts)
        # host buffers, with guard bytes behind and in front of every output
        bufs = [np.full(len(w) + 2 * GUARD, 0xA5, np.uint8) for w in want]
        got, st = engine.bam_to_fastq(c.blob, outs=[b[GUARD:GUARD + len(w)] for b, w in zip(bufs, want)], **opts)
        assert texts_of(got) == want and st.as_dict() == wst.as_dict(), (name, opts)
        assert all((b[:GUARD] == 0xA5).all() and (b[GUARD + len(w):] == 0xA5).all() for b, w in zip(bufs, want))
        # device buffers
        d = [torch.full((len(w) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for w in want]
        lens, reads, st = engine.bam_to_fastq_device(c.blob, [t.data_ptr() + GUARD for t in d], [len(w) for w in want], **opts)
        assert lens == [len(w) for w in want] and reads == list(wst.written) and st.as_dict() == wst.as_dict(), (name, opts)
        for t, w in zip(d, want):
            h = t.cpu().numpy()
            assert h[GUARD:GUARD + len(w)].tobytes() == w and (h[:GUARD] == 0xA5).all() and (h[GUARD + len(w):] == 0xA5).all(), (name, opts)
        # files
        src = str(tmp_path / "in.bam")
        dst = [str(tmp_path / ("out%d.fq" % k)) for k in range(3)]
        with open(src, "wb") as f:
            f.write(c.blob)
        lens, reads, st = engine.bam_to_fastq_files(src, dst, **opts)
        assert [open(p, "rb").read() for p in dst] == want and lens == [len(w) for w in want] and st.as_dict() == wst.as_dict(), (name, opts)
        lens2, _, _ = engine.bam_to_fastq_files(src, **opts)          # verify only
        assert lens2 == lens


def test_capacity_one_byte_short(engine):
    import torch
    c = M.good()["h-paired"]
    want = M.expect(c, split=1)[0]
    for k in (1, 2):
        outs = [np.full(len(w) + GUARD - (GUARD + 1 if i == k else 0), 0xA5, np.uint8) for i, w in enumerate(want)]
        with pytest.raises(api.BfqError) as e:
            engine.bam_to_fastq(c.blob, outs=outs, split=1)
        assert e.value.code == -1 and e.value.needed == [len(w) for w in want] and all((o == 0xA5).all() for o in outs), k
        d = [torch.full((len(w) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda") for w in want]
        with pytest.raises(api.BfqError) as e:
            engine.bam_to_fastq_device(c.blob, [t.data_ptr() for t in d], [len(w) - (1 if i == k else 0) for i, w in enumerate(want)], split=1)
        assert e.value.code == -1 and e.value.needed == [len(w) for w in want] and all(bool((t == 0xA5).all()) for t in d), k
    for bad in (dict(piece=63), dict(default_qual=94), dict(paired_check=1)):
        with pytest.raises(api.BfqError) as e:
            engine.bam_to_fastq(c.blob, **bad)
        assert e.value.code == -1, bad
    assert texts_of(engine.bam_to_fastq(c.blob, split=1)[0]) == want


def test_refusals(engine):
    good = M.good()["a-ubam"]
    good_text = M.expect(good)[0]
    for name, (blob, stream, code, msg) in M.refusals().items():
        for piece in (256, 0):
            with pytest.raises(api.BfqError) as e:
                engine.bam_to_fastq(blob, outs=[np.empty(1 << 20, np.uint8), np.empty(0, np.uint8), np.empty(0, np.uint8)], piece=piece)
            assert e.value.code == code and (msg in str(e.value) if stream is None else str(e.value).endswith(msg)), (name, piece, str(e.value))
        with pytest.raises(api.BfqError) as e:
            engine.bam_measure(blob)
        assert e.value.code == code, name
        assert texts_of(engine.bam_to_fastq(good.blob, piece=1024)[0]) == good_text, name


def test_pairing_check(engine):
    c = M.good()["h-paired"]
    want = M.expect(c, split=1)[0]
    got, st = engine.bam_to_fastq(c.blob, split=1, paired_check=1, piece=256)
    assert texts_of(got) == want and list(st.written) == [0, 500, 500]
    for name, (case, msg) in M.pair_refusals().items():
        for piece in (256, 0):
            with pytest.raises(api.BfqError) as e:
                engine.bam_to_fastq(case.blob, split=1, paired_check=1, piece=piece)
            assert e.value.code == -1 and str(e.value).endswith(msg), (name, str(e.value))
        assert texts_of(engine.bam_to_fastq(case.blob, split=1)[0]) == M.expect(case, split=1)[0]
    assert "pair 17" in M.pair_refusals()["pair-name"][1]


def test_golden_input_round(engine):
    c = M.good()["i-golden"]
    fq = M.B.golden_text(M.GOLDEN + ".fastq")
    got, st = engine.bam_to_fastq(c.blob)
    assert got[0].tobytes() == fq and st.records == util.golden_index()[M.GOLDEN]["reads"]
    engine.set_params(m=5)
    r = engine.fastq_job([got[0]])
    assert util.md5(r.fastq.tobytes()) == util.golden_index()[M.GOLDEN]["out"]["M2B0 -m 5"]


def test_tool(tmp_path):
    tool = os.path.join(DROP, "bfq_bam")
    g = M.good()
    run = lambda *a: subprocess.run([tool] + list(a), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    path = lambda n: str(tmp_path / n)

    def put(name, data):
        with open(path(name), "wb") as f:
            f.write(data)
        return path(name)

    a = put("a.bam", g["a-ubam"].blob)
    r = run("-i", a, "-o", path("a.fq"))
    assert r.returncode == 0 and open(path("a.fq"), "rb").read() == M.expect(g["a-ubam"])[0][0], r.stderr
    r = run("-i", a, "-o", path("a2.fq"), "-n", "-F", "0", "-v", "30", "-C", "1024")
    assert r.returncode == 0 and open(path("a2.fq"), "rb").read() == M.expect(g["a-ubam"], mate_suffix=0, exclude_flags=0, default_qual=30)[0][0], r.stderr
    h = put("h.bam", g["h-paired"].blob)
    want = M.expect(g["a-ubam"], split=1)[0]
    r = run("-i", a, "-1", path("a_1.fq"), "-2", path("a_2.fq"), "-0", path("a_0.fq"))
    assert r.returncode == 0 and [open(path("a_%d.fq" % k), "rb").read() for k in range(3)] == want, r.stderr
    want = M.expect(g["h-paired"], split=1)[0]
    r = run("-i", h, "-1", path("h_1.fq"), "-2", path("h_2.fq"), "-c")
    assert r.returncode == 0 and [open(path("h_%d.fq" % k), "rb").read() for k in (1, 2)] == want[1:], r.stderr
    r = run("-t", a)
    assert r.returncode == 0 and b"verified" in r.stdout and b"4000 records" in r.stdout, (r.stdout, r.stderr)
    r = run("-l", a)
    j = json.loads(r.stdout.decode())
    wst = host.bam_to_fastq_host(g["a-ubam"].stream)[1].as_dict()
    assert r.returncode == 0 and j.pop("bytes") == [len(M.expect(g["a-ubam"])[0][0]), 0, 0] and j == wst, (j, wst)
    bad, _, _, msg = M.refusals()["rec-layout"]
    b = put("bad.bam", bad)
    for args in (("-i", b, "-o", path("bad.fq")), ("-t", b), ("-l", b)):
        r = run(*args)
        assert r.returncode == 1 and msg.encode() in r.stderr, (args, r.stderr)
    assert os.path.getsize(path("bad.fq")) == 0
    case, msg = M.pair_refusals()["pair-name"]
    u = put("unpaired.bam", case.blob)
    r = run("-i", u, "-1", path("u_1.fq"), "-2", path("u_2.fq"), "-c")
    assert r.returncode == 1 and msg.encode() in r.stderr and os.path.getsize(path("u_1.fq")) == 0 and os.path.getsize(path("u_2.fq")) == 0, r.stderr
    assert run("-i", a).returncode == 1 and run("-i", a, "-o", path("x.fq"), "-c").returncode == 1 and run("-i", a, "-1", path("x.fq")).returncode == 1


def test_parallel_bam(tmp_path):
    c = M.good()["h-paired"]
    want = M.expect(c, split=1)[0]
    bam, fq1, fq2 = str(tmp_path / "in.bam"), str(tmp_path / "in_1.fastq"), str(tmp_path / "in_2.fastq")
    for p, data in ((bam, c.blob), (fq1, want[1]), (fq2, want[2])):
        with open(p, "wb") as f:
            f.write(data)
    for d in "abc":
        os.mkdir(str(tmp_path / d))
    assert parallel.main([fq1, fq2, "-p", "-o", str(tmp_path / "a" / "OUT"), "-t", "2", "-0", "--m3"]) == 0
    assert parallel.main([bam, "-p", "--bam", "-o", str(tmp_path / "b" / "OUT"), "-t", "2", "-0", "--m3"]) == 0
    assert parallel.main([bam, "-p", "--bam", "-o", str(tmp_path / "c" / "OUT"), "-t", "2", "-0", "--m3", "--keep-inflated"]) == 0
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == sorted(os.listdir(str(tmp_path / "b"))) and len(names) == 8          # the converted files are gone
    assert sorted(os.listdir(str(tmp_path / "c"))) == sorted(names + ["in_1.fastq", "in_2.fastq"])
    assert open(str(tmp_path / "c" / "in_1.fastq"), "rb").read() == want[1] and open(str(tmp_path / "c" / "in_2.fastq"), "rb").read() == want[2]
    for n in names:
        ref = open(str(tmp_path / "a" / n), "rb").read()
        assert open(str(tmp_path / "b" / n), "rb").read() == ref and open(str(tmp_path / "c" / n), "rb").read() == ref, n
    # one BAM input, not paired: <name>.fastq, the run of the converted text
    os.mkdir(str(tmp_path / "d")); os.mkdir(str(tmp_path / "e"))
    single = str(tmp_path / "single.fastq")
    with open(single, "wb") as f:
        f.write(M.expect(c)[0][0])
    assert parallel.main([single, "-o", str(tmp_path / "d" / "OUT"), "-t", "2", "-0"]) == 0
    assert parallel.main([bam, "--bam", "-o", str(tmp_path / "e" / "OUT"), "-t", "2", "-0"]) == 0
    assert os.listdir(str(tmp_path / "e")) == ["OUT.fastq"]
    assert open(str(tmp_path / "e" / "OUT.fastq"), "rb").read() == open(str(tmp_path / "d" / "OUT.fastq"), "rb").read()

def test_bam_without_the_flag_is_not_taken(engine, tmp_path):
    """BAM is taken only by the new calls and the new flag: the FASTQ entry points read 1f 8b as BGZF-compressed FASTQ"""
    c = M.good()["h-paired"]
    with pytest.raises(api.BfqError):
        engine.fastq_run(c.blob)
    bam = str(tmp_path / "in.bam")
    with open(bam, "wb") as f:
        f.write(c.blob)
    assert parallel.main([bam, "-p", "-o", str(tmp_path / "OUT"), "-t", "2", "-0"]) == 1          # one input is no paired run
    with pytest.raises((api.BfqError, ValueError, RuntimeError, IndexError)):
        parallel.main([bam, "-o", str(tmp_path / "OUT"), "-t", "2", "-0"])
