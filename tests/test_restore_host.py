"""The way back on the host: bfqzip_amd.fastq.restore_text (line streams -> FASTQ text; the numpy mirror of
bfq_fastq_restore and the expected-value builder of tests/test_gpu_restore.py), through the CPU statement of the stream
codec, and the front-end's argument handling.  No GPU needed."""
import os, subprocess
import numpy as np
import pytest
from bfqzip_amd import fastq
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(util.golden_index())


def _streams(name):
    """(golden OUT.fq of the reference, its 2~4p and 4~4p line streams, 1~4p of the input)."""
    want = open(os.path.join(util.GOLDEN, name + ".M2B0.fq"), "rb").read()
    lines = want.split(b"\n")[:-1]
    src = open(os.path.join(util.GOLDEN, name + ".fastq"), "rb").read().split(b"\n")
    if src[-1] == b"":
        src.pop()
    cat = lambda xs: b"".join(x + b"\n" for x in xs)
    return want, cat(lines[1::4]), cat(lines[3::4]), cat(src[0::4])


@pytest.mark.parametrize("name", NAMES)
def test_restore_text_gives_the_golden_file_back(name):
    want, dna, qs, hdr = _streams(name)
    assert fastq.restore_text(dna, qs) == want                       # bfq_int without -H writes "@"
    with_headers = fastq.restore_text(dna, qs, hdr)
    key = "M2B0 -m 5 -H"
    if key in util.golden_index()[name]["out"]:
        assert util.md5(with_headers) == util.golden_index()[name]["out"][key]
    got, lines = with_headers.split(b"\n")[:-1], want.split(b"\n")[:-1]
    assert got[0::4] == hdr.split(b"\n")[:-1] and got[1::4] == lines[1::4] and got[2::4] == lines[2::4] and got[3::4] == lines[3::4]
    # a last line without its newline gets one (as the device line index does)
    assert fastq.restore_text(dna[:-1], qs[:-1], hdr[:-1]) == with_headers
    assert fastq.restore_text(b"", b"") == b"" and fastq.restore_text(b"", b"", b"") == b""


@pytest.mark.parametrize("name", NAMES)
def test_restore_text_after_the_codec_round_trip(orc, name):
    want, dna, qs, hdr = _streams(name)
    back = [orc.codec_decode(orc.codec_encode(np.frombuffer(s, np.uint8))).tobytes() for s in (dna, qs, hdr)]
    assert fastq.restore_text(back[0], back[1]) == want
    assert fastq.restore_text(*back) == fastq.restore_text(dna, qs, hdr)


def test_restore_text_refuses_streams_that_do_not_belong_together():
    _, dna, qs, hdr = _streams("synth_var")
    ql = qs.split(b"\n")[:-1]
    k = 1234
    assert len(ql[k]) > 1
    ql[k] = ql[k][:-1]                                                # one quality line one byte short
    with pytest.raises(ValueError, match=rf"read {k}\b"):
        fastq.restore_text(dna, b"".join(x + b"\n" for x in ql))
    hl = hdr.split(b"\n")[:-1]
    with pytest.raises(ValueError, match=rf"read {len(hl) - 1}\b.*header"):
        fastq.restore_text(dna, qs, b"".join(x + b"\n" for x in hl[:-1]))     # one header too few
    _, dna2, qs2, _ = _streams("synth_fix")                           # another collection's qualities
    d, q = dna.split(b"\n")[:-1], qs2.split(b"\n")[:-1]
    first = next(i for i in range(min(len(d), len(q))) if len(d[i]) != len(q[i]))
    with pytest.raises(ValueError, match=rf"read {first}\b"):
        fastq.restore_text(dna, qs2)
    whole = qs.split(b"\n")[:-1]
    with pytest.raises(ValueError, match=rf"read {len(whole) - 1}\b.*no partner"):
        fastq.restore_text(dna, b"".join(x + b"\n" for x in whole[:-1]))        # the last quality line is missing


def test_front_end_prints_usage_without_arguments():
    exe = os.path.join(ROOT, "dropin", "bfq_restore")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    for args in ([], ["-d", "x.bsc"], ["-d", "x.bsc", "-q", "y.bsc"]):
        r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1 and b"usage:" in r.stderr and b"-d" in r.stderr, (args, r.stderr)
