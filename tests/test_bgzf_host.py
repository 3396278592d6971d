"""Host side of the BGZF input (bfq_bgzf.h): the header walk, the inflate and the CRC32 that the kernel runs, compiled for the
host with sanitizers and run as a program of its own over the model's files (tests/bgzf_model.py); the directory the library
reports."""
import ctypes as C
import os
import subprocess
import zlib
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import bgzf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_is_gzip():
    """every good case of the model is a multi-member gzip that Python's own inflate accepts; the EOF member is htslib's"""
    assert len(M.EOF) == 28 and M.bgzf(b"", eof=True) == M.EOF
    for name, blob in {**M.extremes(), **M.crafted()}.items():
        M.expected(blob)
    blob = M.matrix()["synth-c700-l9"]
    assert M.expected(blob) == M.synth_var() and len(M.directory(blob)) == 273 + 1
    assert len(M.extremes()["A-65536"]) == 105 + 28 and len(M.extremes()["random-65280"]) == 65316 + 28


def test_bgzf_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_bgzf")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_bgzf.cpp")])
    lines = []

    def put(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        return p

    good = {**M.matrix(), **M.extremes(), **M.crafted(), "big": M.big()}
    for name, blob in good.items():
        text = M.expected(blob)
        lines.append("good %s %s %08x" % (put(name + ".gz", blob), put(name + ".txt", text), zlib.crc32(text)))
    bad, _, _ = M.refusals()
    assert {r for _, r, _, _ in bad.values()} == set(range(1, len(M.REASONS)))       # one input per reason code at least
    for name, (blob, reason, member, off) in bad.items():
        lines.append("bad %s %d %d %d" % (put(name + ".gz", blob), reason, member, off))
    text = M.golden_text("example.fastq")[:400]
    sweep = M.bgzf(text, 200, eof=False)
    assert len(M.directory(sweep)) == 2 and len(sweep) < 600
    lines.append("sweep %s %s" % (put("sweep.gz", sweep), put("sweep.txt", text)))
    man = put("manifest", ("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]


def test_probe_and_index():
    host = api.HostText
    text = M.synth_var()
    blob = M.bgzf(text, 700, level=1)
    assert host.bgzf_probe(blob) and not host.bgzf_probe(text) and not host.bgzf_probe(b"") and not host.bgzf_probe(blob[:17])
    assert not host.bgzf_probe(__import__("gzip").compress(text[:100]))
    members, raw = host.bgzf_index(blob)
    assert raw == len(text) and [tuple(int(x) for x in m) for m in members] == M.directory(blob)
    assert host.bgzf_index(M.EOF) == ([(0, 0, 28, 0)], 0)
    bad, good, _ = M.refusals()
    for name in ("short-header", "not-gzip", "flg", "subfield", "no-bc", "total-small", "truncated-mid-member", "isize", "plain-gzip"):
        blob, reason, member, off = bad[name]
        with pytest.raises(api.BgzfIndexError) as e:
            host.bgzf_index(blob)
        assert e.value.code == -1 and e.value.members == member and e.value.bad_off == off, name


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_bgzf_probe", "bfq_bgzf_index", "bfq_bgzf_inflate", "bfq_bgzf_inflate_device", "bfq_bgzf_inflate_fd"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert C.sizeof(_lib.BgzfMember) == 24
