"""Host side of the BGZF output (bfq_deflate.h): the writer that the kernel runs, compiled for the host with sanitizers and
run as a program of its own over the texts of tests/deflate_cases.py; the same texts through the library's host form
(HostText.bgzf_deflate_model), read back by Python's gzip and measured against zlib's Huffman-only coding."""
import ctypes as C
import gzip
import os
import subprocess
import zlib
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import bgzf_model as M
from tests import deflate_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deflate_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_deflate")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_deflate.cpp")])
    lines = []
    for name, text in D.texts().items():
        p = str(tmp_path / (name + ".txt"))
        with open(p, "wb") as f:
            f.write(text)
        lines.append(p)
    man = str(tmp_path / "manifest")
    with open(man, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-4000:]
    assert ("%d texts, 0 failures" % len(lines)) in r.stdout.decode()


@pytest.mark.parametrize("name", list(D.texts()))
def test_host_form(name):
    text = D.texts()[name]
    host = api.HostText
    out = host.bgzf_deflate_model(text).tobytes()
    assert gzip.decompress(out) == text if text else out == M.EOF
    assert out.endswith(M.EOF)
    d = M.directory(out)
    assert len(d) == D.members(len(text)) + 1 and d[-1][2:] == (28, 0)
    for k, (in_off, out_off, in_len, out_len) in enumerate(d[:-1]):
        assert in_len <= 65536 and in_len <= out_len + 31
        assert out_off == k * D.PIECE and out_len == (D.PIECE if k + 2 < len(d) else len(text) - k * D.PIECE)
    assert len(out) <= host.bgzf_deflate_bound(len(text)) == D.bound(len(text))
    stored = host.bgzf_deflate_model(text, level=0).tobytes()
    assert len(stored) == len(text) + 31 * D.members(len(text)) + 28
    assert (gzip.decompress(stored) if text else b"") == text and stored.endswith(M.EOF)
    assert len(out) <= len(stored)
    assert host.bgzf_deflate_model(text).tobytes() == out                      # the same bytes again


def test_host_form_sizes():
    host = api.HostText
    t = D.texts()
    assert len(host.bgzf_deflate_model(t["random-65280"])) <= len(host.bgzf_deflate_model(t["random-65280"], level=0))   # the stored fallback
    assert len(host.bgzf_deflate_model(t["A-run"])) < len(t["A-run"]) // 100
    assert host.bgzf_deflate_model(b"").tobytes() == M.EOF


@pytest.mark.parametrize("name", ["example", "synth_var"])
def test_huffman_only_floor(name):
    """a compressor that builds correct dynamic codes and takes only matches that pay is not larger than Huffman coding alone"""
    text = D.texts()[name]
    out = api.HostText.bgzf_deflate_model(text)
    floor = len(M.bgzf(text, 65280, strategy=zlib.Z_HUFFMAN_ONLY))
    print("%s: %d bytes, Huffman only %d, zlib level 1 %d" % (name, len(out), floor, len(M.bgzf(text, 65280, level=1))))
    assert len(out) <= floor


def test_host_form_refusals():
    L = _lib.lib()
    text = np.frombuffer(D.texts()["example"], np.uint8)
    bound = D.bound(len(text))
    out = np.full(bound, 0xA5, np.uint8)
    ol = C.c_uint64(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.bfq_bgzf_deflate_host(p(text), len(text), 1, p(out), bound - 1, C.byref(ol)) == -1 and ol.value == 0 and (out == 0xA5).all()
    assert L.bfq_bgzf_deflate_host(p(text), len(text), 2, p(out), bound, C.byref(ol)) == -1 and (out == 0xA5).all()
    gz = np.frombuffer(M.bgzf(D.texts()["example"]), np.uint8)
    big = np.full(D.bound(len(gz)), 0xA5, np.uint8)
    assert L.bfq_bgzf_deflate_host(p(gz), len(gz), 1, p(big), len(big), C.byref(ol)) == -1 and (big == 0xA5).all()
    with pytest.raises(api.BfqError):
        api.HostText.bgzf_deflate_model(text, level=3)


def test_exports_and_bound():
    L = _lib.lib()
    for s in ("bfq_bgzf_deflate_bound", "bfq_bgzf_deflate_host", "bfq_bgzf_deflate", "bfq_bgzf_deflate_device", "bfq_bgzf_deflate_fd"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    assert "bfq_fastq_restore_bgzf_fd" in _lib.SYMBOLS and L.bfq_fastq_restore_bgzf_fd
    bound = api.HostText.bgzf_deflate_bound
    assert [bound(n) for n in (0, 1, 65280, 65281)] == [28, 60, 65339, 65371]
    assert bound(3 * 65280) == 3 * 65280 + 3 * 31 + 28
