"""Host side of the plain gzip input (csrc/bfq_gzip.h): the model's inputs against Python's zlib, the host form of the
side-by-side inflate (HostText.gzip_inflate_host) against zlib's text and the model's chain (tests/gzip_model.py), every
refusal's message, and the same code compiled for the host with sanitizers and run as a program of its own."""
import os
import subprocess
import numpy as np
import pytest
from bfqzip_amd import _lib, api
from tests import gzip_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
host = api.HostText


def stats_of(st):
    return st.as_dict()


def test_model_inputs_are_gzip():
    """every good input inflates under zlib, member by member, to its text; the feasibility figures of the design hold"""
    g = M.good()
    text = M.B.synth_var()
    for name in ("a-l1-m1", "a-l6-m1", "a-l9-m8", "b-huff", "b-rle", "b-fixed", "b-l0", "f-inside", "f-boundary", "g-flush", "j-bgzf"):
        assert M.expected(g[name]) == text, name
    assert M.expected(g["d-big-m1"]) == M.big_text() == M.expected(g["d-big-m8"]) and len(M.big_text()) == 3_000_000
    assert len(M.expected(g["e-repeat"])) == 2_000_000 and len(M.expected(g["c-random"])) == 200_000
    assert len(M.expected(g["h-reach"])) == 32768 + 258 + 7 and M.expected(g["i-false"]).endswith(b"tail\n")
    assert len(g["f-boundary"]) > 98304 and g["f-boundary"][98304:98306] == b"\x1f\x8b" and g["f-inside"][-700:] == b"\0" * 700
    # no candidate at all: one serial decoder
    for name in ("b-fixed", "b-l0"):
        assert M.rule_offsets(g[name]) == (), name
    # level 6 / memLevel 1: a true start, and no false one, in every 4096-byte piece behind the first
    st, on, off = M.chain(g["a-l6-m1"], 4096)
    assert st["pieces"] == 22 and st["chain"] == 22 and st["skipped"] == 0 and st["discarded"] == 0, st
    # the crafted far reach starts a decoder; the crafted header in a stored block is a candidate and no block
    for chunk in (512, 1024, 4096, 32768):
        st, on, off = M.chain(g["h-reach"], chunk)
        assert M.far_reach(32768)[1] in on[1:], chunk
        st, on, off = M.chain(g["i-false"], chunk)
        assert off == [M.false_start()[1]] and st["discarded"] == 1, (chunk, off)


def test_model_header_parse():
    rec = b"@r\nACGT\n+\nIIII\n"
    m = M.member(M.raw(rec), rec, extra=b"XY\x03\x00abc", name=b"reads.fq", comment=b"c", hcrc=True)
    assert M.member_header(m, 0) == (0, 10 + 2 + 7 + 9 + 2 + 2) and M.expected(m) == rec
    assert host.gzip_probe(m) and host.gzip_probe(M.gz(rec)) and host.gzip_probe(M.B.EOF) and not host.gzip_probe(rec) and not host.gzip_probe(b"")
    for name, (blob, reason, member, off) in M.refusals().items():
        if M.REASONS[reason] in ("SHORT", "NOT_GZIP", "RESERVED", "HCRC", "FIELD"):
            assert M.member_header(blob, off)[0] == reason, name
            assert not host.gzip_probe(blob[off:]), name


@pytest.mark.parametrize("chunk", M.CHUNKS)
def test_host_form_gives_zlibs_text(chunk):
    for name, blob in M.good().items():
        text = M.expected(blob)
        got, st = host.gzip_inflate_host(blob, chunk)
        assert got.tobytes() == text, (name, chunk)
        assert st.decoders == st.chain + st.discarded and st.pieces == max(1, -(-len(blob) // (chunk or M.DEF_CHUNK))), (name, chunk, st)
        assert stats_of(st) == M.chain(blob, chunk)[0], (name, chunk)


def test_chain_is_parallel():
    """the suite does not pass on a one-decoder run"""
    g = M.good()
    st = host.gzip_inflate_host(g["a-l6-m1"], 4096)[1]
    print("a-l6-m1 @4096:", st)
    assert st.chain >= 20 and st.skipped == 0
    st = host.gzip_inflate_host(g["d-big-m1"], 4096)[1]
    print("d-big-m1 @4096:", st)
    assert st.chain >= 20
    st = host.gzip_inflate_host(g["e-repeat"], 1024)[1]
    print("e-repeat @1024:", st)
    assert st.chain >= 20
    for chunk in M.CHUNKS:
        st = host.gzip_inflate_host(g["i-false"], chunk)[1]
        assert st.discarded == 1 and st.skipped == 1 and st.chain == st.decoders - 1, (chunk, st)
    st = host.gzip_inflate_host(g["f-boundary"], 4096)[1]
    assert st.members == 3 and st.chain >= 10


def test_buffer_rules():
    blob = M.good()["a-l6-m1"]
    text = M.expected(blob)
    buf = np.full(len(text) + 64, 0xA5, np.uint8)
    got, _ = host.gzip_inflate_host(blob, 1024, out=buf[32:32 + len(text)])
    assert got.tobytes() == text and (buf[:32] == 0xA5).all() and (buf[32 + len(text):] == 0xA5).all()
    small = np.full(1000, 0xA5, np.uint8)
    with pytest.raises(api.BfqError) as e:
        host.gzip_inflate_host(blob, 1024, out=small)
    assert e.value.code == -1 and e.value.needed == len(text) and (small == 0xA5).all()
    for chunk in (100, 256, 513, 3000):
        with pytest.raises(api.BfqError) as e:
            host.gzip_inflate_host(blob, chunk)
        assert e.value.code == -1 and "power of two" in str(e.value)


def test_refusals_carry_their_message():
    bad = M.refusals()
    assert {M.REASONS[r] for _, r, _, _ in bad.values()} == set(M.REACHABLE)          # one input per reason code at least
    for name, (blob, reason, member, off) in bad.items():
        for chunk in (512, 4096, 0):
            with pytest.raises(api.BfqError) as e:
                host.gzip_inflate_host(blob, chunk)
            assert e.value.code == -1 and str(e.value).endswith(M.message(member, off, reason)), (name, chunk, str(e.value))


def test_gzip_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_gzip")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_gzip.cpp")])
    lines = []

    def put(name, data):
        p = str(tmp_path / name)
        with open(p, "wb") as f:
            f.write(data)
        return p

    for name, blob in M.good().items():
        chunks = "1024,4096" if name.startswith(("d-", "e-")) else "512,1024,4096,32768"
        lines.append("good %s %s %s" % (put(name + ".gz", blob), put(name + ".txt", M.expected(blob)), chunks))
    for name, (blob, reason, member, off) in M.refusals().items():
        lines.append("bad %s %d %d %d" % (put(name + ".gz", blob), reason, member, off))
    text = M.B.synth_var()[:3000]
    sweep = M.gz(text, 6, 1) + b"\0" * 20
    assert M.chain(sweep, 512)[0]["chain"] >= 2
    lines.append("sweep %s %s" % (put("sweep.gz", sweep), put("sweep.txt", text)))
    man = put("manifest", ("\n".join(lines) + "\n").encode())
    r = subprocess.run([exe, man], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert r.returncode == 0, r.stdout.decode()[-4000:]


def test_symbols_exported():
    L = _lib.lib()
    for s in ("bfq_gzip_probe", "bfq_gzip_measure", "bfq_gzip_inflate", "bfq_gzip_inflate_device", "bfq_gzip_inflate_fd", "bfq_gzip_inflate_host",
              "bfq_gzip_host_error"):
        assert s in _lib.SYMBOLS and getattr(L, s)
    import ctypes as C
    assert C.sizeof(_lib.GzipStats) == 48
