"""Host side of the sparse position bins (bfq_posbin.h): the live regions of a partially filled bin, the gap tiles, the polarity
rule and the terminator-rank arithmetic of a window, compiled for the host with sanitizers and run as a program of its own;
the introspection entry on a context that has run nothing."""
import ctypes as C
import os
import subprocess
from bfqzip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posbin_sparse_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_posbin_sparse")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_posbin_sparse.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_sparse_last_refuses_no_context():
    pol, sent = C.c_int(7), C.c_uint64(7)
    assert _lib.lib().bfq_posbin_sparse_last(None, C.byref(pol), C.byref(sent)) != 0
    assert pol.value == 7 and sent.value == 7
