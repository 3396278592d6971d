"""Host side of the sort's record builder (bfq_keyrec.h), which k_build_keys and the generating first radix pass share:
compiled for the host with sanitizers and run as a program of its own, against a byte-wise restatement of every record;
the sort geometry the library reports."""
import ctypes as C
import os
import subprocess
from bfqzip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyrec_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_keyrec")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_keyrec.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_radix_geometry_accessor():
    L = _lib.lib()
    t, b = C.c_uint64(0), C.c_uint64(0)
    assert L.bfq_radix_geometry(1, C.byref(t), C.byref(b)) == 0
    tile = int(t.value)
    assert tile > 0 and b.value == tile                                   # a small collection: one tile per radix block
    assert L.bfq_radix_geometry(30_000_000 * 151, C.byref(t), C.byref(b)) == 0
    assert b.value % tile == 0 and b.value > tile
    assert L.bfq_radix_geometry(5, None, None) == 0
