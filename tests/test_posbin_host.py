"""Host side of the position-bin inversion (bfq_posbin.h): the bin arithmetic and the position -> read search, compiled for
the host with sanitizers and run as a program of its own; the geometry the library reports."""
import ctypes as C
import os
import subprocess
from bfqzip_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posbin_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_posbin")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_posbin.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]


def test_geometry_accessor():
    L = _lib.lib()
    w, s = C.c_uint64(0), C.c_int(0)
    assert L.bfq_posbin_geometry(1, C.byref(w), C.byref(s)) == 0
    W = int(w.value)
    assert W & (W - 1) == 0 and (1 << s.value) == W                    # a small collection: one window per first-level bin
    assert L.bfq_posbin_geometry(512 * W, C.byref(w), C.byref(s)) == 0 and (1 << s.value) == W
    assert L.bfq_posbin_geometry(512 * W + 1, C.byref(w), C.byref(s)) == 0 and (1 << s.value) == 2 * W
    assert L.bfq_posbin_geometry(30_000_000 * 151, C.byref(w), C.byref(s)) == 0 and 30_000_000 * 151 <= 512 << s.value
    assert L.bfq_posbin_geometry(1 << 40, C.byref(w), C.byref(s)) != 0 and s.value == -1
    assert L.bfq_posbin_geometry(5, None, None) == 0
