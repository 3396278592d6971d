"""Host side of the position bins' write-combining (bfq_posbin.h: chunk size per level, head claims, tail slots): a model of
the partition kernel's bookkeeping, compiled for the host with sanitizers and run as a program of its own over every n up to
a few thousand and n around a window and a first-level bin (tests/cxx/test_posbin_wc.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posbin_wc_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_posbin_wc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_posbin_wc.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
