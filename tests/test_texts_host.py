"""Host side of the staging of a call's FASTQ texts (bfq_texts.h): the plan -- which texts move into the text buffer, where,
and how long they are there -- against a table, and the arena sizes of the line kernels against the allocations k_fastq.hip
makes through the same helper.  Compiled for the host with sanitizers and run as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_texts_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_texts")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_texts.cpp")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
