"""The output files of a *_fd call (bfq_outfiles.h): committed at their final lengths, or left empty however the call ends --
with registered mappings picked up, replaced or taken along, absent members skipped and pipes written through their
descriptor.  Compiled for the host with sanitizers over bfq_host.cpp and run as a program of its own: a mapping that is neither
closed nor left registered is a leak LeakSanitizer reports."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_outfiles_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_outfiles")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cxx", "test_outfiles.cpp"), os.path.join(ROOT, "bfqzip_amd", "csrc", "bfq_host.cpp"), "-lpthread"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert r.returncode == 0, r.stdout.decode()[-3000:]
