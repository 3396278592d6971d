"""The two files of profiles/compare/measure.sh: A = the synthetic collection as FASTQ text (bfq_synth_fastq), written to
argv[3]; B is made from it by the caller (parallel.py -H).  usage: make_inputs.py N L OUT.fastq"""
import sys
import numpy as np
from bfqzip_amd import api

N, L, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
eng = api.Engine(0)
buf = np.empty(N * (2 * L + 30), np.uint8)
n = eng.synth_fastq(api.synth_spec(N, L), buf)
buf[:n].tofile(out)
eng.close()
print(f"{out}: {N} x {L}, {n} bytes")
