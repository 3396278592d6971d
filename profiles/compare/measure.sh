#!/bin/bash
# The numbers of profiles/compare/README.md: bfq_compare on a synthetic collection against its smoothed output, both on
# /dev/shm.  Run from the repository root after the build: bash profiles/compare/measure.sh [READS] [LENGTH] [OUTDIR]
# Every step that uses the GPU has its own time limit and the script stops at the first step that fails.
set -o pipefail
N=${1:-30000000}; L=${2:-150}; OUT=${3:-${TMPDIR:-/tmp}/bfq_compare_measure}
D=$(mktemp -d /dev/shm/bfqcmp.XXXXXX) || exit 1
trap 'rm -rf "$D"' EXIT
mkdir -p "$OUT"
export PYTHONPATH=$PWD BFQ_TRACE=1
T=dropin/bfq_compare
{
echo "== inputs: $N x $L"
timeout -k 10 300 python profiles/compare/make_inputs.py "$N" "$L" "$D/A.fastq" || exit 1
# B: what a sharded run with headers kept writes (same length as A: cmp -l can walk both), and the driver's own report
TIMEFORMAT="parallel.py -t 4 -H --report: %R s wall"
time timeout -k 10 600 python -m bfqzip_amd.parallel "$D/A.fastq" -t 4 -H -o "$D/B" --report || exit 1
ls -l "$D"
python -c "import json,sys; r=json.load(open(sys.argv[1])); print({k: r[k] for k in ('n_reads','total_bases','n_diffs','reads_changed','bases_changed','quals_changed','qual_abs_sum','headers_same')})" "$D/B.fastq.report.json"
echo "== bfq_compare -V, histogram adds by run heads (BFQ_CMP_HIST=runs) and per lane (direct), alternating"
for i in 1 2 3; do
  for h in runs direct; do
    echo "-- run $i, $h"
    BFQ_CMP_HIST=$h timeout -k 10 120 $T -a "$D/A.fastq" -b "$D/B.fastq" -V -o "$OUT/report_$h.json"; rc=$?
    [ $rc -le 1 ] || exit 1
  done
done
cmp "$OUT/report_runs.json" "$OUT/report_direct.json" && echo "reports of both variants identical"
echo "== the first 1000 differing positions as well (-n 1000)"
timeout -k 10 120 $T -a "$D/A.fastq" -b "$D/B.fastq" -n 1000 -V -o "$OUT/report_n1000.json"; [ $? -le 1 ] || exit 1
echo "== rocprofv3 --kernel-trace --stats, one run per variant"
for h in runs direct; do
  BFQ_CMP_HIST=$h BFQ_TRACE= timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$h" -o k -- $T -a "$D/A.fastq" -b "$D/B.fastq" -o "$OUT/report_prof.json" > "$OUT/prof_$h.log" 2>&1; rc=$?
  [ $rc -le 1 ] || { tail -20 "$OUT/prof_$h.log"; exit 1; }
  echo "-- $h"; find "$OUT/prof_$h" -name '*kernel_stats.csv' -exec head -12 {} \;
done
echo "== cmp -l on the same two files (one line per differing byte), 120 s at the most"
TIMEFORMAT="cmp -l | wc -l: %R s wall"
time (timeout 120 cmp -l "$D/A.fastq" "$D/B.fastq" | wc -l)
echo "== cmp of A with a copy of itself (the plain walk over two files of this size)"
TIMEFORMAT="cmp A A2: %R s wall"
cp "$D/A.fastq" "$D/A2.fastq" && time cmp "$D/A.fastq" "$D/A2.fastq"
} 2>&1 | tee "$OUT/measure.log"
