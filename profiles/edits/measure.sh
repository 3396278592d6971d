#!/bin/bash
# The numbers of profiles/edits/README.md.  Run from the repository root after the build:
#     bash profiles/edits/measure.sh [READS] [LENGTH] [OUTDIR] [PARENT_ROOT]
# PARENT_ROOT: a built checkout of the parent commit (its bfqzip_amd package with libbfqhip.so): the job without edits is then
# timed on both packages, alternating.  Every step that uses the GPU has its own time limit and the script stops at the first
# step that fails.
set -o pipefail
N=${1:-3000000}; L=${2:-150}; OUT=${3:-${TMPDIR:-/tmp}/bfq_edits_measure}; PARENT=${4:-}
D=$(mktemp -d /dev/shm/bfqedits.XXXXXX) || exit 1
trap 'rm -rf "$D"' EXIT
mkdir -p "$OUT"
export PYTHONPATH=$PWD
{
echo "== size, job with and without edits, make against compare, the way back: $N x $L" &&
timeout -k 10 540 python profiles/edits/measure.py --reads "$N" --len "$L" --out "$OUT/measure_${N}x${L}.json" &&
if [ -n "$PARENT" ]; then
  echo "== the job without edits: this tree and the parent commit, alternating" &&
  for i in 1 2 3; do
    timeout -k 10 200 python profiles/edits/measure.py --reads "$N" --len "$L" --job-only --out "$OUT/job_this_$i.json" > /dev/null &&
    BFQ_MEASURE_ROOT=$PARENT PYTHONPATH=$PARENT timeout -k 10 200 python profiles/edits/measure.py --reads "$N" --len "$L" --job-only --out "$OUT/job_parent_$i.json" > /dev/null || exit 1
    python -c "import json,sys; [print(p, json.load(open(p))['job_plain_walls']) for p in sys.argv[1:]]" "$OUT/job_this_$i.json" "$OUT/job_parent_$i.json"
  done
fi &&
echo "== rocprofv3 --kernel-trace --stats: bfq_edits (make) and bfq_compare on the same two files, one run each" &&
timeout -k 10 200 python profiles/compare/make_inputs.py "$N" "$L" "$D/A.fastq" &&
timeout -k 10 300 python -m bfqzip_amd.parallel "$D/A.fastq" -t 1 -H -o "$D/B" &&
{ timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_edits" -o k -- dropin/bfq_edits -a "$D/A.fastq" -b "$D/B.fastq" -o "$D/run.edits" > "$OUT/prof_edits.log" 2>&1; rc=$?; [ $rc -le 1 ] || { tail -20 "$OUT/prof_edits.log"; exit 1; }; } &&
find "$OUT/prof_edits" -name '*kernel_stats.csv' -exec head -14 {} \; &&
{ timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_compare" -o k -- dropin/bfq_compare -a "$D/A.fastq" -b "$D/B.fastq" -o "$D/report.json" > "$OUT/prof_compare.log" 2>&1; rc=$?; [ $rc -le 1 ] || { tail -20 "$OUT/prof_compare.log"; exit 1; }; } &&
find "$OUT/prof_compare" -name '*kernel_stats.csv' -exec head -10 {} \; &&
dropin/bfq_edits -l "$D/run.edits"
} 2>&1 | tee "$OUT/measure.log"
