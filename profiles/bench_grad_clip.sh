#!/bin/bash
# usage (on the GPU box, from the repo root): bash profiles/bench_grad_clip.sh [outdir]
# The kernel times of DESIGN.md section 13: fp32 and bf16 batch-32 train steps with and without max_grad_norm, each in a
# process of its own under rocprofv3 --kernel-trace --stats and under its own time limit; a run starts only if the one
# before it succeeded.
set -o pipefail
out=${1:-bench_out}
mkdir -p $out
export TMPDIR=/tmp PYTHONPATH=.
: > $out/grad_clip_kernels.txt
for dtype in fp32 bf16; do
  for clip in on off; do
    d=$out/grad_clip_prof_${dtype}_${clip}
    timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $d -- \
        python3 profiles/bench_grad_clip.py --dtype $dtype --clip $clip > $out/grad_clip_${dtype}_${clip}.log 2>&1 || exit 1
    f=$(find $d -name "*kernel_stats.csv" | head -1)
    python3 - "$f" "$out/grad_clip_${dtype}_${clip}.log" <<'PY' | tee -a $out/grad_clip_kernels.txt
import csv, sys
print([l.strip() for l in open(sys.argv[2]) if "step median" in l][-1])
for r in csv.DictReader(open(sys.argv[1])):
    if "grad_norm" in r["Name"] or "adam_ema" in r["Name"]:
        print("  %-62s calls %3s avg_us %8.1f min_us %8.1f max_us %8.1f" % (r["Name"][:62], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                          float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
PY
  done
done
