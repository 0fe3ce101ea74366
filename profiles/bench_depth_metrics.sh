#!/bin/bash
# usage (on the GPU box, from the repo root): bash profiles/bench_depth_metrics.sh [outdir]
# The times of DESIGN.md section 15: the metrics launch against the depth-aware loss launch at batch 32 and batch 16, each
# batch in a process of its own under rocprofv3 --kernel-trace --stats, then (profiler off) the validation pass with and
# without metrics.  Every run has its own time limit and starts only if the one before succeeded.
set -o pipefail
out=${1:-bench_out}
mkdir -p $out
export TMPDIR=/tmp PYTHONPATH=.
: > $out/depth_metrics_kernels.txt
for batch in 32 16; do
  d=$out/depth_metrics_prof_b${batch}
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $d -- \
      python3 profiles/bench_depth_metrics.py --mode kernels --batch $batch > $out/depth_metrics_b${batch}.log 2>&1 || exit 1
  f=$(find $d -name "*kernel_stats.csv" | head -1)
  python3 profiles/depth_metrics_kernel_times.py "$f" "$out/depth_metrics_b${batch}.log" | tee -a $out/depth_metrics_kernels.txt || exit 1
done
for batch in 32 16; do
  timeout -k 10 300 python3 profiles/bench_depth_metrics.py --mode pass --batch $batch 2>&1 | grep "validation pass" \
      | tee -a $out/depth_metrics_kernels.txt || exit 1
done
