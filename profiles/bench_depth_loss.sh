#!/bin/bash
# usage (on the GPU box, from the repo root): bash profiles/bench_depth_loss.sh [outdir]
# The kernel times of DESIGN.md section 14: fp32 batch-32 train steps with loss="mse" and with a full DepthLoss, each in a
# process of its own under rocprofv3 --kernel-trace --stats and under its own time limit; the second run starts only if the
# first succeeded.
set -o pipefail
out=${1:-bench_out}
mkdir -p $out
export TMPDIR=/tmp PYTHONPATH=.
: > $out/depth_loss_kernels.txt
for loss in mse depth; do
  d=$out/depth_loss_prof_${loss}
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $d -- \
      python3 profiles/bench_depth_loss.py --loss $loss > $out/depth_loss_${loss}.log 2>&1 || exit 1
  f=$(find $d -name "*kernel_stats.csv" | head -1)
  python3 - "$f" "$out/depth_loss_${loss}.log" <<'PY' | tee -a $out/depth_loss_kernels.txt
import csv, sys
print([l.strip() for l in open(sys.argv[2]) if "step median" in l][-1])
for r in csv.DictReader(open(sys.argv[1])):
    if "loss_stage" in r["Name"]:
        print("  %-62s calls %3s avg_us %8.1f min_us %8.1f max_us %8.1f" % (r["Name"][:62], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                          float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
PY
done
