#!/bin/bash
# usage (on the GPU box, from the repo root): bash profiles/bench_gather_augment.sh [outdir]
# The timing table of DESIGN.md section 12: profiles/bench_gather_augment.py with device events (and the fp32 train step it
# is held against), then the same launches under rocprofv3 --kernel-trace --stats for the kernel times.  Each GPU step runs
# under its own time limit and the second starts only if the first succeeded.
set -o pipefail
out=${1:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
prof=$out/gather_augment_prof
timeout -k 10 420 python3 profiles/bench_gather_augment.py --out $out/gather_augment_b32.json | tee $out/gather_augment_b32.txt &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $prof -- \
    python3 profiles/bench_gather_augment.py --launches 100 --no-step --no-events > $out/gather_augment_prof.log 2>&1 &&
f=$(find $prof -name "*kernel_stats.csv" | head -1) &&
python3 - "$f" <<'PY' | tee $out/gather_augment_b32_kernels.txt
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
print("rocprofv3 --kernel-trace --stats, 232 launches of each case (warm-up included)")
for r in rows:
    if "gather" in r["Name"] or "opy" in r["Name"]:
        print("%-70s calls %5s avg_us %8.1f min_us %8.1f max_us %8.1f" % (r["Name"][:70], r["Calls"], float(r["AverageNs"]) / 1e3,
                                                                        float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
PY
