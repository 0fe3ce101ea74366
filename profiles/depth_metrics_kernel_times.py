"""Reads rocprofv3's kernel_stats.csv of a profiles/bench_depth_metrics.py --mode kernels run: the times of the two kernels of
each launch, their sums and the ratio DESIGN.md section 15 reports.  usage: depth_metrics_kernel_times.py STATS.csv RUN.log"""
import csv
import sys

print([l.strip() for l in open(sys.argv[2]) if "device events" in l][-1])
avg = {}
for r in csv.DictReader(open(sys.argv[1])):
    for key in ("depth_metrics_stage1", "depth_metrics_stage2", "depth_loss_stage1", "depth_loss_stage2"):
        if key in r["Name"]:
            avg[key] = float(r["AverageNs"]) / 1e3
            print("  %-62s calls %3s avg_us %8.1f min_us %8.1f max_us %8.1f" % (r["Name"][:62], r["Calls"], avg[key],
                                                                              float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
m = avg["depth_metrics_stage1"] + avg["depth_metrics_stage2"]
l = avg["depth_loss_stage1"] + avg["depth_loss_stage2"]
print("  kernel time of the launch: metrics %.1f us, depth loss %.1f us, ratio %.2f (stage 1 alone: %.2f)"
      % (m, l, m / l, avg["depth_metrics_stage1"] / avg["depth_loss_stage1"]))
