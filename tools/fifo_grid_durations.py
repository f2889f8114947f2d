#!/usr/bin/env python3
"""Does a FIFO launch pay for a second round of resident workgroups?  Tabulate the durations of fw_k_update_fifo in a rocprofv3
kernel trace (CSV, --kernel-trace alone) by the launch's grid size in workgroups: configs[1] launches ~1042 of them in a frame
that spawns and ~976 in the one frame of sixty that does not (the cycle wrap).
    tools/fifo_grid_durations.py trace.csv [slots]      slots: resident workgroups the split is made at (default 1024)"""
import collections
import csv
import statistics
import sys


def col(row, *names):
    low = {k.lower(): k for k in row}
    for n in names:
        if n in low:
            return row[low[n]]
    raise KeyError(names)


def main(path, slots=1024):
    per_grid = collections.defaultdict(list)
    names = collections.Counter()
    for r in csv.DictReader(open(path)):
        name = col(r, "kernel_name")
        if "fw_k_update_fifo" not in name:
            continue
        wg = int(col(r, "workgroup_size_x", "workgroup_size"))
        grid = int(col(r, "grid_size_x", "grid_size")) // max(1, wg)
        per_grid[grid].append((int(col(r, "end_timestamp")) - int(col(r, "start_timestamp"))) / 1e3)
        names[name.split("(")[0][-60:]] += 1
    for n, c in names.most_common():
        print(f"{c:6d} launches of {n}")
    steady = {g: v for g, v in per_grid.items() if g > slots * 3 // 4}  # (the first frames of a run: the ring still fills)

    def line(label, v):
        v = sorted(v)
        if not v:
            print(f"  {label:28s} n=    0")
            return
        q = lambda f: v[min(len(v) - 1, int(f * len(v)))]
        print(f"  {label:28s} n={len(v):5d} mean={statistics.fmean(v):7.2f} us  p10={q(0.1):7.2f}  p50={q(0.5):7.2f}  p90={q(0.9):7.2f}  "
              f"min={v[0]:7.2f}  max={v[-1]:7.2f}  spread(p90-p10)={q(0.9) - q(0.1):5.2f}")

    print(f"grids above {slots * 3 // 4} workgroups, by grid size:")
    for g in sorted(steady):
        line(f"{g} workgroups", steady[g])
    print(f"split at {slots} resident workgroups:")
    le = [x for g, v in steady.items() if g <= slots for x in v]
    gt = [x for g, v in steady.items() if g > slots for x in v]
    line(f"grid <= {slots}", le)
    line(f"grid >  {slots}", gt)
    if le and gt:
        print(f"  difference of the medians: {statistics.median(gt) - statistics.median(le):.2f} us")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1024)
