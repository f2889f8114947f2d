#!/usr/bin/env python3
"""p10 / p50 / p90 / mean of every kernel of the last N dispatches of a rocprofv3 kernel trace CSV, and the gaps between them
(profiles/analyze_trace.py prints averages and extremes; the fused-launch rounds quote quantiles).  usage: trace_quantiles.py CSV [N]"""
import collections
import csv
import sys

import numpy as np

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
rows = rows[-(int(sys.argv[2]) if len(sys.argv) > 2 else 600):]
dur = collections.defaultdict(list)
for r in rows:
    dur[r["Kernel_Name"].split("(")[0][-60:]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
span = (int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])) / 1e3
gaps = np.array([int(b["Start_Timestamp"]) - int(a["End_Timestamp"]) for a, b in zip(rows, rows[1:])]) / 1e3
print(f"last {len(rows)} dispatches, span {span:.1f} us")
for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
    p = np.percentile(v, [10, 50, 90])
    print(f"  {k:62s} n={len(v):4d}  p10 {p[0]:6.2f}  p50 {p[1]:6.2f}  p90 {p[2]:6.2f}  mean {np.mean(v):6.2f} us  {sum(v) / span * 100:5.1f} % of the span")
print(f"  gaps: mean {gaps.mean():.2f} us  p50 {np.median(gaps):.2f}  p90 {np.percentile(gaps, 90):.2f}")
