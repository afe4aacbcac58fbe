#!/usr/bin/env python3
"""Per-kernel median time from a launch's begin stamp to the next launch's begin stamp (and the launch's own begin-to-end) out of the
*_kernel_trace.csv files of `rocprofv3 --kernel-trace --stats` runs, one column per run -- the table of profiles/fa_tail_two_launches.txt
section 2 and profiles/wave_priority.txt.  Launches are taken in start order; a gap of more than GAP us to the next launch (the end of a
step: the host synchronises) counts with its own duration instead.
usage: kernel_trace_b2b.py [--gap US] NAME=trace.csv [NAME=trace.csv ...]"""
import csv
import statistics
import sys

GAP = 100.0
args = sys.argv[1:]
if args and args[0] == "--gap":
    GAP = float(args[1])
    args = args[2:]
runs = {}
for a in args:
    name, path = a.split("=", 1)
    with open(path, newline="") as f:
        rows = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    rows.sort()
    per = {}
    for i, (b, e, k) in enumerate(rows):
        own = (e - b) * 1e-3
        b2b = (rows[i + 1][0] - b) * 1e-3 if i + 1 < len(rows) else own
        if b2b > own + GAP:
            b2b = own
        per.setdefault(k, []).append((b2b, own))
    runs[name] = per
kernels = []
for per in runs.values():
    for k in per:
        if k not in kernels:
            kernels.append(k)
short = lambda k: k.replace("void c3::", "").replace("c3::", "").split("(")[0]  # noqa: E731
print("%-64s %5s | " % ("kernel: median begin-to-begin us (median own duration us)", "n") + " | ".join("%-15s" % n for n in runs))
total = {n: 0.0 for n in runs}
for k in kernels:
    cells, cnt = [], 0
    for n, per in runs.items():
        v = per.get(k)
        if not v:
            cells.append(" " * 15)
            continue
        cnt = max(cnt, len(v))
        m = statistics.median(x[0] for x in v)
        total[n] += m
        cells.append("%6.2f (%6.2f)" % (m, statistics.median(x[1] for x in v)))
    print("%-64s %5d | " % (short(k)[:64], cnt) + " | ".join(cells))
print("%-64s %5s | " % ("sum of the medians", "") + " | ".join("%15.2f" % total[n] for n in runs))
