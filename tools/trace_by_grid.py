#!/usr/bin/env python3
"""Kernel-trace CSV of rocprofv3 (--kernel-trace --output-format csv) -> the per-(kernel, grid) table the profiles/ folder keeps:
calls, total and average duration, sorted by total.  usage: python tools/trace_by_grid.py <kernel_trace.csv> "<header line>" [rows]"""
import collections
import csv
import sys


def short(name):
    n = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return n.split("(")[0][:80]


def main():
    path, header = sys.argv[1], sys.argv[2]
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 44
    agg = collections.defaultdict(lambda: [0, 0.0])
    for r in csv.DictReader(open(path)):
        key = (short(r["Kernel_Name"]), f'{int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]}')
        agg[key][0] += 1
        agg[key][1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    print(f"# {header}")
    print(f"# total kernel time {sum(v[1] for v in agg.values()) / 1e3:.2f} ms over {sum(v[0] for v in agg.values())} dispatches")
    for (k, g), (n, t) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:rows]:
        print(f"{k:82s} grid={g:>14s} calls={n:6d} total_ms={t / 1e3:9.2f} avg_us={t / n:9.2f}")


if __name__ == "__main__":
    main()
