#!/usr/bin/env python3
"""Per-launch durations of the absorbed cross-attention's streaming kernel and of the skinny GEMMs next to it, by grid, from
rocprofv3 kernel traces of the bench command taken with different xa residency budgets (tools/profile.sh xa-trace).  The tracer
runs the passes in flight one after another, so these are LONE launches: the policy's effect on one launch (latency, Infinity
Cache hits from layer to layer of one pass), not on launches of several passes side by side.
usage: python tools/xa_trace_summary.py LABEL=trace.csv [LABEL=trace.csv ...]"""
import collections
import csv
import sys


def by_grid(path):
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        n = r["Kernel_Name"]
        if "cross_absorbed" in n and "kernel" in n and "absorb_q" not in n and "prologue" not in n:
            k = "cross_absorbed_v2_kernel" if "v2" in n else "cross_absorbed_kernel"
        elif "gemm_skinny" in n:
            k = "gemm_skinny_kernel"
        elif "cross_merge_proj" in n:
            k = "cross_merge_proj_kernel"
        else:
            continue
        grid = f'{int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1)}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]}'
        agg[(k, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return agg


def main():
    runs = [a.split("=", 1) for a in sys.argv[1:]]
    data = {label: by_grid(path) for label, path in runs}
    keys = sorted({k for d in data.values() for k in d}, key=lambda k: -sum(sum(d.get(k, [])) for d in data.values()))
    print(f"{'kernel':26s} {'grid':>10s} " + " ".join(f"{label + ' calls':>14s} {'avg us':>8s} {'med us':>8s}" for label, _ in runs))
    for k in keys[:14]:
        row = f"{k[0]:26s} {k[1]:>10s} "
        for label, _ in runs:
            v = sorted(data[label].get(k, []))
            row += f"{len(v):14d} {sum(v) / max(len(v), 1):8.2f} {(v[len(v) // 2] if v else 0):8.2f} "
        print(row)


if __name__ == "__main__":
    main()
