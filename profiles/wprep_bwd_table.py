"""Kernel durations of the expert scatter per layer shape, serial against expert-split form, from two rocprofv3
--kernel-trace csvs of profiles/microbench_wprep_bwd.py (COMA_WPREP_BWD_SPLIT=0 and =1).

    python profiles/wprep_bwd_table.py <serial kernel_trace.csv> <split kernel_trace.csv>"""
import csv
import statistics
import sys

from microbench_wprep_bwd import ITERS, SHAPES


def durations(path):
    with open(path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "weight_prep_bwd27_k" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows]
    assert len(us) == ITERS * len(SHAPES), (len(us), ITERS * len(SHAPES))
    return [statistics.median(us[i * ITERS + 2:(i + 1) * ITERS]) for i in range(len(SHAPES))]      # (the first two: cold)


if __name__ == "__main__":
    serial, split = durations(sys.argv[1]), durations(sys.argv[2])
    print("expert scatter, E = 8, batch 2: median kernel duration (us) of weight_prep_bwd27_k, rocprofv3 --kernel-trace")
    print(f"{'layer':>14s} {'blocks':>7s} {'serial':>8s} {'split':>8s}")
    for (cin, cout, tr), a, b in zip(SHAPES, serial, split):
        print(f"{cin:5d}->{cout:4d} {'T' if tr else ' '} {(cin * cout + 255) // 256:7d} {a:8.1f} {b:8.1f}")
