#!/usr/bin/env python3
"""What a rocprofv3 kernel trace of the bench loop says about k_mark beside the ray march.
usage: mark_overlap_trace.py <kernel_trace.csv> [frames to skip at the front, default 30]
Per steady-state frame: the kernels' durations, the queue each ran on, where k_mark started and ended relative to the
k_render it ran beside, the idle gap in front of k_alloc_sweep, and the frame period (k_alloc_sweep to k_alloc_sweep)."""
import csv
import json
import statistics
import sys

SHORT = (("k_mark", "k_mark"), ("k_alloc_sweep", "k_alloc_sweep"), ("k_integrate", "k_integrate"),
         ("k_fill_range_tiles", "k_fill_range_tiles"), ("k_render", "k_render"), ("k_bits_select", "k_bits_select"))


def short(name):
    for key, s in SHORT:
        if key in name:
            return s
    return None


def main():
    path, skip = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rows = []
    for r in csv.DictReader(open(path)):
        s = short(r["Kernel_Name"])
        if s:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, r["Queue_Id"]))
    rows.sort()
    sweeps = [i for i, r in enumerate(rows) if r[2] == "k_alloc_sweep"]
    med = lambda v: round(statistics.median(v) / 1e3, 2) if v else None
    dur = {s: [] for _, s in SHORT}
    queues = {s: set() for _, s in SHORT}
    period, gap_before_sweep, mark_start_in_render, mark_end_in_render, inside = [], [], [], [], 0
    frames = 0
    for a, b in zip(sweeps[skip:-1], sweeps[skip + 1:]):
        frame = rows[a:b + 1]   # sweep(i) ... sweep(i + 1)
        names = [r[2] for r in frame[:-1]]
        if names.count("k_render") != 1 or names.count("k_mark") != 1:
            continue   # (not a steady-state frame of the loop)
        frames += 1
        period.append(frame[-1][0] - frame[0][0])
        for r in frame[:-1]:
            dur[r[2]].append(r[1] - r[0])
            queues[r[2]].add(r[3])
        render = next(r for r in frame if r[2] == "k_render")
        mark = next(r for r in frame[1:] if r[2] == "k_mark")
        # what ended last in front of the next sweep
        gap_before_sweep.append(frame[-1][0] - max(r[1] for r in frame[:-1]))
        mark_start_in_render.append(mark[0] - render[0])
        mark_end_in_render.append(mark[1] - render[1])
        inside += render[0] <= mark[0] and mark[1] <= render[1]
    out = {"frames": frames, "frame_period_us_median": med(period),
           "kernel_us_median": {s: med(v) for s, v in dur.items() if v},
           "queues": {s: sorted(q) for s, q in queues.items() if q},
           "k_mark_start_minus_k_render_start_us_median": med(mark_start_in_render),
           "k_mark_end_minus_k_render_end_us_median": med(mark_end_in_render),
           "frames_with_k_mark_inside_k_render": inside,
           "idle_in_front_of_k_alloc_sweep_us_median": med(gap_before_sweep),
           "idle_in_front_of_k_alloc_sweep_us_max": round(max(gap_before_sweep) / 1e3, 2) if gap_before_sweep else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
