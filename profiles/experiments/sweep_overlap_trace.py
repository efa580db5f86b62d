#!/usr/bin/env python3
"""What a rocprofv3 kernel trace of the bench loop says about k_mark and k_alloc_sweep beside the ray march.
usage: sweep_overlap_trace.py <kernel_trace.csv> [frames to skip at the front, default 30]
       sweep_overlap_trace.py --dump <kernel_trace.csv> <first frame> <frames>     (the rows of some frames, times in us)
A frame runs from one k_integrate to the next.  Per steady-state frame: the kernels' durations, the queue each ran on,
where k_mark and k_alloc_sweep started and ended relative to the k_render they ran beside (for a sweep in the stream these
figures say where it sat behind it), k_publish_entries' duration, the idle gap in front of the first launch of the engine
stream behind k_render, and the frame period."""
import csv
import json
import statistics
import sys

NAMES = ("k_mark", "k_alloc_sweep", "k_publish_entries", "k_integrate", "k_fill_range_tiles", "k_render")


def short(name):
    for key in NAMES:
        if key in name:
            return key
    return None


def load(path):
    rows = []
    for r in csv.DictReader(open(path)):
        s = short(r["Kernel_Name"])
        if s:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, r["Queue_Id"]))
    rows.sort()
    return rows


def main():
    if sys.argv[1] == "--dump":
        rows = load(sys.argv[2])
        ints = [i for i, r in enumerate(rows) if r[2] == "k_integrate"]
        first, count = int(sys.argv[3]), int(sys.argv[4])
        a, b = ints[first], ints[first + count]
        t0 = rows[a][0]
        for r in rows[a:b + 1]:
            print("%9.2f %9.2f  q%-3s %s" % ((r[0] - t0) / 1e3, (r[1] - t0) / 1e3, r[3], r[2]))
        return
    path, skip = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 30
    rows = load(path)
    ints = [i for i, r in enumerate(rows) if r[2] == "k_integrate"]
    med = lambda v: round(statistics.median(v) / 1e3, 2) if v else None
    dur = {s: [] for s in NAMES}
    queues = {s: set() for s in NAMES}
    period, gap, inside = [], [], {"k_mark": 0, "k_alloc_sweep": 0}
    rel = {k: ([], []) for k in inside}
    frames = 0
    for a, b in zip(ints[skip:-1], ints[skip + 1:]):
        frame = rows[a:b]   # integrate(i) ... whatever ran in front of integrate(i + 1)
        names = [r[2] for r in frame]
        if names.count("k_render") != 1 or names.count("k_mark") != 1 or names.count("k_alloc_sweep") != 1:
            continue   # (not a steady-state frame of the loop)
        frames += 1
        period.append(rows[b][0] - frame[0][0])
        for r in frame:
            dur[r[2]].append(r[1] - r[0])
            queues[r[2]].add(r[3])
        render = next(r for r in frame if r[2] == "k_render")
        main_q = render[3]
        behind = [r for r in frame + [rows[b]] if r[3] == main_q and r[0] >= render[1]]
        if behind:
            gap.append(behind[0][0] - render[1])
        for k in inside:
            x = next(r for r in frame if r[2] == k)
            rel[k][0].append(x[0] - render[0])
            rel[k][1].append(x[1] - render[1])
            inside[k] += render[0] <= x[0] and x[1] <= render[1]
    out = {"frames": frames, "frame_period_us_median": med(period),
           "kernel_us_median": {s: med(v) for s, v in dur.items() if v},
           "queues": {s: sorted(q) for s, q in queues.items() if q},
           "idle_behind_k_render_on_its_queue_us_median": med(gap)}
    for k in inside:
        out[k + "_start_minus_k_render_start_us_median"] = med(rel[k][0])
        out[k + "_end_minus_k_render_end_us_median"] = med(rel[k][1])
        out["frames_with_" + k + "_inside_k_render"] = inside[k]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
