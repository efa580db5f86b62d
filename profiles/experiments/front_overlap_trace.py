#!/usr/bin/env python3
"""What a rocprofv3 kernel trace of the bench loop says about GetImage's front end on the auxiliary stream.
usage: front_overlap_trace.py <kernel_trace.csv> [frames to skip at the front, default 30]
       front_overlap_trace.py --dump <kernel_trace.csv> <first frame> <frames>     (the rows of some frames, times in us)
A frame runs from one k_integrate to the next.  Per steady-state frame: the kernels' durations and the queue each ran on;
where k_mark, k_alloc_sweep, the selection (k_bits_select) and the range pass started and ended relative to the k_render
they ran beside and relative to the fusion launch that follows them; the idle gap behind k_render on its queue; whether the
fusion launch is the plain instantiation; the frame period."""
import csv
import json
import statistics
import sys

NAMES = ("k_mark", "k_alloc_sweep", "k_publish_entries", "k_integrate", "k_bits_select", "k_fill_range_tiles", "k_render")
AUX = ("k_mark", "k_alloc_sweep", "k_bits_select", "k_fill_range_tiles")


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
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), s, r["Queue_Id"], r["Kernel_Name"]))
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
    period, gap = [], []
    rel = {k: ([], [], [], []) for k in AUX}
    inside = {k: 0 for k in AUX}
    fusion_names = set()
    frames = 0
    for a, b in zip(ints[skip:-1], ints[skip + 1:]):
        frame = rows[a:b]   # integrate(i) ... whatever ran in front of integrate(i + 1)
        names = [r[2] for r in frame]
        if names.count("k_render") != 1 or names.count("k_mark") != 1 or names.count("k_alloc_sweep") != 1:
            continue   # (not a steady-state frame of the loop)
        frames += 1
        period.append(rows[b][0] - frame[0][0])
        fusion_names.add(rows[b][4])
        for r in frame:
            dur[r[2]].append(r[1] - r[0])
            queues[r[2]].add(r[3])
        render = next(r for r in frame if r[2] == "k_render")
        behind = [r for r in frame + [rows[b]] if r[3] == render[3] and r[0] >= render[1]]
        if behind:
            gap.append(behind[0][0] - render[1])
        for k in AUX:
            xs = [r for r in frame if r[2] == k]
            if len(xs) != 1:
                continue
            x = xs[0]
            rel[k][0].append(x[0] - render[0])
            rel[k][1].append(x[1] - render[1])
            rel[k][2].append(x[0] - rows[b][0])
            rel[k][3].append(x[1] - rows[b][1])
            inside[k] += render[0] <= x[0] and x[1] <= render[1]
    q = sorted(period)
    out = {"frames": frames, "frame_period_us_median": med(period),
           "frame_period_us_p10_p90": [round(q[len(q) // 10] / 1e3, 2), round(q[(len(q) * 9) // 10] / 1e3, 2)] if q else None,
           "kernel_us_median": {s: med(v) for s, v in dur.items() if v},
           "queues": {s: sorted(q) for s, q in queues.items() if q},
           "idle_behind_k_render_on_its_queue_us_median": med(gap),
           "fusion_launch_instantiations": sorted(fusion_names)}
    for k in AUX:
        if not rel[k][0]:
            continue
        out[k] = {"start_minus_k_render_start_us_median": med(rel[k][0]), "end_minus_k_render_end_us_median": med(rel[k][1]),
                  "start_minus_next_fusion_start_us_median": med(rel[k][2]), "end_minus_next_fusion_end_us_median": med(rel[k][3]),
                  "frames_inside_k_render": inside[k]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
