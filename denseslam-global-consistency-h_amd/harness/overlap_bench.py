"""Cost of the overlap survey (dslam_survey_overlaps) and of the pair selection on 4, 8 and 16 consecutive S-street local maps.

Local maps of K = 4 keyframes each (640x480, the maps register_graph_bench.py builds: the poses of map j relative to its
first keyframe, whose pose is the map's world -> map transform).  Per map count N:
  * the live blocks and the probes of a call, 8 * sum(live) * (N - 1);
  * wall clock of dslam_survey_overlaps (the compactions, the read-back of the counts, one k_survey_overlaps launch, the
    wait and the host's sums of the rows) and of dslam_select_register_pairs with its defaults;
  * for N <= 8, where all N (N - 1) ordered pairs fit DSLAM_MAX_REGISTER_PAIRS: wall clock of the way to learn the same
    thing without the survey, one dslam_register_graph with max_evaluations = 1 over all ordered pairs, and per pair
    valid_first / shared_octants.
Kernel time: run the script under a kernel trace with statistics, once, in an invocation of its own (`--maps 16` keeps
every k_survey_overlaps launch of the run alike), and `--kernel-stats N:stats.csv ...` then adds k_survey_overlaps'
average time to an existing out.json.

    python denseslam-global-consistency-h_amd/harness/overlap_bench.py [reps] [out.json] [--maps 4,8,16]
    python denseslam-global-consistency-h_amd/harness/overlap_bench.py --into out.json --kernel-stats 4:a.csv 16:b.csv
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from register_bench import K, timed  # noqa: E402


def merge_kernel_stats(out_path, specs):
    """Add k_survey_overlaps' average kernel time (kernel-trace statistics, ns) to the runs of an existing out.json."""
    out = json.load(open(out_path))
    for spec in specs:
        n, path = spec.split(":", 1)
        row = next(r for r in csv.DictReader(open(path)) if "k_survey_overlaps" in r["Name"])
        run = next(r for r in out["runs"] if r["maps"] == int(n))
        us = float(row["AverageNs"]) / 1e3
        run["k_survey_overlaps_kernel_us"] = us
        run["k_survey_overlaps_launches_in_trace"] = int(row["Calls"])
        run["probes_per_second_in_the_kernel"] = run["probes_per_call"] / (us * 1e-6)
    out["kernel_time_from"] = "kernel trace statistics of this script, one traced run per map count (5 repetitions)"
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=20)
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--maps", default="4,8,16")
    ap.add_argument("--kernel-stats", nargs="+", metavar="N:CSV", default=None)
    ap.add_argument("--into", default=None, help="the out.json --kernel-stats adds to")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.into, args.kernel_stats)
    reps, out_path = args.reps, args.out
    counts = [int(v) for v in args.maps.split(",")]
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    view = eng.create_view(W, H)
    maps, states, Ts = [], [], []
    for j in range(max(counts)):
        s = eng.create_scene(p)
        rs = eng.create_render_state(s, W, H)
        frames = [wl.frame(i) for i in range(j * K, j * K + K)]
        T = np.asarray(frames[0][2], np.float32)
        Tinv = np.linalg.inv(T.astype(np.float64))
        for i, (rgba, mm, M) in enumerate(frames):
            eng.view_update(view, rgba, mm, timestamp=float(j * K + i))
            eng.process_frame(s, view, rs, (np.asarray(M, np.float64) @ Tinv).astype(np.float32), intr)
        maps.append(s)
        states.append(rs)
        Ts.append(T)
    eng.synchronize()
    one = pkg.RegisterParams(max_evaluations=1)
    runs = []
    for n in counts:
        T = np.stack(Ts[:n])
        live, blocks, octants = eng.survey_overlaps(maps[:n], T)
        pairs, component, sel = eng.select_register_pairs(live, octants)
        t_survey = timed(lambda: eng.survey_overlaps(maps[:n], T), reps)
        l32, o32 = np.ascontiguousarray(live), np.ascontiguousarray(octants)
        t_select = timed(lambda: eng.select_register_pairs(l32, o32), reps)
        run = {"maps": n, "live_blocks": live.tolist(), "probes_per_call": int(8 * int(live.sum()) * (n - 1)),
               "survey_ms": t_survey, "select_ms": t_select,
               "shared_octants": octants.tolist(), "shared_blocks": blocks.tolist(),
               "qualifying_pairs": sel.qualifying, "selected_pairs": sel.selected, "components": sel.num_components}
        ordered = [(s, d) for s in range(n) for d in range(n) if s != d]
        if len(ordered) <= pkg.MAX_REGISTER_PAIRS:
            _, r1, p1 = eng.register_graph(maps[:n], T, ordered, 0, one)
            run["register_graph_one_evaluation_all_ordered_pairs_ms"] = timed(lambda: eng.register_graph(maps[:n], T, ordered, 0, one), reps)
            run["ordered_pairs"] = len(ordered)
            run["survey_share_of_that_call"] = t_survey / run["register_graph_one_evaluation_all_ordered_pairs_ms"]
            run["valid_first_over_shared_octants"] = [
                {"pair": [s, d], "valid_first": q.valid_first, "shared_octants": int(octants[s, d]),
                 "ratio": (q.valid_first / int(octants[s, d])) if octants[s, d] else None} for (s, d), q in zip(ordered, p1)]
            run["pairs_active_at_min_valid_500_but_below_64_shared_octants"] = [
                [s, d] for (s, d), q in zip(ordered, p1) if q.valid_first >= 500 and octants[s, d] < 64]
        runs.append(run)
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call (wall clock; the calls wait for the stream)", "runs": runs}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
