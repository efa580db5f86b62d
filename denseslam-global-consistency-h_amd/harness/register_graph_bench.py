"""Cost of the joint map registration (dslam_register_graph) on 3 and on 4 consecutive S-street local maps.

The drive is split into local maps as register_bench.py does it (a new map every K keyframes, anchored at that keyframe's
pose, every keyframe fused into the newest map at its pose relative to that map).  Pairs: every two neighbouring maps in
both directions, (0, 1), (1, 0), (1, 2), (2, 1), ...; anchor: map 0; starts: the true poses, every free map moved 0.5
voxel / 2 mrad off.  Reported per map count:
  * one call that evaluates once (max_evaluations = 1: the ordered compactions of the sources' entries, the read-back of
    their counts, one k_register_graph launch and the host's sums of the partial rows);
  * one call with default parameters, its evaluations, and the time per further evaluation (the difference of the two
    calls over the further evaluations: one launch, one wait, the host's joint system);
  * the same pairs as P dslam_register_maps calls of one evaluation each (the pairwise path, unchanged by this feature);
  * the bytes the source walks read per joint evaluation (the live blocks' voxels, their table entries and the lists).
Wall clock per call (the calls wait for the stream themselves).  Prints one JSON line; with an argument `out.json` also
writes it.

The kernel's own time comes from a kernel trace of this script, one map count per traced run (`--maps N`, so that every
k_register_graph launch of the run has the same pairs), and `--kernel-stats N:stats.csv ...` then adds to an existing
out.json, per map count, k_register_graph's average time from the trace's kernel statistics and the rate of the source
walk inside the kernel (source_walk_bytes_per_evaluation over that time).

    python denseslam-global-consistency-h_amd/harness/register_graph_bench.py [reps] [out.json] [--maps 3,4]
    python denseslam-global-consistency-h_amd/harness/register_graph_bench.py --into out.json --kernel-stats 3:a.csv 4:b.csv
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
from register_bench import K, small_motion, timed  # noqa: E402

MAX_MAPS = 4


def merge_kernel_stats(out_path, specs):
    """Add k_register_graph's average kernel time (kernel-trace statistics, ns) to the runs of an existing out.json."""
    out = json.load(open(out_path))
    for spec in specs:
        n, path = spec.split(":", 1)
        row = next(r for r in csv.DictReader(open(path)) if "k_register_graph" in r["Name"])
        run = next(r for r in out["runs"] if r["maps"] == int(n))
        us = float(row["AverageNs"]) / 1e3
        run["k_register_graph_kernel_us"] = us
        run["k_register_graph_launches_in_trace"] = int(row["Calls"])
        run["source_walk_GBps_in_the_kernel"] = run["source_walk_bytes_per_evaluation"] / (us * 1e-6) / 1e9
    out["kernel_time_from"] = "kernel trace statistics of this script, one traced run per map count (5 repetitions)"
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reps", nargs="?", type=int, default=20)
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--maps", default="3,4")
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
    frames = [wl.frame(i) for i in range(MAX_MAPS * K)]
    view = eng.create_view(W, H)
    maps, Ts = [], []
    for j in range(MAX_MAPS):
        s = eng.create_scene(p)
        rs = eng.create_render_state(s, W, H)
        T = np.asarray(frames[j * K][2], np.float32)
        Tinv = np.linalg.inv(T.astype(np.float64))
        for i in range(j * K, j * K + K):
            rgba, mm, M = frames[i]
            eng.view_update(view, rgba, mm, timestamp=float(i))
            eng.process_frame(s, view, rs, (np.asarray(M, np.float64) @ Tinv).astype(np.float32), intr)
        maps.append(s)
        Ts.append(T)
    eng.synchronize()
    live = [int((eng.download_hash_table(s)["ptr"] >= 0).sum()) for s in maps]
    off = small_motion(2e-3, (0.42, -0.61, 0.67), np.array([0.6, -0.64, 0.48]) * 0.5 * p.voxel_size)
    one = pkg.RegisterParams(max_evaluations=1)
    runs = []
    for n in counts:
        pairs = [pr for i in range(n - 1) for pr in ((i, i + 1), (i + 1, i))]
        start = np.stack([Ts[0]] + [(off @ Ts[i].astype(np.float64)).astype(np.float32) for i in range(1, n)])
        X0 = [(start[d].astype(np.float64) @ np.linalg.inv(start[s].astype(np.float64))).astype(np.float32) for s, d in pairs]
        _, r1, p1 = eng.register_graph(maps[:n], start, pairs, 0, one)
        T, rd, pd = eng.register_graph(maps[:n], start, pairs, 0)
        t_one = timed(lambda: eng.register_graph(maps[:n], start, pairs, 0, one), reps)
        t_call = timed(lambda: eng.register_graph(maps[:n], start, pairs, 0), reps)

        def pairwise():
            for (s, d), X in zip(pairs, X0):
                eng.register_maps(maps[s], maps[d], X, one)

        t_pairwise = timed(pairwise, reps)
        walk = sum(live[s] * (512 * 8 + 16 + 4) for s, _ in pairs)
        dist = []
        for i in range(1, n):
            err = T[i].astype(np.float64) @ np.linalg.inv(Ts[i].astype(np.float64))
            dist.append(float(np.linalg.norm(err[:3, 3]) / p.voxel_size))
        runs.append({"maps": n, "pairs": len(pairs), "active_pairs": r1.active_pairs,
                     "source_live_blocks": [live[s] for s, _ in pairs],
                     "candidates": [q.candidates for q in p1], "valid_at_start": [q.valid_first for q in p1],
                     "source_walk_bytes_per_evaluation": walk,
                     "call_one_evaluation_ms": t_one,
                     "call_default_ms": t_call, "call_default_evaluations": rd.evaluations,
                     "call_default_stop_reason": rd.stop_reason,
                     "further_evaluation_ms": (t_call - t_one) / max(rd.evaluations - 1, 1),
                     "pairwise_one_evaluation_calls_ms": t_pairwise, "pairwise_per_pair_ms": t_pairwise / len(pairs),
                     "cost_first": rd.cost_first, "cost_last": rd.cost_last, "conditioning": rd.conditioning,
                     "end_translation_error_voxels": dist})
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call (wall clock; the calls wait for the stream)", "runs": runs}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
