"""Cost and accuracy of the depth-to-SDF tracker over local maps (dslam_track_camera_sdf) on the S-street drive.

The local maps are built as multimap_bench.py builds them: a new map every K keyframes, anchored at that keyframe's pose,
every keyframe fused into the newest map.  For N = 1, 2, 4, 8 maps and a few frames that lie between keyframes (the
trajectory is evaluated at half-integer indices, so their true poses are known), 640x480, each from its true pose moved by
1 voxel / 5 mrad:
  * dslam_track_camera_sdf over the first N maps with the default parameters: ms per call, evaluations (per level, from
    runs cut off above each level), ms per evaluation, and one level-0 evaluation alone;
  * the parent's yardsticks in the same run: dslam_create_icp_maps (Prepare) and dslam_track_camera on ONE map fused from
    the same keyframes, and -- for N > 1 -- the composite depth raycast dslam_get_image_multi a multi-map ICP would need
    before its first evaluation;
  * the maps holding a pixel on average: per map the pixels whose 8 taps it holds (one evaluation with the residual gate
    wide open), summed over the maps, over the candidates;
  * the pose error of both trackers against the synthetic ground truth (mrad, voxels at the centre of what the frame sees).
Wall clock per call on a synchronous engine (every call waits for the stream itself); one warm-up round, then `reps`
rounds with the variants alternated inside each round; the median is reported.  Prints one JSON line; with an argument
`out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/track_sdf_bench.py [reps] [out.json]
    python denseslam-global-consistency-h_amd/harness/track_sdf_bench.py order [reps]

`order`: only the level-0 evaluation at N = 1, 4, 8 -- the measurement behind the kernel's pixel order; run it once per
value of DSLAM_TRACK_SDF_PIXELS (rows, tiles), which a process reads once.
"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

K = 4          # keyframes per local map
N_MAX = 8
TRACKED = (0.5, 1.5, 2.5)


def rigid(angle, axis, t, centre):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + np.asarray(t, np.float64)
    return X


def pose_error(M, M_true, centre_cam, vs):
    """(mrad, voxels at `centre_cam`, a point in the true camera frame) between two world -> camera poses."""
    D = np.asarray(M, np.float64) @ np.linalg.inv(np.asarray(M_true, np.float64))
    ang = math.acos(max(-1.0, min(1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0)))
    c = np.append(centre_cam, 1.0)
    return 1e3 * ang, float(np.linalg.norm((D @ c - c)[:3]) / vs)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    order_only = len(sys.argv) > 1 and sys.argv[1] == "order"
    args = sys.argv[2:] if order_only else sys.argv[1:]
    reps = int(args[0]) if args else (20 if order_only else 5)
    out_path = args[1] if len(args) > 1 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    vs = p.voxel_size
    frames = [wl.frame(i) for i in range(K * N_MAX)]
    view = eng.create_view(W, H)
    maps, Ts = [], []
    for j in range(N_MAX):
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
    tracked = []
    for t in TRACKED:
        rgba, mm, M_true = wl.frame(t)
        z = mm[mm > 0].astype(np.float64) * 1e-3
        centre = np.array([0.0, 0.0, float(np.median(z))])
        start = (rigid(5e-3, (0.3, 0.8, -0.52), vs * np.array([0.6, -0.64, 0.48]), centre) @ M_true.astype(np.float64)).astype(np.float32)
        v = eng.create_view(W, H)
        eng.view_update(v, rgba, mm, timestamp=float(t))
        tracked.append(dict(t=t, view=v, M_true=M_true, start=start, centre=centre))
    eval0 = pkg.TrackSdfParams(no_hierarchy_levels=1, max_evaluations=1)
    open_gate = pkg.TrackSdfParams(no_hierarchy_levels=1, max_evaluations=1, residual_gate=1e9)

    if order_only:
        rows = []
        for n in (1, 4, 8):
            f = tracked[0]
            call = lambda: eng.track_camera_sdf(f["view"], maps[:n], Ts[:n], f["start"], intr, eval0)  # noqa: E731
            call()
            ms = sorted(clock(call)[0] for _ in range(reps))
            rows.append({"maps": n, "level0_evaluation_ms_median": ms[len(ms) // 2], "min": ms[0]})
        print(json.dumps({"pixels": os.environ.get("DSLAM_TRACK_SDF_PIXELS", "default"), "reps": reps, "rows": rows}))
        return

    rows = []
    for n in (1, 2, 4, 8):
        scenes, Tn = maps[:n], Ts[:n]
        s1 = eng.create_scene(p)           # one map fused from the same keyframes (world frame)
        rs1 = eng.create_render_state(s1, W, H)
        for i in range(n * K):
            rgba, mm, M = frames[i]
            eng.view_update(view, rgba, mm, timestamp=float(i))
            eng.process_frame(s1, view, rs1, M, intr)
        rs_multi = eng.create_render_state(scenes[0], W, H)
        for f in tracked:
            variants = {
                "sdf_call": lambda: eng.track_camera_sdf(f["view"], scenes, Tn, f["start"], intr),
                "sdf_level0_evaluation": lambda: eng.track_camera_sdf(f["view"], scenes, Tn, f["start"], intr, eval0),
                "icp_prepare": lambda: eng.create_icp_maps(s1, rs1, f["start"], intr, download=False),
                "icp_track": lambda: eng.track_camera(f["view"], rs1, f["start"], f["start"], intr),
            }
            if n > 1:
                variants["composite_depth"] = lambda: eng.get_image_multi(scenes, Tn, rs_multi, f["start"], intr, pkg.IMAGE_DEPTH,
                                                                          download=False)
            times = {k: [] for k in variants}
            last = {}
            for r in range(reps + 1):       # round 0 warms up
                for k, fn in variants.items():
                    ms, out = clock(fn)
                    if r:
                        times[k].append(ms)
                    last[k] = out
            row = {"maps": n, "frame": f["t"]}
            for k, v in times.items():
                row[k + "_ms"] = sorted(v)[len(v) // 2]
            M_sdf, r_sdf = last["sdf_call"]
            M_icp, r_icp = last["icp_track"]
            row["sdf_evaluations"] = r_sdf.evaluations
            upto = [eng.track_camera_sdf(f["view"], scenes, Tn, f["start"], intr, pkg.TrackSdfParams(run_till_level=lv))[1].evaluations
                    for lv in (2, 1)]
            row["sdf_evaluations_per_level"] = {"2": upto[0], "1": upto[1] - upto[0], "0": r_sdf.evaluations - upto[1]}
            row["sdf_ms_per_evaluation"] = row["sdf_call_ms"] / max(r_sdf.evaluations, 1)
            row["sdf_stop_reason"], row["sdf_valid"], row["sdf_candidates"] = r_sdf.stop_reason, r_sdf.valid_last, r_sdf.candidates
            row["icp_iterations"] = r_icp.iterations
            held = sum(eng.track_camera_sdf(f["view"], [s], [T], f["M_true"], intr, open_gate)[1].valid_last
                       for s, T in zip(scenes, Tn))
            row["maps_holding_a_pixel"] = held / max(r_sdf.candidates, 1)
            for name, M in (("start", f["start"]), ("sdf", M_sdf), ("icp", M_icp)):
                a, d = pose_error(M, f["M_true"], f["centre"], vs)
                row[f"{name}_error_mrad"], row[f"{name}_error_voxels"] = a, d
            rows.append(row)
        del s1, rs1, rs_multi
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps, "tracked_frames": list(TRACKED),
           "pixels": os.environ.get("DSLAM_TRACK_SDF_PIXELS", "default"),
           "unit": "ms per call, wall clock on a synchronous engine, median of the repetitions, variants alternated", "rows": rows}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fo:
            fo.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
