"""Cost of the photometric term in the depth-to-SDF tracker (dslam_track_camera_sdf_rgb) on the
S-street drive, against dslam_track_camera_sdf of the same library on the same frames and starts.

Set up as track_sdf_bench.py: a new local map every K keyframes, anchored at that keyframe's pose, every keyframe fused
(with its colours) into the newest map; frames between keyframes, 640x480, tracked from their true pose moved by
1 voxel / 5 mrad.  For N = 1, 4, 8 maps:
  * one level-0 evaluation of either call (no_hierarchy_levels = 1, max_evaluations = 1): the term adds arithmetic and one
    image read per pixel, and no voxel traffic -- the expectation this measurement confirms or refutes;
  * a whole default call of either: ms, evaluations, ms per evaluation, the pose error against the synthetic ground truth;
  * the colour-valid share and the colour rms at the returned pose.
Wall clock per call on a synchronous engine (every call waits for the stream itself); one warm-up round, then `reps`
rounds with the variants alternated inside each round; the median is reported.  The grey pyramid is built per call and is
part of both of the rgb call's figures.  Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/track_sdf_rgb_bench.py [reps] [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402
from track_sdf_bench import K, TRACKED, clock, pose_error, rigid  # noqa: E402  (the same directory)

N_MAX = 8


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 5
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
    eval0_rgb = pkg.TrackSdfRgbParams(no_hierarchy_levels=1, max_evaluations=1)

    rows = []
    for n in (1, 4, 8):
        scenes, Tn = maps[:n], Ts[:n]
        for f in tracked:
            variants = {
                "rgb_call": lambda: eng.track_camera_sdf_rgb(f["view"], scenes, Tn, f["start"], intr),
                "sdf_call": lambda: eng.track_camera_sdf(f["view"], scenes, Tn, f["start"], intr),
                "rgb_level0_evaluation": lambda: eng.track_camera_sdf_rgb(f["view"], scenes, Tn, f["start"], intr, eval0_rgb),
                "sdf_level0_evaluation": lambda: eng.track_camera_sdf(f["view"], scenes, Tn, f["start"], intr, eval0),
            }
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
            M_rgb, r_rgb = last["rgb_call"]
            M_sdf, r_sdf = last["sdf_call"]
            r0 = last["rgb_level0_evaluation"][1]
            row["rgb_evaluations"], row["sdf_evaluations"] = r_rgb.base.evaluations, r_sdf.evaluations
            row["rgb_ms_per_evaluation"] = row["rgb_call_ms"] / max(r_rgb.base.evaluations, 1)
            row["sdf_ms_per_evaluation"] = row["sdf_call_ms"] / max(r_sdf.evaluations, 1)
            row["rgb_stop_reason"], row["sdf_stop_reason"] = r_rgb.base.stop_reason, r_sdf.stop_reason
            row["rgb_conditioning"], row["sdf_conditioning"] = r_rgb.base.conditioning, r_sdf.conditioning
            row["candidates"], row["valid_at_start"], row["colour_valid_at_start"] = r0.base.candidates, r0.base.valid_last, r0.colour_valid_last
            row["colour_valid_last"], row["colour_rms_last"] = r_rgb.colour_valid_last, r_rgb.colour_rms_last
            for name, M in (("start", f["start"]), ("rgb", M_rgb), ("sdf", M_sdf)):
                a, d = pose_error(M, f["M_true"], f["centre"], vs)
                row[f"{name}_error_mrad"], row[f"{name}_error_voxels"] = a, d
            rows.append(row)
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps, "tracked_frames": list(TRACKED),
           "unit": "ms per call, wall clock on a synchronous engine, median of the repetitions, variants alternated", "rows": rows}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as fo:
            fo.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
