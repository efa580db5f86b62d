"""Cost of the view survey (dslam_survey_views + dslam_select_view_maps) and what it saves, on the S-street drive.

The local maps are built as multimap_bench.py builds them: a new map every K keyframes, anchored at that keyframe's pose,
every keyframe fused into the newest map.  For N = 8, 16, 32 and 64 maps along the street, 640x480, the frame half way
between the two middle keyframes of the listed stretch (the maps behind the camera and those beyond the depth range cannot
be reached), from its true pose moved by 1 voxel / 5 mrad:
  * dslam_survey_views of the N maps from that start pose (near 0, far = the frame's largest depth) and
    dslam_select_view_maps with the current map -- the one the frame lies in -- always kept; for the raycast, which draws
    whatever its rays meet, a second list from a survey without a far plane;
  * with the full list and with the surveyed list: one level-0 evaluation of dslam_track_camera_sdf, the whole call with
    its default parameters, and the composite depth raycast dslam_get_image_multi;
  * how many maps each list holds, and whether the two lists give the same bytes (pose and result; depth image).
And the survey alone over 128 maps with small pools (one keyframe each).
Wall clock per call on a synchronous engine (every call waits for the stream itself); one warm-up round, then `reps`
rounds with the variants alternated inside each round; the median is reported.  No time was fixed in advance: the JSON
says at which N survey + select pays for itself within one tracker call and within one raycast.  Prints one JSON line;
with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/view_survey_bench.py [reps] [out.json]
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
N_LIST = (8, 16, 32, 64)
N_SMALL = 128


def rigid(angle, axis, t, centre):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    X = np.eye(4)
    X[:3, :3] = R
    X[:3, 3] = np.asarray(centre) - R @ np.asarray(centre) + np.asarray(t, np.float64)
    return X


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    vs = p.voxel_size
    n_max = max(N_LIST)
    frames = [wl.frame(i) for i in range(K * n_max)]
    view = eng.create_view(W, H)
    maps, Ts = [], []
    for j in range(n_max):
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
        del rs
    eng.synchronize()
    eval0 = pkg.TrackSdfParams(no_hierarchy_levels=1, max_evaluations=1)

    rows = []
    for n in N_LIST:
        scenes, Tn = maps[:n], np.stack(Ts[:n])
        t = n * K / 2 + 0.5
        current = int(t) // K
        rgba, mm, M_true = wl.frame(t)
        z = mm[mm > 0].astype(np.float64) * 1e-3
        centre = np.array([0.0, 0.0, float(np.median(z))])
        start = (rigid(5e-3, (0.3, 0.8, -0.52), vs * np.array([0.6, -0.64, 0.48]), centre) @ M_true.astype(np.float64)).astype(np.float32)
        v = eng.create_view(W, H)
        eng.view_update(v, rgba, mm, timestamp=float(t))
        far = float(z.max()) + 0.001
        cam = [pkg.SurveyView.of(start, intr, W, H, 0.0, far)]
        select = pkg.ViewSelectParams(always_keep=current)
        live, reach, nearest, farthest = eng.survey_views(scenes, Tn, cam)
        keep, res = eng.select_view_maps(reach, nearest, select)
        sub, T_sub = [scenes[i] for i in keep], Tn[keep]
        # the renderer draws whatever a ray meets, not only what the frame's depth image holds: its list has no far plane
        cam_r = [pkg.SurveyView.of(start, intr, W, H, 0.0, 0.0)]
        _, reach_r, nearest_r, _ = eng.survey_views(scenes, Tn, cam_r)
        keep_r, res_r = eng.select_view_maps(reach_r, nearest_r, select)
        sub_r, T_sub_r = [scenes[i] for i in keep_r], Tn[keep_r]
        rs_multi = eng.create_render_state(scenes[0], W, H)
        variants = {
            "survey": lambda: eng.survey_views(scenes, Tn, cam),
            "select": lambda: eng.select_view_maps(reach, nearest, select),
            "full_level0_evaluation": lambda: eng.track_camera_sdf(v, scenes, Tn, start, intr, eval0),
            "kept_level0_evaluation": lambda: eng.track_camera_sdf(v, sub, T_sub, start, intr, eval0),
            "full_tracker_call": lambda: eng.track_camera_sdf(v, scenes, Tn, start, intr),
            "kept_tracker_call": lambda: eng.track_camera_sdf(v, sub, T_sub, start, intr),
            "full_composite_depth": lambda: eng.get_image_multi(scenes, Tn, rs_multi, start, intr, pkg.IMAGE_DEPTH, download=False),
            "kept_composite_depth": lambda: eng.get_image_multi(sub_r, T_sub_r, rs_multi, start, intr, pkg.IMAGE_DEPTH, download=False),
        }
        times = {k: [] for k in variants}
        last = {}
        for r in range(reps + 1):       # round 0 warms up
            for k, fn in variants.items():
                ms, out = clock(fn)
                last[k] = out
                if r:
                    times[k].append(ms)
        row = {"maps": n, "tracked_frame": t, "current_map": current, "far_m": far, "live_blocks": int(live.sum()),
               "maps_reaching": int(res.reaching), "maps_kept": int(res.selected), "kept": keep.tolist(), "maps_kept_for_the_raycast": int(res_r.selected),
               "kept_for_the_raycast": keep_r.tolist()}
        for k in variants:
            row[k + "_ms"] = median(times[k])
        full, kept = last["full_tracker_call"], last["kept_tracker_call"]
        row["tracker_evaluations"] = int(full[1].evaluations)
        row["tracker_bytes_equal"] = bool(full[0].tobytes() == kept[0].tobytes() and bytes(full[1]) == bytes(kept[1]))
        d_full = eng.get_image_multi(scenes, Tn, rs_multi, start, intr, pkg.IMAGE_DEPTH)
        d_kept = eng.get_image_multi(sub_r, T_sub_r, rs_multi, start, intr, pkg.IMAGE_DEPTH)
        row["composite_depth_pixels_differing"] = int((d_full.view(np.uint32) != d_kept.view(np.uint32)).sum())
        overhead = row["survey_ms"] + row["select_ms"]
        row["survey_plus_select_ms"] = overhead
        row["tracker_call_saved_ms"] = row["full_tracker_call_ms"] - row["kept_tracker_call_ms"]
        row["composite_saved_ms"] = row["full_composite_depth_ms"] - row["kept_composite_depth_ms"]
        row["level0_saved_us_per_dropped_map"] = (1e3 * (row["full_level0_evaluation_ms"] - row["kept_level0_evaluation_ms"])
                                                  / max(1, n - int(res.selected)))
        row["pays_within_one_tracker_call"] = bool(row["tracker_call_saved_ms"] > overhead)
        row["pays_within_one_raycast"] = bool(row["composite_saved_ms"] > overhead)
        rows.append(row)
        del rs_multi, v

    # the survey alone over 128 maps with small pools
    small_p = pkg.SceneParams(num_local_blocks=0x4000, num_buckets=0x8000, num_excess=0x2000, **wl.scene_kwargs)
    small, T_small = [], []
    for j in range(N_SMALL):
        s = eng.create_scene(small_p)
        rs = eng.create_render_state(s, W, H)
        rgba, mm, M = frames[2 * j]
        eng.view_update(view, rgba, mm, timestamp=float(j))
        eng.process_frame(s, view, rs, np.eye(4, dtype=np.float32), intr)
        small.append(s)
        T_small.append(np.asarray(M, np.float32))
        del rs
    eng.synchronize()
    T_small = np.stack(T_small)
    cam = [pkg.SurveyView.of(np.asarray(frames[N_SMALL][2], np.float32), intr, W, H, 0.0, 40.0)]
    eng.survey_views(small, T_small, cam)
    ms = [clock(lambda: eng.survey_views(small, T_small, cam))[0] for _ in range(4 * reps)]
    live, reach, nearest, _ = eng.survey_views(small, T_small, cam)
    keep, res = eng.select_view_maps(reach, nearest)
    small_row = {"maps": N_SMALL, "table_entries_per_map": 0x8000 + 0x2000, "live_blocks": int(live.sum()), "survey_ms": median(ms),
                 "survey_ms_min": min(ms), "maps_reaching": int(res.reaching), "maps_kept": int(res.selected)}

    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call, median (wall clock, synchronous engine: every call waits for the stream)",
           "rows": rows, "survey_alone_small_pools": small_row,
           "pays_within_one_tracker_call_from_maps": next((r["maps"] for r in rows if r["pays_within_one_tracker_call"]), None),
           "pays_within_one_raycast_from_maps": next((r["maps"] for r in rows if r["pays_within_one_raycast"]), None)}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
