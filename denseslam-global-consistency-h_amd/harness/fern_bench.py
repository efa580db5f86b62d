"""The fern keyframe index (dslam_fern_*): what encoding and searching cost, and the pose-free
relocaliser chain end to end on S-room and S-street at 640x480.

  * encode: dslam_fern_encode of a 640x480 view that reads a frame-store slot in place, channels 1 and 2, next to
    dslam_view_update_from_store (UpdateView from the store) and to the same call on an 8x8 view -- two launches, one copy
    back and one wait with next to nothing to read: the launch floor of the call's shape;
  * scan: dslam_fern_query_stored over N = 1 k, 16 k, 150 k stored codes with 1 and 64 queries, k = 16, the whole range as
    the window; bytes per second over 256 N.  dslam_score_camera_poses over 256 poses, the only other way a caller has to
    test that many hypotheses, is measured in the same run on the street map (pyramid levels 2 and 0);
  * chain: the keyframe store is filled while one map is fused, the index is built from it with one
    dslam_fern_add_from_store, frames between the keyframe poses are queried (k = 4), the matched keyframes' poses go to
    dslam_track_camera_sdf_starts as the starts, the estimates are scored (dslam_score_camera_poses) and the best is kept
    (dslam_select_start_poses).  The yardstick is the tracker's own answer: dslam_track_camera_sdf from the TRUE pose.  A
    query counts as relocalised when the chain's pose lies within 1 voxel (at the median depth) and 5 mrad of that answer.

Wall clock per call on an otherwise idle synchronous engine (every call waits for the stream itself), one warm-up call, then
`reps` calls; median, 10th and 90th percentile.  Prints one JSON line and writes profiles/fern_bench.json (or the path given).

    python denseslam-global-consistency-h_amd/harness/fern_bench.py [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
from track_sdf_bench import pose_error  # noqa: E402  (the same directory)

HBM_PEAK = 8.0e12     # bytes per second: the peak DESIGN.md section 4 measures against
SCAN_N = (1000, 16000, 150000)


def spread(fn, reps):
    """{median, p10, p90} microseconds per call of fn, after one warm-up call."""
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    return {"median_us": round(t[len(t) // 2], 2), "p10_us": round(t[len(t) // 10], 2), "p90_us": round(t[(9 * len(t)) // 10], 2)}


def bench_encode(pkg, eng, wl, reps):
    W, H = wl.W, wl.H
    rgba, mm, _ = wl.frame(0)
    store = eng.create_frame_store(W, H, 2)
    eng.frame_store_put(store, 0, rgba, mm)
    view = eng.create_view(W, H)
    out = {"image": f"{W}x{H}", "view_update_from_store": spread(lambda: eng.view_update_from_store(view, store, 0), reps),
           "engine_synchronize": spread(eng.synchronize, reps)}
    for channels, nbytes in ((1, W * H * 2), (2, W * H * 6)):
        idx = eng.create_fern_index(W, H, 4, pkg.FernParams(channels=channels))
        row = spread(lambda: eng.fern_encode(idx, view), reps)
        row["image_bytes"] = nbytes
        row["image_bytes_per_second_at_median"] = round(nbytes / (row["median_us"] * 1e-6), 0)
        out[f"fern_encode_channels_{channels}"] = row
        out[f"fern_query_empty_index_channels_{channels}"] = spread(lambda: eng.fern_query(idx, view, 0, 4, 4), reps)
        idx.close()
    small = eng.create_view(8, 8)
    eng.view_update(small, np.zeros((8, 8, 4), np.uint8), np.full((8, 8), 1000, np.int16))
    idx = eng.create_fern_index(8, 8, 4, pkg.FernParams(cell=1))
    out["fern_encode_8x8_launch_floor"] = spread(lambda: eng.fern_encode(idx, small), reps)
    return out


def bench_scan(pkg, eng, reps):
    rng = np.random.RandomState(3)
    store = eng.create_frame_store(8, 8, 1000)
    rgba = np.zeros((8, 8, 4), np.uint8)
    for s in range(1000):
        eng.frame_store_put(store, s, rgba, rng.randint(300, 9000, size=(8, 8)).astype(np.int16))
    rows = []
    for n in SCAN_N:
        idx = eng.create_fern_index(8, 8, n, pkg.FernParams(cell=1, depth_max_mm=9000))
        t0 = time.perf_counter()
        for first in range(0, n, 1000):
            eng.fern_add_from_store(idx, store, 0, min(1000, n - first))
        build_ms = (time.perf_counter() - t0) * 1e3
        for nq in (1, 64):
            ids = rng.randint(0, n, size=nq).tolist()
            row = spread(lambda: eng.fern_query_stored(idx, ids, 0, n, 16), reps)
            row.update(codes=n, queries=nq, k=16, code_bytes=256 * n, add_from_store_calls_of_1000_ms=round(build_ms, 2))
            row["code_bytes_per_second_at_median"] = round(256 * n / (row["median_us"] * 1e-6), 0)
            row["fraction_of_hbm_peak"] = round(row["code_bytes_per_second_at_median"] / HBM_PEAK, 4)
            rows.append(row)
        idx.close()
    return rows


def build_map(pkg, eng, wl, key_frames):
    """One map fused from the keyframes, the keyframe store filled on the way."""
    p = pkg.SceneParams(**wl.scene_kwargs)
    scene = eng.create_scene(p)
    rs, view = eng.create_render_state(scene, wl.W, wl.H), eng.create_view(wl.W, wl.H)
    store = eng.create_frame_store(wl.W, wl.H, len(key_frames))
    poses = []
    for slot, i in enumerate(key_frames):
        rgba, mm, M = wl.frame(i)
        eng.view_update(view, rgba, mm, timestamp=float(i))
        eng.frame_store_put_view(store, slot, view)
        eng.process_frame(scene, view, rs, M, wl.intr)
        poses.append(np.asarray(M, np.float32))
    return scene, store, poses, view, p.voxel_size


def bench_chain(pkg, eng, wl, key_step, n_keys, query_offsets, params, reps):
    key_frames = [key_step * j for j in range(n_keys)]
    scene, store, key_poses, view, vs = build_map(pkg, eng, wl, key_frames)
    idx = eng.create_fern_index(wl.W, wl.H, n_keys, params)
    t0 = time.perf_counter()
    assert eng.fern_add_from_store(idx, store, 0, n_keys) == 0
    add_ms = (time.perf_counter() - t0) * 1e3
    I4 = [np.eye(4, dtype=np.float32)]
    queries, landed, first_ok = [], 0, 0
    for j in range(1, n_keys - 1, 2):
        for off in query_offsets:
            i = key_frames[j] + off
            rgba, mm, M_true = wl.frame(i)
            eng.view_update(view, rgba, mm, timestamp=float(i))
            z = mm[mm > 0].astype(np.float64) * 1e-3
            centre = np.array([0.0, 0.0, float(np.median(z))])
            M_ref, r_ref = eng.track_camera_sdf(view, [scene], I4, M_true, wl.intr)    # the tracker's own answer

            def chain():
                matches = eng.fern_query(idx, view, 0, n_keys, 4)
                starts = [key_poses[int(m["id"])] for m in matches]
                est, res = eng.track_camera_sdf_starts(view, [scene], I4, starts, wl.intr)
                scores = eng.score_camera_poses(view, [scene], I4, list(est), wl.intr, 0)
                kept = eng.select_start_poses(scores, 1, 1)
                return matches, est, kept
            t0 = time.perf_counter()
            matches, est, kept = chain()
            chain_ms = (time.perf_counter() - t0) * 1e3
            row = {"frame": i, "true_keyframe": j + off / key_step, "matches": [[int(m["id"]), int(m["dissimilarity"])] for m in matches],
                   "chain_ms": round(chain_ms, 3), "tracker_from_truth_error_mrad_voxels": [round(x, 3) for x in pose_error(M_ref, M_true, centre, vs)]}
            row["first_match_within_one_keyframe"] = bool(len(matches) and abs(int(matches[0]["id"]) - row["true_keyframe"]) <= 1.0)
            first_ok += row["first_match_within_one_keyframe"]
            if len(kept):
                M = est[int(kept[0])]
                row["kept_start"] = int(matches[int(kept[0])]["id"])
                row["error_to_truth_mrad_voxels"] = [round(x, 3) for x in pose_error(M, M_true, centre, vs)]
                row["error_to_tracker_mrad_voxels"] = [round(x, 3) for x in pose_error(M, M_ref, centre, vs)]
                row["relocalised"] = bool(row["error_to_tracker_mrad_voxels"][0] <= 5.0 and row["error_to_tracker_mrad_voxels"][1] <= 1.0)
            else:
                row["relocalised"] = False
            landed += row["relocalised"]
            queries.append(row)
    query_time = spread(lambda: eng.fern_query(idx, view, 0, n_keys, 4), reps)
    return {"workload": wl.name, "image": f"{wl.W}x{wl.H}", "keyframes": n_keys, "keyframe_step": key_step, "query_offsets": list(query_offsets),
            "fern_params": params.as_dict(), "add_from_store_ms": round(add_ms, 3), "fern_query": query_time,
            "queries": len(queries), "first_match_within_one_keyframe": int(first_ok), "relocalised": int(landed), "rows": queries}


def bench_score_256(pkg, eng, wl, reps):
    """dslam_score_camera_poses over 256 poses on a street map of four keyframes."""
    scene, _, key_poses, view, vs = build_map(pkg, eng, wl, [0, 1, 2, 3])
    rng = np.random.RandomState(5)
    poses = []
    for _ in range(256):
        M = key_poses[3].astype(np.float64).copy()
        M[:3, 3] += rng.uniform(-1.5, 1.5, 3) * vs
        poses.append(M.astype(np.float32))
    I4 = [np.eye(4, dtype=np.float32)]
    return {f"level_{lv}": spread(lambda: eng.score_camera_poses(view, [scene], I4, poses, wl.intr, lv), max(3, reps // 10)) for lv in (2, 0)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "fern_bench.json")
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    room, street = synth.s_room(640, 480), synth.s_street(640, 480)
    out = {"reps": reps, "unit": "wall clock per call on a synchronous, otherwise idle engine; median and 10th / 90th percentile",
           "hbm_peak_bytes_per_second": HBM_PEAK}
    out["encode"] = bench_encode(pkg, eng, room, reps)
    out["scan"] = bench_scan(pkg, eng, max(10, reps // 2))
    out["score_camera_poses_256"] = bench_score_256(pkg, eng, street, reps)
    out["chain"] = [bench_chain(pkg, eng, room, 6, 12, (2, 3), pkg.FernParams(depth_max_mm=5000, seed=12345), reps),
                    bench_chain(pkg, eng, room, 6, 12, (2, 3), pkg.FernParams(channels=2, depth_max_mm=5000, seed=12345), reps),
                    bench_chain(pkg, eng, street, 2, 12, (1,), pkg.FernParams(depth_min_mm=500, depth_max_mm=30000, seed=12345), reps)]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fo:
        fo.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
