"""Cost of the composite raycast over local maps (dslam_get_image_multi) on the S-street drive.

The drive is split into local maps the way the reference does it (DenseSlam.cpp:133-141, 260-261): a new map every K
keyframes, anchored at that keyframe's pose (estimatedGlobalPose = the keyframe's world -> camera matrix), every keyframe
fused into the newest map at its pose relative to that map.  For N = 1, 2, 4, 8 maps, from the first keyframe's pose
(the drive lies ahead of it, so every map is in view), 640x480:
  * composite DEPTH and SHADED image of the first N maps;
  * N separate dslam_get_image calls, one per map (each from the camera M T_i^-1);
  * one dslam_get_image on a single map fused from the same keyframes;
  * launches per composite call (2N + 1) and the mean number of maps per 8x8 tile that any map reaches.
Wall clock per call around an asynchronous engine (synchronised around the batch); every call alternates between two
poses, so dslam_get_image's memo never turns a call into a shade-only pass.  Prints one JSON line; with an argument
`out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/multimap_bench.py [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

K = 4          # keyframes per local map
N_MAX = 8


def timed(eng, fn, reps):
    fn(0)
    fn(1)
    eng.synchronize()
    t0 = time.perf_counter()
    for r in range(reps):
        fn(r & 1)
    eng.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def tile_mask_bits(eng, scenes, Ts, M, intr, W, H, vs):
    """Per 8x8 tile the number of maps one of whose blocks projects into it (ProjectSingleBlock's bbox, host numpy):
    mean over the tiles at least one map reaches."""
    cw, ch = (W + 7) // 8, (H + 7) // 8
    count = np.zeros((ch, cw), np.int64)
    for s, T in zip(scenes, Ts):
        h = eng.download_hash_table(s)
        pos = h["pos"][h["ptr"] >= 0].astype(np.float64)
        Mi = np.asarray(M, np.float64) @ np.linalg.inv(np.asarray(T, np.float64))
        fx, fy, cx, cy = (float(v) for v in intr)
        us, vs_, zs = [], [], []
        for c in range(8):
            d = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.float64)
            p = (pos + d) * 8 * vs
            q = p @ Mi[:3, :3].T + Mi[:3, 3]
            zs.append(q[:, 2])
            with np.errstate(divide="ignore", invalid="ignore"):
                us.append((fx * q[:, 0] / q[:, 2] + cx) / 8)
                vs_.append((fy * q[:, 1] / q[:, 2] + cy) / 8)
        u, v, z = np.stack(us, 1), np.stack(vs_, 1), np.stack(zs, 1)
        good = z > 1e-6
        with np.errstate(invalid="ignore"):
            x0 = np.maximum(np.where(good, np.floor(u), np.inf).min(1), 0)
            y0 = np.maximum(np.where(good, np.floor(v), np.inf).min(1), 0)
            x1 = np.minimum(np.where(good, np.ceil(u), -np.inf).max(1), cw - 1)
            y1 = np.minimum(np.where(good, np.ceil(v), -np.inf).max(1), ch - 1)
        hit = np.zeros((ch, cw), bool)
        for a, b, c_, d_ in zip(x0, y0, x1, y1):
            if np.isfinite(a) and np.isfinite(c_) and a <= c_ and b <= d_:
                hit[int(b):int(d_) + 1, int(a):int(c_) + 1] = True
        count += hit
    reached = count > 0
    return float(count[reached].mean()) if reached.any() else 0.0, int(reached.sum()), cw * ch


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    n_kf = K * N_MAX
    frames = [wl.frame(i) for i in range(n_kf)]
    view = eng.create_view(W, H)

    # local maps: map j holds keyframes j K .. j K + K - 1, anchored at keyframe j K
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
        maps.append((s, rs))
        Ts.append(T)
    eng.synchronize()

    M0 = np.asarray(frames[0][2], np.float32)
    M1 = (synth.pose_matrix(synth.look_rotation(0.002, 0.0), [0.01, 0.0, 0.0]) @ M0.astype(np.float64)).astype(np.float32)
    poses = (M0, M1)
    eng.set_async(True)
    rows = []
    for n in (1, 2, 4, 8):
        scenes = [m[0] for m in maps[:n]]
        Tn = Ts[:n]
        rs_multi = eng.create_render_state(scenes[0], W, H)
        row = {"maps": n, "keyframes": n * K, "launches_per_composite": 2 * n + 1}
        for name, t in (("depth", pkg.IMAGE_DEPTH), ("shaded", pkg.IMAGE_SHADED)):
            row[f"composite_{name}_ms"] = timed(
                eng, lambda k: eng.get_image_multi(scenes, Tn, rs_multi, poses[k], intr, t, download=False), reps)
        cams = [[(np.asarray(poses[k], np.float64) @ np.linalg.inv(T.astype(np.float64))).astype(np.float32) for T in Tn]
                for k in (0, 1)]

        def separate(k):
            for (s, rs), Mi in zip(maps[:n], cams[k]):
                eng.get_image(s, rs, Mi, intr, pkg.IMAGE_DEPTH, download=False)
        row["separate_get_image_depth_ms"] = timed(eng, separate, reps)
        # one map fused from the same keyframes (world frame)
        eng.set_async(False)
        s1 = eng.create_scene(p)
        rs1 = eng.create_render_state(s1, W, H)
        for i in range(n * K):
            rgba, mm, M = frames[i]
            eng.view_update(view, rgba, mm, timestamp=float(i))
            eng.process_frame(s1, view, rs1, M, intr)
        eng.set_async(True)
        row["single_map_get_image_depth_ms"] = timed(
            eng, lambda k: eng.get_image(s1, rs1, poses[k], intr, pkg.IMAGE_DEPTH, download=False), reps)
        row["single_map_get_image_shaded_ms"] = timed(
            eng, lambda k: eng.get_image(s1, rs1, poses[k], intr, pkg.IMAGE_SHADED, download=False), reps)
        row["composite_over_single_depth"] = row["composite_depth_ms"] / row["single_map_get_image_depth_ms"]
        eng.set_async(False)
        bits, reached, tiles = tile_mask_bits(eng, scenes, Tn, M0, intr, W, H, p.voxel_size)
        eng.set_async(True)
        row["mean_maps_per_reached_tile"] = bits
        row["tiles_reached"] = reached
        row["tiles"] = tiles
        rows.append(row)
        del s1, rs1
    eng.set_async(False)
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call (wall clock, asynchronous engine synchronised around the batch, output left on the device)",
           "target": "composite of 4 maps <= 1.5 x the single-map dslam_get_image time", "rows": rows}
    r4 = [r for r in rows if r["maps"] == 4][0]
    out["target_met"] = bool(r4["composite_depth_ms"] <= 1.5 * r4["single_map_get_image_depth_ms"])
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
