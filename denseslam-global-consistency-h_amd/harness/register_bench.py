"""Cost of the map-to-map registration (dslam_register_maps) on two S-street local maps.

The drive is split into local maps as multimap_bench.py does it (a new map every K keyframes, anchored at that keyframe's
pose, every keyframe fused into the newest map at its pose relative to that map).  Source: map 1, destination: map 0; the
true transform between them is T_0 T_1^-1.  Reported:
  * one call that evaluates once (max_evaluations = 1: the ordered compaction of the source's entries + one k_register
    launch + the host's sum of the partial rows);
  * one call with default parameters from a start 0.5 voxel / 2 mrad off, its evaluations, and the time per further
    evaluation (the difference of the two calls over the further evaluations);
  * the bytes the source walk reads per evaluation (the live blocks' voxels, their table entries and the live list);
  * dslam_mesh_scene on the same source map: the existing pass that also visits every live block.
Wall clock per call (the call waits for the stream itself).  Prints one JSON line; with an argument `out.json` also
writes it there.

    python denseslam-global-consistency-h_amd/harness/register_bench.py [reps] [out.json]
"""
import ctypes as C
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


def timed(fn, reps):
    fn()
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def small_motion(angle, axis, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    D[:3, 3] = t
    return D


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    frames = [wl.frame(i) for i in range(2 * K)]
    view = eng.create_view(W, H)
    maps, Ts = [], []
    for j in range(2):
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
    src, dst = maps[1], maps[0]
    X_true = Ts[0].astype(np.float64) @ np.linalg.inv(Ts[1].astype(np.float64))
    start = (small_motion(2e-3, (0.42, -0.61, 0.67), np.array([0.6, -0.64, 0.48]) * 0.5 * p.voxel_size) @ X_true).astype(np.float32)
    live = int((eng.download_hash_table(src)["ptr"] >= 0).sum())

    one = pkg.RegisterParams(max_evaluations=1)
    _, r1 = eng.register_maps(src, dst, start, one)
    X, rd = eng.register_maps(src, dst, start)
    t_one = timed(lambda: eng.register_maps(src, dst, start, one), reps)
    t_call = timed(lambda: eng.register_maps(src, dst, start), reps)
    n_tri = C.c_int(0)
    # (the mesh stays on the device: the pass itself, without the download)
    t_mesh = timed(lambda: eng._call("mesh_scene", eng._engine, src.ptr, C.c_int(0), C.c_int(0), C.byref(n_tri)), reps)
    err = X.astype(np.float64) @ np.linalg.inv(X_true)
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call (wall clock; the call waits for the stream)",
           "source_live_blocks": live, "candidates": r1.candidates, "valid_at_start": r1.valid_last,
           "source_walk_bytes_per_evaluation": live * (512 * 8 + 16 + 4),
           "call_one_evaluation_ms": t_one,
           "call_default_ms": t_call, "call_default_evaluations": rd.evaluations, "call_default_stop_reason": rd.stop_reason,
           "further_evaluation_ms": (t_call - t_one) / max(rd.evaluations - 1, 1),
           "source_walk_GBps_in_one_evaluation_call": live * (512 * 8 + 16 + 4) / (t_one * 1e-3) / 1e9,
           "mesh_scene_same_source_ms": t_mesh, "mesh_scene_triangles": n_tri.value,
           "conditioning": rd.conditioning,
           "end_translation_error_voxels": float(np.linalg.norm(err[:3, 3]) / p.voxel_size),
           "end_rotation_error_mrad": float(1e3 * math.acos(min(1.0, (np.trace(err[:3, :3]) - 1) / 2)))}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
