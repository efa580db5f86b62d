"""Cost of undoing a map merge (dslam_unmerge_maps) and of correcting one (dslam_remerge_maps) on two S-street local maps,
with dslam_merge_maps on the same pair in the same run as the yardstick.

The pair is merge_bench.py's: the drive split into local maps of K keyframes, map 1 merged into map 0 under the transform
dslam_register_maps returns from a start 0.5 voxel / 2 mrad off (X_old here).  Every call changes its destination, so map 0
is reset and re-fused from its keyframes before every repetition, and for the unmerge and the remerge merged under X_old as
well (none of that is timed).  X_new is X_old moved by 0.5 voxel / 2 mrad.  Reported, as wall clock per call (every call
waits for the stream itself):
  * dslam_merge_maps(X_old);
  * dslam_unmerge_maps(X_old) on the merged map;
  * dslam_remerge_maps(X_old, X_new) on the merged map, and the two separate calls it stands for, timed together;
  * the result fields of each.
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/unmerge_bench.py [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402

from merge_bench import K, small_motion  # noqa: E402  (the same pair, the same offsets)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
    frames = [wl.frame(i) for i in range(2 * K)]
    view = eng.create_view(W, H)
    Ts = [np.asarray(frames[j * K][2], np.float32) for j in range(2)]

    def fuse(scene, j):
        rs = eng.create_render_state(scene, W, H)
        Tinv = np.linalg.inv(Ts[j].astype(np.float64))
        for i in range(j * K, j * K + K):
            rgba, mm, M = frames[i]
            eng.view_update(view, rgba, mm, timestamp=float(i))
            eng.process_frame(scene, view, rs, (np.asarray(M, np.float64) @ Tinv).astype(np.float32), intr)
        return rs

    maps = [eng.create_scene(p) for _ in range(2)]
    for j in range(2):
        fuse(maps[j], j)
    eng.synchronize()
    src, dst = maps[1], maps[0]
    X_true = Ts[0].astype(np.float64) @ np.linalg.inv(Ts[1].astype(np.float64))
    offset = small_motion(2e-3, (0.42, -0.61, 0.67), np.array([0.6, -0.64, 0.48]) * 0.5 * p.voxel_size)
    X_old, reg = eng.register_maps(src, dst, (offset @ X_true).astype(np.float32))
    X_new = (offset @ X_old.astype(np.float64)).astype(np.float32)

    def fresh_destination(merged):
        eng._call("scene_reset", eng._engine, dst.ptr)
        fuse(dst, 0)
        if merged:
            eng.merge_maps(src, dst, X_old)
        eng.synchronize()

    def measure(merged, call):
        times, res = [], None
        for rep in range(reps + 1):             # (the first repetition allocates scratch: not counted)
            fresh_destination(merged)
            t0 = time.perf_counter()
            res = call()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        return times, res

    t_merge, r_merge = measure(False, lambda: eng.merge_maps(src, dst, X_old))
    t_unmerge, r_unmerge = measure(True, lambda: eng.unmerge_maps(src, dst, X_old))
    t_remerge, r_remerge = measure(True, lambda: eng.remerge_maps(src, dst, X_old, X_new))
    t_two, r_two = measure(True, lambda: (eng.unmerge_maps(src, dst, X_old), eng.merge_maps(src, dst, X_new)))

    def ms(times):
        return {"mean": float(np.mean(times)), "min": float(np.min(times)), "max": float(np.max(times))}

    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms per call, wall clock; measured on the part",
           "registration_stop_reason": reg.stop_reason,
           "merge_call_ms": ms(t_merge), "unmerge_call_ms": ms(t_unmerge), "remerge_call_ms": ms(t_remerge),
           "unmerge_then_merge_calls_ms": ms(t_two),
           "unmerge_over_merge": float(np.mean(t_unmerge) / np.mean(t_merge)),
           "remerge_over_two_calls": float(np.mean(t_remerge) / np.mean(t_two)),
           "merge": r_merge.as_dict(), "unmerge": r_unmerge.as_dict(),
           "remerge": {"unmerged": r_remerge[0].as_dict(), "merged": r_remerge[1].as_dict()},
           "two_calls": {"unmerged": r_two[0].as_dict(), "merged": r_two[1].as_dict()}}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
