"""Cost of fusing one local map into another (dslam_merge_maps) on two S-street local maps.

The drive is split into local maps as register_bench.py does it (a new map every K keyframes, anchored at that keyframe's
pose).  Map 1 is merged into map 0 under the transform dslam_register_maps returns from a start 0.5 voxel / 2 mrad off.
A merge changes its destination, so map 0 is reset and re-fused from its keyframes before every repetition (not timed).
Reported:
  * ms per call (wall clock; the call waits for the stream itself), and the same call with the phase hook on
    (dslam_debug_merge_phases: every phase closed by a wait for the stream) split into live list / mark kernels / ordered
    selections (ranks, serve, touched list) / block kernel / read-backs;
  * passes, blocks allocated and touched, voxels changed;
  * the bytes the block kernel moves in the destination (4 KiB read per touched block, 16 bytes written per changed pair
    of voxels, bounded below by 8 bytes per changed voxel) and the rate that makes against the 4 KiB-per-wave
    read-modify-write calibration of DESIGN.md section 4;
  * dslam_get_image on the merged map against dslam_get_image_multi on the two maps, depth, from the first keyframe's pose.
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/merge_bench.py [reps] [out.json]
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
PHASES = ("live_list", "mark_kernels", "selections", "block_kernel", "read_backs")


def small_motion(angle, axis, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    D[:3, 3] = t
    return D


def timed(fn, reps):
    fn()
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


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
    start = (small_motion(2e-3, (0.42, -0.61, 0.67), np.array([0.6, -0.64, 0.48]) * 0.5 * p.voxel_size) @ X_true).astype(np.float32)
    X, reg = eng.register_maps(src, dst, start)

    # the composite image of the two maps, before anything is merged
    M0 = np.asarray(frames[0][2], np.float32)
    rs_multi = eng.create_render_state(dst, W, H)
    both = eng.get_image_multi([dst, src], [Ts[0], (np.linalg.inv(X.astype(np.float64)) @ Ts[0].astype(np.float64)).astype(np.float32)],
                               rs_multi, M0, intr, pkg.IMAGE_DEPTH).copy()
    t_multi = timed(lambda: eng.get_image_multi([dst, src], [Ts[0], (np.linalg.inv(X.astype(np.float64)) @ Ts[0].astype(np.float64)).astype(np.float32)],
                                                rs_multi, M0, intr, pkg.IMAGE_DEPTH, download=False), 20)

    def fresh_destination():
        eng._call("scene_reset", eng._engine, dst.ptr)
        fuse(dst, 0)
        eng.synchronize()

    calls, phases, res = [], np.zeros(5), None
    for rep in range(reps + 1):                 # (the first repetition allocates the merge's scratch: not counted)
        fresh_destination()
        t0 = time.perf_counter()
        res = eng.merge_maps(src, dst, X)
        if rep:
            calls.append((time.perf_counter() - t0) * 1e3)
    eng.debug_merge_phases(True)
    hooked = []
    for rep in range(reps):
        fresh_destination()
        t0 = time.perf_counter()
        eng.merge_maps(src, dst, X)
        hooked.append((time.perf_counter() - t0) * 1e3)
        phases += eng.debug_merge_phases(True)
    eng.debug_merge_phases(False)
    phases /= reps

    M_in_map = (M0.astype(np.float64) @ np.linalg.inv(Ts[0].astype(np.float64))).astype(np.float32)
    rs_one = eng.create_render_state(dst, W, H)
    merged = eng.get_image(dst, rs_one, M_in_map, intr, pkg.IMAGE_DEPTH).copy()
    # (another pose in between, so that the timed calls do not hit GetImage's memo)
    M_other = (small_motion(5e-3, (0.0, 1.0, 0.0), (0.01, 0.0, 0.0)) @ M_in_map.astype(np.float64)).astype(np.float32)
    t_one = timed(lambda: (eng.get_image(dst, rs_one, M_in_map, intr, pkg.IMAGE_DEPTH, download=False),
                           eng.get_image(dst, rs_one, M_other, intr, pkg.IMAGE_DEPTH, download=False)), 20) / 2
    in_both = (both > 0) & (merged > 0)

    r = res.as_dict()
    read_bytes = r["blocks_touched"] * 4096
    written_low, written_high = r["voxels_changed"] * 8, min(r["voxels_changed"] * 16, r["blocks_touched"] * 4096)
    block_s = phases[3] * 1e-3
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps,
           "unit": "ms, wall clock; measured on the part",
           "registration_stop_reason": reg.stop_reason, "registration_evaluations": reg.evaluations,
           "merge_call_ms": float(np.mean(calls)), "merge_call_ms_min": float(np.min(calls)),
           "merge_call_with_phase_hook_ms": float(np.mean(hooked)),
           "phase_ms": {name: float(v) for name, v in zip(PHASES, phases)},
           "waits_ms": "every pass ends with one read-back the host waits for (read_backs); with the hook on every phase "
                       "ends with a wait as well, so the phases add up to the hooked call",
           **r,
           "block_kernel_destination_bytes_read": read_bytes,
           "block_kernel_destination_bytes_written_between": [written_low, written_high],
           "block_kernel_TBps_between": [(read_bytes + written_low) / block_s / 1e12, (read_bytes + written_high) / block_s / 1e12],
           "rmw_calibration_TBps": 5.4,
           "get_image_merged_map_ms": t_one, "get_image_multi_two_maps_ms": t_multi,
           "pixels_in_both_share": float(in_both.mean()),
           "median_abs_depth_difference_voxels": float(np.median(np.abs(both[in_both] - merged[in_both])) / p.voxel_size) if in_both.any() else None}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
