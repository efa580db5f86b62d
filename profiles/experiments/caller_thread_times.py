#!/usr/bin/env python3
"""Where the caller's thread spends a frame of bench.py's pipelined loop: wall time of each ABI call
(fence_wait, view_update, process_frame, get_image, fence_record), medians over the steady state, and the loop's period.
usage: caller_thread_times.py [frames, default 140] [frames to skip at the front, default 30]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402
import bench  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 140
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    W, H = 640, 480
    wl = synth.s_street(W, H)
    rgba_h, depth_h, Ms = bench.generate_frames("s_street", W, H, n, 16)
    eng = pkg.open_engine(0)
    nlb = 0x40000
    while nlb < 9000 + 600 * n:
        nlb *= 2
    scene = eng.create_scene(pkg.SceneParams(num_local_blocks=nlb, **wl.scene_kwargs))
    view = eng.create_view(W, H)
    rs, rs_free = eng.create_render_state(scene, W, H), eng.create_render_state(scene, W, H)
    cs, ds = W * H * 4, W * H * 2
    rec = eng.host_alloc((n, cs + ds), np.uint8)
    rgba_p = rec[:, :cs].reshape(n, H, W, 4)
    depth_p = rec[:, cs:].view(np.int16).reshape(n, H, W)
    rgba_p[...] = rgba_h
    depth_p[...] = depth_h
    ring = bench.OUT_RING
    image_p = eng.host_alloc((ring, H, W), np.float32)
    fences = [eng.fence_create() for _ in range(ring)]
    eng.set_async(True)
    names = ("fence_wait", "view_update", "process_frame", "get_image", "fence_record")
    t = np.zeros((n, len(names) + 1))
    now = time.perf_counter
    for i in range(n):
        slot = i % ring
        a = now(); eng.fence_wait(fences[slot])
        b = now(); eng.view_update(view, rgba_p[i], depth_p[i], timestamp=float(i))
        c = now(); eng.process_frame(scene, view, rs, Ms[i], wl.intr)
        d = now(); eng.get_image(scene, rs_free, Ms[i], wl.intr, pkg.IMAGE_DEPTH, out=image_p[slot])
        e = now(); eng.fence_record(fences[slot])
        f = now()
        t[i] = (b - a, c - b, d - c, e - d, f - e, a)
    eng.synchronize()
    eng.set_async(False)
    us = t[skip:, :len(names)] * 1e6
    period = np.diff(t[skip:, len(names)]) * 1e6
    out = {"frames": n - skip, "period_us_median": round(statistics.median(period), 1),
           "call_us_median": {k: round(float(np.median(us[:, j])), 1) for j, k in enumerate(names)},
           "calls_sum_us_median": round(float(np.median(us.sum(axis=1))), 1)}
    ov = getattr(eng, "debug_mark_overlap_counts", None)
    if ov:
        out["mark_overlap_counts"] = list(ov())
    sw = getattr(eng, "debug_sweep_overlap_counts", None)
    if sw:
        try:
            out["sweep_overlap_counts"] = list(sw())
        except Exception:
            pass
    print(json.dumps(out))


if __name__ == "__main__":
    main()
