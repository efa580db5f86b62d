"""Cost of the composite mesh over local maps (dslam_mesh_scene_multi) on the S-street drive.

The drive is split into local maps as in multimap_bench.py (a new map every K keyframes, anchored at that keyframe's pose,
every keyframe fused into the newest map at its pose relative to that map).  For N = 1, 2, 4, 8 maps:
  * one dslam_mesh_scene_multi call over the first N maps, without and with colours;
  * N separate dslam_mesh_scene calls, one per map (what the reference's export loop does), without and with colours;
  * the triangles of both (the composite drops what earlier maps cover) and the live blocks.
Wall clock per call on a synchronous engine, the mesh left on the device.  Prints one JSON line; with an argument
`out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/multimesh_bench.py [reps] [out.json] [commit]
"""
import ctypes as C
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


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    commit = sys.argv[3] if len(sys.argv) > 3 else "working tree"
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    wl = synth.s_street(640, 480)
    W, H, intr = wl.W, wl.H, wl.intr
    p = pkg.SceneParams(**wl.scene_kwargs)
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
    eng.synchronize()

    rows = []
    for n in (1, 2, 4, 8):
        scenes = maps[:n]
        ptrs = (C.c_void_p * n)(*[s.ptr for s in scenes])
        t_abi = np.ascontiguousarray(np.transpose(np.asarray(Ts[:n], np.float32), (0, 2, 1))).reshape(-1)
        t_ptr = t_abi.ctypes.data_as(C.POINTER(C.c_float))
        total = C.c_int(0)
        counts = np.zeros(n, np.int32)
        c_ptr = counts.ctypes.data_as(C.POINTER(C.c_int32))
        row = {"maps": n, "keyframes": n * K, "host_waits_per_composite": n}
        singles = []
        for colour in (0, 1):
            tag = "colour" if colour else "plain"

            def composite():
                eng._call("mesh_scene_multi", eng._engine, ptrs, t_ptr, C.c_int(n), C.c_int(0), C.c_int(colour),
                          C.byref(total), c_ptr)

            def separate():
                singles.clear()
                for s in scenes:
                    k = C.c_int(0)
                    eng._call("mesh_scene", eng._engine, s.ptr, C.c_int(0), C.c_int(colour), C.byref(k))
                    singles.append(k.value)

            row[f"composite_{tag}_ms"] = timed(composite, reps)
            row[f"separate_{tag}_ms"] = timed(separate, reps)
            row[f"ratio_{tag}"] = row[f"composite_{tag}_ms"] / row[f"separate_{tag}_ms"]
        row["composite_triangles"] = int(total.value)
        row["composite_triangles_per_map"] = [int(c) for c in counts]
        row["separate_triangles"] = int(sum(singles))
        row["live_blocks"] = int(sum((eng.download_hash_table(s)["ptr"] >= 0).sum() for s in scenes))
        rows.append(row)
    out = {"workload": "S-street", "image": f"{W}x{H}", "keyframes_per_map": K, "reps": reps, "measured_on": commit,
           "unit": "ms per call (wall clock, synchronous engine, the mesh left on the device)",
           "target": "none: first measurement of this call", "rows": rows}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
