"""Cost of the point and ray queries (dslam_query_points, dslam_cast_rays) on the S-street drive.

The drive is split into local maps as multimap_bench.py splits it (a new map every K keyframes, anchored at that keyframe's
pose).  For N = 1, 2, 4, 8 listed maps, from the first keyframe's camera at 640x480:
  * rays per second of dslam_cast_rays_device for the camera's 307 200 pixel rays (t 0.2 m .. the frustum's far plane), in
    pixel order and shuffled, with all shading and with none -- next to dslam_get_image_multi (SHADED and DEPTH) of the
    same camera and maps, which culls maps per 8x8 tile and starts each ray at its range cell;
  * points per second of dslam_query_points_device at one point per pixel ray (the 8-map cast's hit point; 5 m along the
    ray where it missed), in pixel order -- neighbouring lanes read neighbouring cells -- and shuffled, with `what` = sdf
    only and with all fields.
Every listed map is visited for every element, so the cost per listed map (the slope from 1 to 8 maps, per element) is
what a per-wavefront culling of maps would have to beat.  Wall clock around an asynchronous engine, synchronised around the
batch, inputs and outputs on the device.  Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/query_bench.py [reps] [out.json]
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
    fn()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    import torch
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

    # the pixel rays of the first keyframe's camera
    M0 = np.asarray(frames[0][2], np.float32)
    Minv = np.linalg.inv(M0.astype(np.float64))
    fx, fy, cx, cy = (float(v) for v in intr)
    ys, xs = np.mgrid[0:H, 0:W]
    d_cam = np.stack([(xs.reshape(-1) - cx) / fx, (ys.reshape(-1) - cy) / fy, np.ones(W * H)], axis=1)
    n = W * H
    far = float(p.frustum_max)
    rays = np.concatenate([np.broadcast_to(Minv[:3, 3], (n, 3)), d_cam @ Minv[:3, :3].T, np.full((n, 1), 0.2), np.full((n, 1), far)],
                          axis=1).astype(np.float32)
    first = eng.cast_rays(maps, Ts, rays)
    unit = rays[:, 3:6] / np.linalg.norm(rays[:, 3:6], axis=1, keepdims=True)
    hit = first["status"] > 0
    points = np.where(hit[:, None], first["point"], rays[:, 0:3] + 5.0 * unit).astype(np.float32)
    perm = np.random.default_rng(0).permutation(n)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    d_rays = {"pixel_order": dev(rays), "shuffled": dev(rays[perm])}
    d_points = {"pixel_order": dev(points), "shuffled": dev(points[perm])}
    d_out = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng.set_async(True)
    rows = []
    for m in (1, 2, 4, 8):
        scenes, Tn = maps[:m], Ts[:m]
        rs_multi = eng.create_render_state(scenes[0], W, H)
        row = {"maps": m}
        for order in ("pixel_order", "shuffled"):
            for name, what in (("all", pkg.QUERY_ALL), ("unshaded", pkg.QUERY_SDF)):
                t = timed(eng, lambda: eng.cast_rays_device(scenes, Tn, d_rays[order].data_ptr(), n, d_out.data_ptr(), 0.0, what), reps)
                row[f"rays_{order}_{name}_ms"] = t * 1e3
                row[f"rays_{order}_{name}_per_s"] = n / t
            for name, what in (("sdf", pkg.QUERY_SDF), ("all", pkg.QUERY_ALL)):
                t = timed(eng, lambda: eng.query_points_device(scenes, Tn, d_points[order].data_ptr(), n, d_out.data_ptr(), what), reps)
                row[f"points_{order}_{name}_ms"] = t * 1e3
                row[f"points_{order}_{name}_per_s"] = n / t
        for name, t in (("depth", pkg.IMAGE_DEPTH), ("shaded", pkg.IMAGE_SHADED)):
            row[f"get_image_multi_{name}_ms"] = timed(eng, lambda: eng.get_image_multi(scenes, Tn, rs_multi, M0, intr, t, download=False), reps) * 1e3
        rows.append(row)
    eng.set_async(False)
    r1, r8 = rows[0], rows[-1]
    per_map = {k[:-3] + "_ns_per_element_per_listed_map": (r8[k] - r1[k]) * 1e6 / (7 * n) for k in r1 if k.endswith("_ms") and not k.startswith("get_image")}
    out = {"workload": "S-street", "image": f"{W}x{H}", "elements": n, "keyframes_per_map": K, "reps": reps,
           "rays_hit_with_8_maps": int(hit.sum()), "t_min_m": 0.2, "t_max_m": far,
           "unit": "wall clock per call, asynchronous engine synchronised around the batch, inputs and outputs on the device",
           "rows": rows, "cost_per_listed_map": per_map}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
