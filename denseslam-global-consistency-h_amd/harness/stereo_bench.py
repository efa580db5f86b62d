"""Cost and quality of the semi-global stereo matcher (dslam_stereo_depth_device).

Cost, at 640 x 480 and 1226 x 370, each with D = 64 and D = 128, on device-resident random images (the work of every kernel
but the left-right check is independent of the image content):
  * wall clock per call of dslam_stereo_depth_device, an asynchronous engine synchronised around `reps` calls after a
    warm-up call;
  * device time of the handle's launches between events (dslam_debug_stereo_phases): census, aggregation (with the memset
    of S), selection (with the memset of the right keys), the left-right check with the conversion; median over `reps`;
  * the bytes each pass moves by the design's own count, and that as a fraction of the HBM peak at the measured time.
    n = W H.  census: 2 n bytes in, 16 n out.  aggregation: 2 n D for the memset, 8 directions x 2 n D of atomic adds into S
    (the adds travel as pairs of disparities, 4 bytes per pair), 8 x 16 n of census codes read once per direction (the D-fold
    re-reads of the right codes along a line are cache hits by design).  selection: 2 n D of S read, 4 n memset and 4 n
    written for the right keys, 4 n of candidates.  left-right check: 8 n in, 4 n out.
Quality, on one rendered stereo pair of S-street (320 x 96, baseline 0.54 m, the right camera displaced along the camera's
+x, colour_k = (6, 9, 4): the default texture is too smooth for a census), D = 128 with the defaults:
  * the share of pixels with a valid disparity (of all pixels, and of those whose true disparity fx b / z lies in 1 .. D - 2);
  * of those, the share within 0.5 px of fx b / z;
  * the same two shares after fusing the resulting depth into an empty map and ray-casting it back from the same pose;
  * whether the device's disparity equals tests/ref_stereo.py's on that pair (it must: the law is exact).
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/stereo_bench.py [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

HBM_PEAK = 8.0e12     # bytes per second: the peak DESIGN.md section 4 measures against
BASELINE = 0.54
FRAME = 10


def moved_bytes(W, H, D):
    n = W * H
    return {"census": 2 * n + 16 * n, "aggregation": 2 * n * D + 8 * 2 * n * D + 8 * 16 * n, "selection": 2 * n * D + 12 * n,
            "lr_check": 12 * n}


def cost_rows(pkg, eng, reps):
    import torch
    rows = []
    for W, H in ((640, 480), (1226, 370)):
        g = torch.Generator(device="cpu").manual_seed(W)
        left = torch.randint(0, 256, (H, W), dtype=torch.uint8, generator=g).to("cuda:0")
        right = torch.randint(0, 256, (H, W), dtype=torch.uint8, generator=g).to("cuda:0")
        depth = torch.zeros(H * W, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        for D in (64, 128):
            st = eng.create_stereo(W, H, pkg.StereoParams(max_disparity=D))
            calib = (480.0, BASELINE, 1.0, 0.5, 30.0)

            def call():
                eng.stereo_depth_device(st, left.data_ptr(), right.data_ptr(), calib, depth.data_ptr())

            eng.set_async(True)
            call()
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            eng.synchronize()
            whole = (time.perf_counter() - t0) / reps
            eng.stereo_phases(st, enable=1, read=False)
            phases = []
            for _ in range(reps):
                call()
                phases.append(eng.stereo_phases(st)[:4])
            eng.stereo_phases(st, enable=0, read=False)
            eng.set_async(False)
            ms = np.median(np.array(phases), axis=0)
            row = {"width": W, "height": H, "max_disparity": D, "lines": 2 * H + 2 * W + 4 * (W + H - 1), "whole_call_ms": whole * 1e3,
                   "phases_sum_ms": float(ms.sum()), "valid_share": float((depth.cpu().numpy() > 0).mean())}
            for (name, nbytes), t in zip(moved_bytes(W, H, D).items(), ms):
                row[name + "_ms"] = float(t)
                row[name + "_bytes"] = int(nbytes)
                row[name + "_fraction_of_hbm_peak"] = round(nbytes / (float(t) * 1e-3) / HBM_PEAK, 4) if t > 0 else None
            rows.append(row)
            st.close()
    return rows


def quality(pkg, eng, synth):
    import ref_stereo as rs
    W, H, D = 320, 96, 128
    wl = synth.s_street(W, H)
    intr = wl.intr.astype(np.float64)
    T_left = wl.pose(FRAME)
    T_right = T_left.copy()
    T_right[:3, 3] += T_left[:3, 0] * BASELINE
    cz = T_left[2, 3]
    prims = [p for p in wl.prims if p.hi[2] >= cz - wl.cull_z[0] and p.lo[2] <= cz + wl.cull_z[1]]
    z, left = synth.render(prims, intr, W, H, T_left, colour_k=(6, 9, 4))
    _, right = synth.render(prims, intr, W, H, T_right, colour_k=(6, 9, 4))
    fb = float(intr[0]) * BASELINE
    with np.errstate(divide="ignore"):
        truth = np.where(np.isfinite(z), fb / z, 0.0)
    in_range = (truth >= 1.0) & (truth <= D - 2)

    def shares(disp_px, valid):
        good = valid & (np.abs(disp_px - truth) <= 0.5)
        return {"valid": float(valid.mean()), "valid_in_range": float(valid[in_range].mean()),
                "within_half_px_of_valid": float(good.sum() / max(valid.sum(), 1)),
                "within_half_px_of_valid_in_range": float(good[in_range].sum() / max(valid[in_range].sum(), 1))}

    st = eng.create_stereo(W, H, pkg.StereoParams(max_disparity=D, channels=4))
    max_depth = float(wl.scene_kwargs["frustum_max"]) * 0.8
    calib = (float(wl.intr[0]), BASELINE, 1.0, float(wl.scene_kwargs["frustum_min"]), min(max_depth, 32.0))
    depth, disp = eng.stereo_depth(st, left, right, calib)
    ref = rs.match(left, right, rs.resolve(dict(max_disparity=D, channels=4)))
    out = {"pair": f"S-street frame {FRAME}, {W} x {H}, baseline {BASELINE} m, colour_k (6, 9, 4), D = {D}, defaults",
           "true_disparity_in_range_share": float(in_range.mean()),
           "device_equals_reference": bool(np.array_equal(disp, ref["disp"]) and np.array_equal(depth, rs.depth_mm(ref["disp"], *calib))),
           "matched": shares(disp.astype(np.float64) / 16.0, disp != pkg.STEREO_INVALID)}
    # fuse the depth into an empty map and cast it back from the same pose
    scene = eng.create_scene(pkg.SceneParams(**wl.scene_kwargs))
    rstate = eng.create_render_state(scene, W, H)
    view = eng.create_view(W, H)
    M = synth.world_to_camera(T_left)
    eng.view_update(view, left, depth)
    eng.process_frame(scene, view, rstate, M, wl.intr)
    cast = eng.get_depth_image_int16(scene, rstate, M, wl.intr, 1000).astype(np.float64)
    with np.errstate(divide="ignore"):
        cast_disp = np.where(cast > 0, fb / (cast / 1000.0), 0.0)
    out["depth_pixels"] = float((depth > 0).mean())
    out["fused_and_cast_back"] = shares(cast_disp, cast > 0)
    for h in (view, rstate, scene, st):
        h.close()
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    out = {"reps": reps, "hbm_peak_bytes_per_second": HBM_PEAK,
           "unit": "whole_call_ms: wall clock per call of dslam_stereo_depth_device, asynchronous engine synchronised around the "
                   "batch, one warm-up call; phases: device time between events, median over the calls; one run, random images",
           "rows": cost_rows(pkg, eng, reps), "quality": quality(pkg, eng, synth)}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
