"""Cost of the sparse scene-flow matcher (dslam_sflow_push_device, dslam_sflow_match_device).

Cost, at 640 x 480 and 1226 x 370, each with half_resolution on and off, on device-resident frames cut from one seeded
texture of 5-pixel cells (disparity 8, motion (4, 2)), so that features and matches exist in realistic numbers:
  * wall clock per dslam_sflow_push_device (a stereo frame: both images) and per quad dslam_sflow_match_device of the sparse
    and of the dense set, an asynchronous engine synchronised around `reps` calls after a warm-up call;
  * device time of the handle's launches between events (dslam_debug_sflow_phases): filters, suppression, feature
    compaction (scan and record scatter), bin lists; matching, match compaction; median over `reps`;
  * the feature and match counts.
Counts, on one rendered pair of frames of S-street (320 x 96, baseline 0.54 m, colour_k = (6, 9, 4)), full resolution: the
features of every image and set and the quad matches of both sets, and whether they equal tests/ref_sflow.py's (they must).
For context only, the wall time of libviso2's own pushBack x 2 and matchFeatures as recorded in tests/golden/sflow_*.npz: a
CPU of another machine, and a different pass set (its matchFeatures runs both passes with refinement and outlier removal).
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/sflow_bench.py [reps] [out.json]
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

BASELINE = 0.54
PHASES = ("filters", "suppression", "feature_compaction", "bin_lists", "matching", "match_compaction")


def cost_rows(pkg, eng, reps):
    import torch
    import sflow_fixtures as sf
    rows = []
    for W, H in ((640, 480), (1226, 370)):
        f = sf.frames(W, H, 8, (4, 2), W)
        dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in f.items()}
        torch.cuda.synchronize()
        for half in (1, -1):
            h = eng.create_sflow(W, H, pkg.SflowParams(half_resolution=half))
            cap = 1 << 17
            out = torch.zeros(12 * cap, dtype=torch.int32, device="cuda:0")
            count = torch.zeros(4, dtype=torch.int32, device="cuda:0")

            def push(k):
                eng.sflow_push_device(h, dev["1" + k].data_ptr(), dev["2" + k].data_ptr())

            def timed(call):
                call()
                eng.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                eng.synchronize()
                return (time.perf_counter() - t0) / reps * 1e3

            eng.set_async(True)
            push("p")
            row = {"width": W, "height": H, "half_resolution": half == 1}
            row["push_ms"] = timed(lambda: push("c"))
            push("p"), push("c")                                # previous and current frame in place for the matches
            for which, name in ((0, "sparse"), (1, "dense")):
                row["quad_match_%s_ms" % name] = timed(lambda: eng.sflow_match_device(h, 2, which, out.data_ptr(), cap, count.data_ptr()))
                row["quad_matches_%s" % name] = int(count.cpu()[0])
            eng.sflow_phases(h, enable=1, read=False)
            phases = []
            for _ in range(reps):
                push("p"), push("c")
                eng.sflow_match_device(h, 2, 1, out.data_ptr(), cap, count.data_ptr())
                phases.append(eng.sflow_phases(h))
            eng.sflow_phases(h, enable=0, read=False)
            eng.set_async(False)
            for name, t in zip(PHASES, np.median(np.array(phases), axis=0)):
                row[name + "_ms"] = float(t)
            for image, name in ((pkg.SFLOW_IMAGE_1C, "1c"), (pkg.SFLOW_IMAGE_2C, "2c")):
                for which in (0, 1):
                    row["features_%s_set%d" % (name, which)] = eng.sflow_features(h, image, which, capacity=0)[1]
            rows.append(row)
            h.close()
    return rows


def street_counts(pkg, eng, synth):
    import ref_sflow as rf
    W, H = 320, 96
    wl = synth.s_street(W, H)
    intr = wl.intr.astype(np.float64)
    frames = []
    for k in (10, 11):
        T_left = wl.pose(k)
        T_right = T_left.copy()
        T_right[:3, 3] += T_left[:3, 0] * BASELINE
        cz = T_left[2, 3]
        prims = [p for p in wl.prims if p.hi[2] >= cz - wl.cull_z[0] and p.lo[2] <= cz + wl.cull_z[1]]
        frames.append(tuple(np.ascontiguousarray(synth.render(prims, intr, W, H, T, colour_k=(6, 9, 4))[1]) for T in (T_left, T_right)))
    enc = dict(half_resolution=-1, channels=4)
    h = eng.create_sflow(W, H, pkg.SflowParams(**enc))
    m = rf.Matcher(W, H, enc)
    for left, right in frames:
        eng.sflow_push(h, left, right)
        m.push(left, right)
    out = {"pair": f"S-street frames 10 and 11, {W} x {H}, baseline {BASELINE} m, colour_k (6, 9, 4), full resolution, defaults otherwise"}
    same = True
    for image, name in ((0, "1c"), (1, "2c"), (2, "1p"), (3, "2p")):
        for which in (0, 1):
            got, n = eng.sflow_features(h, image, which)
            out["features_%s_set%d" % (name, which)] = n
            same &= np.array_equal(got, m.features(image, which))
    for which in (0, 1):
        got, n = eng.sflow_match(h, 2, which)
        out["quad_matches_set%d" % which] = n
        same &= np.array_equal(got, m.match(2, which))
    out["device_equals_reference"] = bool(same)
    h.close()
    return out


def library_context():
    import sflow_fixtures as sf
    out = {}
    for name in sf.CASES:
        us = sf.golden(name)["cpu_us"]
        out[name] = {"pushBack_x2_us": int(us[0]), "matchFeatures_us": int(us[1])}
    return out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    pkg = ge.load_package()
    from dslam_amd.harness import synth
    eng = pkg.open_engine(0)
    out = {"reps": reps,
           "unit": "push_ms / quad_match_*_ms: wall clock per call, asynchronous engine synchronised around the batch, one warm-up "
                   "call; phases: device time between events, median over the calls; ONE run, textured frames",
           "rows": cost_rows(pkg, eng, reps), "street": street_counts(pkg, eng, synth),
           "libviso2_cpu_context": {"note": "wall time of the library's own calls on the fixture cases, on the CPU of the machine that "
                                            "wrote tests/golden: another machine, tiny images, and matchFeatures there runs both passes, "
                                            "refinement and outlier removal -- not comparable, context only",
                                    "cases": library_context()}}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
