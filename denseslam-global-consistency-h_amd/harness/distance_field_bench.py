"""Cost of the occupancy and distance grids (dslam_distance_field_device) on the S-street drive.

The drive is split into local maps as query_bench.py splits it (a new map every K keyframes, anchored at that keyframe's
pose).  The grid is dslam_grid_from_box over the world box of all maps' resident blocks, at cell 2 and cell 4 (a box whose
grid would exceed the limits is cut back about its centre, and the row says so).  Per cell size:
  * wall clock per call of dslam_distance_field_device (states and squared distances, inputs and outputs on the device),
    an asynchronous engine synchronised around `reps` calls -- the call waits once for the live counts of the maps;
  * device time of the phases of one call between events (dslam_debug_distance_field_phases): the packed states (memset
    and k_df_mark), the x pass, the y pass, the last pass; the median over `reps` calls;
  * the bytes each phase has to move and what share of the HBM peak that makes at the measured time.  k_df_mark: 4 KiB
    per resident block (the low words lie 8 bytes apart, so every line of a block is fetched) + the packed states; x pass:
    the packed states in, 4 bytes per cell out; y pass: 4 bytes per cell in and out; last pass: 4 bytes per cell in, 4 + 1
    bytes per cell out (distances and state bytes).
Prints one JSON line; with an argument `out.json` also writes it there.

    python denseslam-global-consistency-h_amd/harness/distance_field_bench.py [reps] [out.json]
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
N_MAPS = 8
HBM_PEAK = 8.0e12     # bytes per second: the peak DESIGN.md section 4 measures against


def world_box(eng, maps, Ts, vs):
    """(lo, hi) in metres of the resident blocks of all maps, taken to the world frame; and the resident blocks in all."""
    lo, hi, blocks = np.full(3, np.inf), np.full(3, -np.inf), 0
    corners = np.array([[x, y, z] for x in (0, 8) for y in (0, 8) for z in (0, 8)], np.float64)
    for s, T in zip(maps, Ts):
        table = eng.download_hash_table(s)
        pos = table["pos"][table["ptr"] >= 0].astype(np.float64)
        blocks += len(pos)
        if not len(pos):
            continue
        p = ((pos[:, None, :] * 8 + corners[None]) * vs).reshape(-1, 3)
        Tinv = np.linalg.inv(np.asarray(T, np.float64))
        w = p @ Tinv[:3, :3].T + Tinv[:3, 3]
        lo, hi = np.minimum(lo, w.min(axis=0)), np.maximum(hi, w.max(axis=0))
    return lo, hi, blocks


def fit_box(pkg, lo, hi, vs, cell):
    """The box cut back about its centre until its grid is within the limits."""
    lo, hi = lo.copy(), hi.copy()
    cut = False
    edge = cell * vs
    for a in range(3):
        if (hi[a] - lo[a]) / edge > pkg.GRID_MAX_DIM - 2:
            c = 0.5 * (lo[a] + hi[a])
            lo[a], hi[a] = c - 0.5 * (pkg.GRID_MAX_DIM - 2) * edge, c + 0.5 * (pkg.GRID_MAX_DIM - 2) * edge
            cut = True
    while np.prod(np.ceil((hi - lo) / edge) + 2) > pkg.GRID_MAX_CELLS:
        a = int(np.argmax(hi - lo))
        c = 0.5 * (lo[a] + hi[a])
        lo[a], hi[a] = c - 0.45 * (hi[a] - lo[a]), c + 0.45 * (hi[a] - lo[a])
        cut = True
    return lo, hi, cut


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
    frames = [wl.frame(i) for i in range(K * N_MAPS)]
    view = eng.create_view(W, H)
    maps, Ts = [], []
    for j in range(N_MAPS):
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
    vs = float(np.float32(p.voxel_size))
    lo, hi, blocks = world_box(eng, maps, Ts, vs)

    rows = []
    for cell in (2, 4):
        blo, bhi, cut = fit_box(pkg, lo, hi, vs, cell)
        g = eng.grid_from_box(blo, bhi, vs, cell)
        cells = g.cells
        words = (g.dims[0] + 15) // 16 * g.dims[1] * g.dims[2]
        d_states = torch.zeros(cells, dtype=torch.uint8, device="cuda:0")
        d_dist = torch.zeros(cells, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def call():
            eng.distance_field_device(maps, Ts, g, d_states.data_ptr(), d_dist.data_ptr())

        call()
        eng.synchronize()
        states = d_states.cpu().numpy()
        dist = d_dist.cpu().numpy()
        eng.set_async(True)
        call()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        eng.synchronize()
        whole = (time.perf_counter() - t0) / reps
        eng.distance_field_phases(enable=1, read=False)
        phases = []
        for _ in range(reps):
            call()
            phases.append(eng.distance_field_phases())
        eng.distance_field_phases(enable=0, read=False)
        eng.set_async(False)
        ms = np.median(np.array(phases), axis=0)
        moved = {"states": blocks * 4096 + 2 * words * 4, "x_pass": words * 4 + cells * 4, "y_pass": 2 * cells * 4, "last_pass": cells * 9}
        row = {"cell": cell, "dims": [int(v) for v in g.dims], "origin": [int(v) for v in g.origin], "cells": cells, "box_cut": bool(cut),
               "occupied": int((states == 3).sum()), "free": int((states == 1).sum()), "unknown": int((states == 0).sum()),
               "largest_d2": int(dist[dist != pkg.DIST_FAR].max()) if (dist != pkg.DIST_FAR).any() else None,
               "whole_call_ms": whole * 1e3, "phases_sum_ms": float(ms.sum())}
        for (name, nbytes), t in zip(moved.items(), ms):
            row[name + "_ms"] = float(t)
            row[name + "_bytes"] = int(nbytes)
            row[name + "_fraction_of_hbm_peak"] = round(nbytes / (float(t) * 1e-3) / HBM_PEAK, 4) if t > 0 else None
        rows.append(row)
    out = {"workload": "S-street", "maps": N_MAPS, "keyframes_per_map": K, "resident_blocks": int(blocks), "reps": reps,
           "voxel_size": vs, "hbm_peak_bytes_per_second": HBM_PEAK,
           "unit": "whole_call_ms: wall clock per call, asynchronous engine synchronised around the batch; phases: device time "
                   "between events, median over the calls; one run",
           "rows": rows}
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(json.dumps(json.loads(line), indent=1) + "\n")


if __name__ == "__main__":
    main()
