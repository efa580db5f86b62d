"""The relocalisation case of track_starts_fixtures.py on the float64 reference alone (ref64_track_sdf.py): the GPU test of
test_gpu_track_starts.py runs a lattice, a scoring, a selection and the tracked starts from a pose the single call cannot
recover; here the reference shows that the case lies inside what the law can do, and the binding exists."""
import numpy as np

import ref64_track_sdf as rt
import track_sdf_fixtures as fx
import track_starts_fixtures as ts


def test_the_displacement_is_the_smallest_the_single_call_does_not_recover():
    f = ts.fixture()
    mu_voxels = f.maps[0].mu / f.vs
    ends = {}
    for k in range(1, ts.D_MU + 1):
        start = ts.displaced(f, k)
        M, res = rt.track(f.posed, f.depth0, f.intr, start, **fx.RUN_PARAMS)
        ends[k] = (f.distance(start), f.distance(M))
        print(f"{k} mu: {ends[k][0]:.4g} voxels at the start, {ends[k][1]:.4g} after {res['evaluations']} evaluations")
        assert abs(ends[k][0] - k * mu_voxels) < 1e-3
    for k in range(1, ts.D_MU):
        assert ends[k][1] < 0.5 * ends[k][0]
    assert ends[ts.D_MU][1] >= 0.5 * ends[ts.D_MU][0]


def test_the_lattice_puts_its_cheapest_node_inside_the_basin():
    f = ts.fixture()
    nodes, evs = ts.reference_scores()
    assert len(nodes) == 27 and nodes[13].tobytes() == ts.displaced(f).tobytes()
    cost = [np.float32(ev.cost) for ev in evs]
    valid = [ev.valid for ev in evs]
    kept = ts.select(valid, cost, fx.RUN_PARAMS["min_valid"], ts.KEEP)
    best = kept[0]
    d_best = f.distance(nodes[best])
    print(f"{sum(v >= fx.RUN_PARAMS['min_valid'] for v in valid)} of {len(nodes)} nodes qualify; kept {kept} with costs "
          f"{[float(cost[k]) for k in kept]}; the cheapest lies {d_best:.4g} voxels from the truth")
    assert best == ts.BEST_NODE and abs(d_best - ts.BEST_NODE_DISTANCE) < 1e-3
    # the order of the first two does not hang on rounding: their cost intervals are far apart
    assert evs[kept[0]].cost_interval()[1] < evs[kept[1]].cost_interval()[0]
    assert len(kept) == ts.KEEP
    # inside the basin: nearer than the displacement of one mu the single call recovers, and the run from it ends within a
    # quarter of its distance, as the 1 voxel / 5 mrad runs of test_track_sdf_ref.py do
    assert d_best < f.maps[0].mu / f.vs
    M, res = rt.track(f.posed, f.depth0, f.intr, nodes[best], **fx.RUN_PARAMS)
    end = f.distance(M)
    print(f"tracked from it: {end:.4g} voxels after {res['evaluations']} evaluations, stop reason {res['stop_reason']}")
    assert end < 0.25 * d_best and abs(end - ts.REFERENCE_END) < 1e-4 and res["stop_reason"] != 3
    assert res["valid_last"] >= fx.RUN_PARAMS["min_valid"]


def test_the_numpy_lattice_states_the_law(pkg):
    """track_starts_fixtures.lattice_poses against the library's host function on the case's own lattice and on one with
    rotation nodes: the same poses to float32 rounding, the same order."""
    import ctypes
    pkg._share_torch_hip_runtime()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    f = ts.fixture()
    for args in (ts.LATTICE, dict(nt=(1, 0, 2), step_t=0.013, nr=2, step_r=0.04, axis=(0.3, -1.0, 0.2))):
        lat = pkg.PoseLattice(**args)
        out = np.zeros(lat.count * 16, np.float32)
        count = ctypes.c_int32(0)
        fptr = ctypes.POINTER(ctypes.c_float)
        assert lib.dslam_camera_pose_lattice(pkg.mat_to_abi(ts.displaced(f)).ctypes.data_as(fptr), ctypes.byref(lat),
                                             out.ctypes.data_as(fptr), lat.count, ctypes.byref(count)) == 0
        want = ts.lattice_poses(ts.displaced(f), **args)
        got = out.reshape(-1, 4, 4).transpose(0, 2, 1)
        assert count.value == len(want) and np.abs(got.astype(np.float64) - want.astype(np.float64)).max() < 1e-6


def test_the_binding_exists(pkg):
    import ctypes
    assert ctypes.sizeof(pkg.PoseScore) == 16 and ctypes.sizeof(pkg.PoseLattice) == 40 and pkg.MAX_TRACK_STARTS == 256
    for name in ("score_camera_poses", "track_camera_sdf_starts", "debug_track_sdf_start_sums", "select_start_poses",
                 "camera_pose_lattice"):
        assert callable(getattr(pkg.CApi, name))
        assert "dslam_" + name in pkg.exported_symbols()
    assert b"k_track_sdf_starts" in open(pkg.LIB_PATH, "rb").read() and b"k_track_sdf_row_sum" in open(pkg.LIB_PATH, "rb").read()
