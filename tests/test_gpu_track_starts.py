"""dslam_score_camera_poses and dslam_track_camera_sdf_starts on the MI355X.  The acceptance
criterion is byte-identity with dslam_track_camera_sdf called alone from each pose, so the float64 evidence of
test_gpu_track_sdf.py carries over; on top of it: the scores against the float64 law directly, pixel coverage of the
two-dimensional grid, the relocalisation case test_track_starts_ref.py fixes on the reference, side effects, rejections and
the ITMLib mirror (RelocaliseAllLocalMaps)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_track_sdf as rt
import track_sdf_fixtures as fx
import track_starts_fixtures as ts
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "relocalise_harness")
LANES = 512 * 256   # the fixed stride of k_track_sdf_starts: a level with more jobs takes a second trip
GATE2 = np.float32(0.75 * 0.75)


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


@pytest.fixture(scope="module")
def loaded(pkg, gpu):
    """Uploaded fixture maps (one scene per map) and views (one per depth image), shared by the tests of this file: none of
    them writes a map."""
    scenes, views = {}, {}

    def get(f):
        out = []
        for m in f.maps:
            if id(m) not in scenes:
                scenes[id(m)] = (m, upload_map(gpu, pkg, m))
            out.append(scenes[id(m)][1])
        if id(f) not in views:
            v = gpu.create_view(f.w, f.h)
            gpu.view_update(v, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
            views[id(f)] = (f, v)
        return out, views[id(f)][1]

    return get


def far_pose(f):
    """The true pose with the camera 3 m away: no pixel's point lies within any map's band."""
    M = f.M_true.astype(np.float64).copy()
    M[0, 3] += 3.0
    return M.astype(np.float32)


def score_poses(f):
    return [f.M_true, f.start(2.0, 0.3), f.start(5.0, 1.0), f.start(-5.0, -1.0), far_pose(f), f.start(5.0, 1.0)]


def single_score(pkg, gpu, view, scenes, T, pose, intr, level, gate=0.0):
    """(candidates, valid, cost as float32) of the single call's one evaluation of `pose` on `level`."""
    params = pkg.TrackSdfParams(no_hierarchy_levels=level + 1, run_till_level=level, max_evaluations=1, residual_gate=gate)
    M, res = gpu.track_camera_sdf(view, scenes, T, pose, intr, params)
    assert M.tobytes() == np.asarray(pose, np.float32).tobytes() and res.cost_last == res.cost_first
    return res.candidates, res.valid_last, np.float32(res.cost_first)


def as_tuples(scores):
    return [(s.candidates, s.valid, np.float32(s.cost).tobytes(), s.pad) for s in scores]


def check_scores_against_single(pkg, gpu, view, scenes, f, poses, level, gate=0.0):
    scores = gpu.score_camera_poses(view, scenes, f.T, poses, f.intr, level, gate)
    assert len(scores) == len(poses)
    for k, (s, pose) in enumerate(zip(scores, poses)):
        cand, valid, cost = single_score(pkg, gpu, view, scenes, f.T, pose, f.intr, level, gate)
        assert (s.candidates, s.valid, s.pad) == (cand, valid, 0) and np.float32(s.cost).tobytes() == cost.tobytes(), \
            (f.name, level, k, (s.candidates, s.valid, s.cost), (cand, valid, cost))
    return scores


# ---------------------------------------------------------------------------------------------------------------------
# 1. scores against the single call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", range(3))
@pytest.mark.parametrize("which", ["three", "ramp"])
def test_scores_equal_the_single_call(pkg, gpu, loaded, which, level):
    f = {"three": fx.three_maps, "ramp": fx.ramp_spheres}[which]()
    scenes, view = loaded(f)
    poses = score_poses(f)
    scores = check_scores_against_single(pkg, gpu, view, scenes, f, poses, level)
    got = as_tuples(scores)
    print(f"{f.name}, level {level}: " + "; ".join(f"{s.valid}/{s.candidates} {s.cost:.5g}" for s in scores))
    assert scores[0].candidates > ((f.w >> level) * (f.h >> level)) // 4 and scores[0].valid > 0.5 * scores[0].candidates
    assert got[2] == got[5]                                    # the same pose twice in one list
    assert len({g for g in got[:5]}) == 5                      # ... and five different ones
    assert (scores[4].candidates, scores[4].valid) == (scores[0].candidates, 0) and np.float32(scores[4].cost) == GATE2
    # a permuted list gives permuted outputs
    perm = [3, 5, 0, 4, 1, 2]
    again = as_tuples(gpu.score_camera_poses(view, scenes, f.T, [poses[k] for k in perm], f.intr, level))
    assert again == [got[k] for k in perm]


def test_one_pose_and_256_poses_agree_elementwise(pkg, gpu, loaded):
    f = fx.three_maps()
    scenes, view = loaded(f)
    poses = [f.start(0.05 * k - 6.0, 0.01 * k - 1.2) for k in range(pkg.MAX_TRACK_STARTS)]
    assert len({p.tobytes() for p in poses}) == 256
    all256 = as_tuples(gpu.score_camera_poses(view, scenes, f.T, poses, f.intr, 2))
    alone = [as_tuples(gpu.score_camera_poses(view, scenes, f.T, [p], f.intr, 2))[0] for p in poses]
    assert all256 == alone and len(set(all256)) > 200
    for k in (0, 100, 255):
        cand, valid, cost = single_score(pkg, gpu, view, scenes, f.T, poses[k], f.intr, 2)
        assert all256[k] == (cand, valid, cost.tobytes(), 0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. scores against the law itself
# ---------------------------------------------------------------------------------------------------------------------
def test_scores_against_the_float64_reference(pkg, gpu, loaded):
    f = fx.three_maps()
    scenes, view = loaded(f)
    poses = score_poses(f)[:3]
    for level in (0, 2):
        depth, intr = rt.pyramid(f.depth0, f.intr, level + 1)[level]
        scores = gpu.score_camera_poses(view, scenes, f.T, poses, f.intr, level)
        for s, pose in zip(scores, poses):
            ev = rt.evaluate(f.posed, depth, intr, rt.camera_to_world(pose, f.vs))
            lo, hi = ev.cost_interval()
            print(f"level {level}: {s.valid} of {s.candidates} valid (reference {ev.valid}, {ev.ties} ties), cost {s.cost:.6g} in "
                  f"[{lo:.6g}, {hi:.6g}]")
            assert s.candidates == ev.candidates and abs(s.valid - ev.valid) <= ev.ties
            assert lo <= s.cost <= hi


# ---------------------------------------------------------------------------------------------------------------------
# 3. pixel coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_pixel_coverage(pkg, gpu, loaded):
    """70 x 45 (partial tiles and waves; 54 tiles: fewer workgroups than the single call's 512); 416 x 320 with three poses
    (133120 pixels: a second trip under the fixed stride, 512 workgroups per pose); 70 x 45 again on the same engine (the
    rows of the larger run must not leak into the smaller one's sums); a view that is all holes."""
    small, big = fx.identity_box(70, 45), fx.identity_box(416, 320)
    assert big.w * big.h > LANES and small.w % 8 and small.h % 8
    scenes, v_small = loaded(small)
    _, v_big = loaded(big)
    p_small = [small.M_true, small.start(2.0, 0.3), small.start(5.0, 1.0), far_pose(small)]
    first = as_tuples(check_scores_against_single(pkg, gpu, v_small, scenes, small, p_small, 0))
    p_big = [big.start(2.0, 0.3), big.M_true, big.start(5.0, 1.0)]
    s_big = check_scores_against_single(pkg, gpu, v_big, scenes, big, p_big, 0)
    assert s_big[0].candidates > LANES * 0.99 and s_big[0].valid > 0.5 * s_big[0].candidates
    again = as_tuples(check_scores_against_single(pkg, gpu, v_small, scenes, small, p_small, 0))
    assert first == again
    # the starts on the large image too: the iteration's rounds take the second trip
    params = pkg.TrackSdfParams(max_evaluations=3)
    M, res = gpu.track_camera_sdf_starts(v_big, scenes, big.T, p_big[:2], big.intr, params)
    for k in range(2):
        M1, r1 = gpu.track_camera_sdf(v_big, scenes, big.T, p_big[k], big.intr, params)
        assert M[k].tobytes() == M1.tobytes() and bytes(res[k]) == bytes(r1)
    holes = gpu.create_view(small.w, small.h)
    gpu.view_update(holes, np.zeros((small.h, small.w, 4), np.uint8), np.zeros((small.h, small.w), np.int16))
    for level in (0, 2):
        for s in gpu.score_camera_poses(holes, scenes, small.T, p_small, small.intr, level):
            assert (s.candidates, s.valid) == (0, 0) and np.float32(s.cost) == GATE2
    M, res = gpu.track_camera_sdf_starts(holes, scenes, small.T, p_small, small.intr)
    for k, pose in enumerate(p_small):
        M1, r1 = gpu.track_camera_sdf(holes, scenes, small.T, pose, small.intr)
        assert M[k].tobytes() == M1.tobytes() == np.asarray(pose, np.float32).tobytes() and bytes(res[k]) == bytes(r1)
        assert res[k].stop_reason == 3 and res[k].evaluations == 3 and not np.any(gpu.debug_track_sdf_start_sums(k))


# ---------------------------------------------------------------------------------------------------------------------
# 4. starts against the single call
# ---------------------------------------------------------------------------------------------------------------------
def check_starts_against_single(pkg, gpu, view, scenes, f, starts, params):
    singles = []
    for pose in starts:
        M1, r1 = gpu.track_camera_sdf(view, scenes, f.T, pose, f.intr, params)
        singles.append((M1, r1, gpu.debug_track_sdf_sums()))
    M, res = gpu.track_camera_sdf_starts(view, scenes, f.T, starts, f.intr, params)
    assert M.shape == (len(starts), 4, 4) and len(res) == len(starts)
    for k, (M1, r1, s1) in enumerate(singles):
        what = (f.name, k, res[k].as_dict(), r1.as_dict())
        assert bytes(res[k]) == bytes(r1), what
        assert M[k].tobytes() == M1.tobytes(), what
        assert gpu.debug_track_sdf_start_sums(k).tobytes() == s1.tobytes(), what
    return M, res, singles


def test_starts_equal_the_single_call(pkg, gpu, loaded):
    f = fx.three_maps()
    scenes, view = loaded(f)
    params = pkg.TrackSdfParams(**fx.RUN_PARAMS)
    # (the 10 mrad / 2 voxel start is the one whose finest level stops early: 23 evaluations next to the others' 26)
    starts = [f.start(5.0, 1.0), f.start(10.0, 2.0), f.M_true, f.start(-5.0, -1.0), far_pose(f)]
    M, res, singles = check_starts_against_single(pkg, gpu, view, scenes, f, starts, params)
    counts = [r.evaluations for _, r, _ in singles]
    print(f"{f.name}: evaluations {counts}, stop reasons {[r.stop_reason for _, r, _ in singles]}, distances "
          f"{[round(f.distance(m), 4) for m in M]}")
    # idle starts sit next to running ones
    assert len(set(counts)) >= 3
    assert res[4].stop_reason == 3 and res[4].evaluations == 3 and res[4].levels_stepped == 0 and res[4].valid_last == 0
    assert M[4].tobytes() == starts[4].tobytes()
    assert f.distance(M[0]) < 0.25 * f.distance(starts[0]) and res[0].levels_stepped == 7
    # the order of the starts is nobody's business but the caller's
    perm = [4, 2, 0, 3, 1]
    Mp, rp = gpu.track_camera_sdf_starts(view, scenes, f.T, [starts[k] for k in perm], f.intr, params)
    for at, k in enumerate(perm):
        assert Mp[at].tobytes() == M[k].tobytes() and bytes(rp[at]) == bytes(res[k])
        assert gpu.debug_track_sdf_start_sums(at).tobytes() == singles[k][2].tobytes()
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu.debug_track_sdf_start_sums(5)
    # one posed map, one start, default parameters but min_valid
    g = fx.posed_box()
    g_scenes, g_view = loaded(g)
    _, r_one, _ = check_starts_against_single(pkg, gpu, g_view, g_scenes, g, [g.start()], params)
    assert r_one[0].levels_stepped == 7
    # run_till_level and max_evaluations reach the starts as they reach the single call
    check_starts_against_single(pkg, gpu, view, scenes, f, starts[:3], pkg.TrackSdfParams(run_till_level=1, max_evaluations=4, min_valid=100))
    check_starts_against_single(pkg, gpu, view, scenes, f, starts[:2], pkg.TrackSdfParams(max_evaluations=1, min_valid=100))


# ---------------------------------------------------------------------------------------------------------------------
# 5. relocalisation
# ---------------------------------------------------------------------------------------------------------------------
def test_relocalisation_from_beyond_the_band(pkg, gpu, loaded):
    """The case test_track_starts_ref.py fixes: two truncation bands off, the single call goes nowhere; lattice -> scores ->
    selection -> starts -> the winner by the mirror's rule ends within twice the reference's end distance."""
    f = ts.fixture()
    scenes, view = loaded(f)
    params = pkg.TrackSdfParams(**fx.RUN_PARAMS)
    start = ts.displaced(f)
    d0 = f.distance(start)
    M_single, r_single = gpu.track_camera_sdf(view, scenes, f.T, start, f.intr, params)
    assert f.distance(M_single) >= 0.5 * d0
    nodes = gpu.camera_pose_lattice(start, pkg.PoseLattice(**ts.LATTICE))
    assert len(nodes) == 27 and nodes[13].tobytes() == start.tobytes()
    scores = gpu.score_camera_poses(view, scenes, f.T, nodes, f.intr, ts.SCORE_LEVEL)
    kept = gpu.select_start_poses(scores, fx.RUN_PARAMS["min_valid"], ts.KEEP)
    assert len(kept) == ts.KEEP and kept[0] == ts.BEST_NODE
    M, res = gpu.track_camera_sdf_starts(view, scenes, f.T, nodes[kept], f.intr, params)
    win = ts.winner(res, fx.RUN_PARAMS["min_valid"])
    assert win is not None
    print(f"single call: {d0:.4g} -> {f.distance(M_single):.4g} voxels (stop {r_single.stop_reason}); kept nodes {kept.tolist()} at "
          f"{[round(f.distance(nodes[k]), 3) for k in kept]} voxels, tracked to {[round(f.distance(m), 4) for m in M]} with cost "
          f"{[r.cost_last for r in res]}; winner: start {win} (node {kept[win]})")
    assert f.distance(M[win]) <= 2 * ts.REFERENCE_END


# ---------------------------------------------------------------------------------------------------------------------
# 6. side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    f = fx.three_maps()
    scenes = [upload_map(gpu, pkg, m) for m in f.maps]
    view = gpu.create_view(f.w, f.h)
    gpu.view_update(view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    before = [util.snapshot(gpu, s) for s in scenes]
    rs = gpu.create_render_state(scenes[0], f.w, f.h)
    M_map0 = (f.M_true.astype(np.float64) @ np.linalg.inv(f.T[0].astype(np.float64))).astype(np.float32)
    seen = gpu.get_image(scenes[0], rs, M_map0, f.intr, pkg.IMAGE_DEPTH).copy()
    params = pkg.TrackSdfParams(**fx.RUN_PARAMS)
    starts = [f.start(5.0, 1.0), far_pose(f), f.start(2.0, 0.3)]

    def run():
        sc = as_tuples(gpu.score_camera_poses(view, scenes, f.T, starts, f.intr, 1))
        M, res = gpu.track_camera_sdf_starts(view, scenes, f.T, starts, f.intr, params)
        return sc, M.tobytes(), [bytes(r) for r in res], [gpu.debug_track_sdf_start_sums(k).tobytes() for k in range(len(starts))]

    first, second = run(), run()
    assert first == second
    assert np.array_equal(gpu.get_image(scenes[0], rs, M_map0, f.intr, pkg.IMAGE_DEPTH), seen) and (seen > 0).sum() > 1000
    # an asynchronous engine with work in flight: frames being fused into another scene
    wl = synth.s_tiny()
    third = gpu.create_scene(util.small_params(pkg, wl))
    rs3 = gpu.create_render_state(third, wl.W, wl.H)
    view3 = gpu.create_view(wl.W, wl.H)
    try:
        gpu.set_async(True)
        for i in range(3):
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view3, rgba, mm, timestamp=float(i))
            gpu.process_frame(third, view3, rs3, M, wl.intr)
        third_run = run()
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert third_run == first
    for s, snap in zip(scenes, before):
        util.assert_same_state(snap, util.snapshot(gpu, s), "a tracked map")
        assert snap["stats"] == gpu.stats(s)


# ---------------------------------------------------------------------------------------------------------------------
# 7. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_every_output_untouched(pkg, gpu, loaded):
    f = fx.posed_box()
    (A,), view = loaded(f)
    m = f.maps[0]
    other_vs, other_mu = upload_map(gpu, pkg, m, voxel_size=0.006), upload_map(gpu, pkg, m, mu=0.03)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = upload_map(second, pkg, m)
    foreign_view = second.create_view(f.w, f.h)
    second.view_update(foreign_view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    fresh_view = gpu.create_view(f.w, f.h)          # never updated
    B = upload_map(gpu, pkg, m)
    T = f.T[0]
    good = [f.start(), f.start(2.0, 0.3), f.M_true]
    nan, skew = f.start().copy(), f.start().copy()
    nan[1, 3] = np.nan
    skew[:3, :3] *= 1.01
    T_nan, T_skew = T.copy(), T.copy()
    T_nan[0, 0] = np.inf
    T_skew[0, 1] += 0.01
    fptr = C.POINTER(C.c_float)

    def call(which, v=view, scenes=(A,), Ts=(T,), poses=good, intr=f.intr, params=None, n=None, k=None, null=(), level=0, gate=0.0):
        count = len(poses) if k is None else k
        P = np.concatenate([pkg.mat_to_abi(p) for p in poses] + [np.zeros(16, np.float32)] * max(count - len(poses), 0))
        keep = P.copy()
        ptrs = (C.c_void_p * max(len(scenes), 1))(*[None if s is None else s.ptr for s in scenes])
        t_abi = np.concatenate([pkg.mat_to_abi(t) for t in Ts]) if len(Ts) else np.zeros(16, np.float32)
        kk = np.ascontiguousarray(intr, np.float32)
        out = np.full(max(count, len(poses), 1) * 8, 0x5a5a5a5a, np.uint32)   # 32 bytes per start, 16 per score
        filled = out.copy()
        head = (gpu._engine, None if "view" in null else v.ptr, None if "scenes" in null else ptrs,
                None if "T" in null else t_abi.ctypes.data_as(fptr), C.c_int(len(scenes) if n is None else n),
                None if "poses" in null else P.ctypes.data_as(fptr), C.c_int(count), None if "intr" in null else kk.ctypes.data_as(fptr))
        outp = None if "out" in null else out.ctypes.data_as(C.c_void_p)
        with pytest.raises(pkg.DslamError, match="status -1 "):
            if which == "score":
                gpu._call("score_camera_poses", *head, C.c_int(level), C.c_float(gate), outp)
            else:
                gpu._call("track_camera_sdf_starts", *head, C.byref(params) if params is not None else None, outp)
        assert P.tobytes() == keep.tobytes() and out.tobytes() == filled.tobytes()

    for which in ("score", "starts"):
        for what in ("view", "scenes", "T", "poses", "intr", "out"):
            call(which, null=(what,))
        call(which, scenes=(None,))
        call(which, n=0)
        call(which, n=pkg.MAX_RENDER_MAPS + 1)
        call(which, scenes=(A, A), Ts=(T, T))
        call(which, scenes=(A, foreign), Ts=(T, T))
        call(which, v=foreign_view)
        call(which, v=fresh_view)
        call(which, scenes=(A, other_vs), Ts=(T, T))
        call(which, scenes=(A, other_mu), Ts=(T, T))
        call(which, Ts=(T_nan,))
        call(which, scenes=(A, B), Ts=(T, T_skew))
        call(which, intr=np.array([np.nan, 1, 1, 1], np.float32))
        # the pose list: its length, and a bad pose anywhere in it
        call(which, k=0)
        call(which, k=-1)
        call(which, poses=[f.M_true] * (pkg.MAX_TRACK_STARTS + 1))
        for at in range(3):
            for bad in (nan, skew):
                call(which, poses=good[:at] + [bad] + good[at + 1:])
    for level in (-1, 7, 8, 100):           # 96 x 72 has levels 0 .. 6
        call("score", level=level)
    call("score", gate=-1.0)
    call("score", gate=float("nan"))
    call("starts", params=pkg.TrackSdfParams(no_hierarchy_levels=9))
    call("starts", params=pkg.TrackSdfParams(no_hierarchy_levels=8))
    call("starts", params=pkg.TrackSdfParams(no_hierarchy_levels=2, run_till_level=2))
    call("starts", params=pkg.TrackSdfParams(run_till_level=3))
    for field in ("no_hierarchy_levels", "run_till_level", "max_evaluations", "min_valid", "residual_gate", "term_rotation",
                  "term_translation_voxels"):
        call("starts", params=pkg.TrackSdfParams(**{field: -1}))
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("debug_track_sdf_start_sums", gpu._engine, C.c_int(0), None)
    with pytest.raises(pkg.DslamError, match="status -1 "):
        second.debug_track_sdf_start_sums(0)      # no _starts call has run on that engine
    # the largest list is accepted, level 6 (1 x 1 pixel) is a level, and NULL params are the defaults
    s = gpu.score_camera_poses(view, [A], [T], [f.M_true] * pkg.MAX_TRACK_STARTS, f.intr, 6)
    assert len({t for t in as_tuples(s)}) == 1 and s[0].candidates <= 1
    Md, rd = gpu.track_camera_sdf_starts(view, [A], [T], good, f.intr)
    Me, re_ = gpu.track_camera_sdf_starts(view, [A], [T], good, f.intr, pkg.TrackSdfParams(3, 0, 10, 500, 0.75, 1e-5, 1e-3))
    assert Md.tobytes() == Me.tobytes() and [bytes(r) for r in rd] == [bytes(r) for r in re_] and rd[0].levels_stepped == 3


# ---------------------------------------------------------------------------------------------------------------------
# 8. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
KEYFRAMES, HELD_OUT = (40, 44, 48), 47      # S-tiny, as test_gpu_track_sdf.py's mirror test


def _rigid_inverse(M):
    """ITMMainEngine::RigidInverse on a column-major list of 16 Python floats (doubles), operation for operation."""
    out = [0.0] * 16
    for r in range(3):
        for c in range(3):
            out[c * 4 + r] = M[r * 4 + c]
        out[12 + r] = -((M[r * 4 + 0] * M[12] + M[r * 4 + 1] * M[13]) + M[r * 4 + 2] * M[14])
    out[15] = 1.0
    return out


def _rigid_product(A, B):
    """ITMMainEngine::RigidProduct, operation for operation."""
    return [((A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1]) + A[2 * 4 + r] * B[c * 4 + 2]) + A[3 * 4 + r] * B[c * 4 + 3]
            for c in range(4) for r in range(4)]


def _as_doubles(abi16):
    return [float(v) for v in np.asarray(abi16, np.float32)]


def test_mirror_relocalise_all_local_maps_equals_abi(pkg, gpu, synth, tmp_path):
    """relocalise_harness: two local maps fused from S-tiny keyframes and a current local map that has just been created,
    whose pose_d is the held-out frame's true pose moved by 5 voxels (the band is 4); RelocaliseAllLocalMaps(current, ...)
    puts pose_d exactly where the ABI sequence lattice -> scores -> selection -> starts -> winner puts the camera on the
    same maps, re-fused through the C ABI."""
    wl = synth.s_tiny(80, 60)
    p = util.small_params(pkg, wl)
    vs = p.voxel_size
    frames = [wl.frame(i) for i in KEYFRAMES]
    rgba, mm, M_true = wl.frame(HELD_OUT)
    start = (rt.rigid(0.0, (0.3, 0.8, -0.52), 5.0 * vs * np.array([0.6, -0.64, 0.48]), (0.0, 0.0, 2.0)) @ M_true.astype(np.float64)).astype(np.float32)
    D = rt.rigid(0.12, (0.42, -0.61, 0.67), (0.05, -0.03, 0.04)).astype(np.float32)
    E = rt.rigid(-0.07, (0.1, 0.9, 0.2), (-0.02, 0.01, 0.03)).astype(np.float32)
    lattice = pkg.PoseLattice(nt=(1, 1, 1), step_t=float(np.float32(3.0 * vs)), nr=1, step_r=0.004, axis=(0.0, 1.0, 0.0))
    score_level, keep = 1, 5                 # level 1 of 80 x 60 has 1200 pixels; level 2 has 300, below the default min_valid
    n = len(frames)
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<3i", wl.W, wl.H, n + 1))
        for a, b, M in frames + [(rgba, mm, start)]:
            fh.write(a.tobytes()); fh.write(b.tobytes()); fh.write(pkg.mat_to_abi(M).tobytes())
        fh.write(np.asarray(wl.intr, np.float32).tobytes())
        fh.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        fh.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        fh.write(pkg.mat_to_abi(D).tobytes()); fh.write(pkg.mat_to_abi(E).tobytes())
        fh.write(bytes(lattice)); fh.write(struct.pack("<2i", score_level, keep))
    run = subprocess.run([HARNESS, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    T = [np.frombuffer(raw, np.float32, 16, 64 * k) for k in range(3)]
    before, after = (np.frombuffer(raw, np.float32, 16, 192 + 64 * k) for k in range(2))
    fused = np.frombuffer(raw, np.float32, 16 * 2 * n, 320).reshape(2, n, 4, 4).transpose(0, 1, 3, 2)
    tail = 320 + 64 * 2 * n
    assert len(raw) == tail + 36
    res_h = pkg.TrackSdfResult.from_buffer_copy(raw[tail:tail + 32])
    found, = struct.unpack_from("<i", raw, tail + 32)
    # the same maps through the C ABI
    view = gpu.create_view(wl.W, wl.H)
    made = []
    for k in range(2):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (a, b, _) in enumerate(frames):
            gpu.view_update(view, a, b, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    made.append(gpu.create_scene(p))
    gpu.view_update(view, rgba, mm, timestamp=float(n))
    Ts = [t.reshape(4, 4).T for t in T]
    W0 = np.array(_rigid_product(_as_doubles(before), _as_doubles(T[2])), np.float64).astype(np.float32).reshape(4, 4).T
    nodes = gpu.camera_pose_lattice(W0, lattice)
    scores = gpu.score_camera_poses(view, made, Ts, nodes, wl.intr, score_level)
    kept = gpu.select_start_poses(scores, 500, keep)
    M, res = gpu.track_camera_sdf_starts(view, made, Ts, nodes[kept], wl.intr)
    win = ts.winner(res, 500)
    corners_depth = gpu.download_view_depth(view)
    _, seen, _ = rt.world_points(corners_depth, wl.intr, rt.camera_to_world(M_true, vs), vs)
    lo, hi = seen.min(0) * vs, seen.max(0) * vs
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    dist = lambda X: rt.pose_distance(X, M_true, corners, vs)
    print(f"mirror: {run.stdout.strip()}; C ABI: {len(nodes)} nodes, kept {kept.tolist()}, winner {win}: "
          f"{dist(W0):.4g} -> {dist(M[win]) if win is not None else float('nan'):.4g} voxels")
    assert len(nodes) == 81 and len(kept) == keep and win is not None and found == 1
    assert bytes(res[win]) == bytes(res_h)
    want = _rigid_product(_as_doubles(pkg.mat_to_abi(M[win])), _rigid_inverse(_as_doubles(T[2])))
    assert np.array(want, np.float64).astype(np.float32).tobytes() == after.tobytes()
    assert after.tobytes() != before.tobytes()
    # and the camera moved towards the frame's true pose
    assert dist(M[win]) < dist(W0)
