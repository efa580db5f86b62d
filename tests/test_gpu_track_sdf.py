"""dslam_track_camera_sdf on the MI355X against the float64 reference of ref64_track_sdf.py: single evaluations sum by sum
within the derived rounding bound, maps that miss, pixel coverage of the fixed grid, the pyramid's levels, whole runs,
maps fused from frames (and the empty current map next to its neighbour), side effects, argument errors and the ITMLib
mirror (TrackAllLocalMaps)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_track_sdf as rt
import track_sdf_fixtures as fx
import util

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "track_sdf_harness")
LANES = 512 * 256   # kTrackSdfGrid x kTrackSdfThreads (track_sdf.hip): a level with more pixels takes a second trip


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
            assert np.array_equal(gpu.download_view_depth(v), f.depth0)   # level 0 is what the reference takes it to be
            views[id(f)] = (f, v)
        return out, views[id(f)][1]

    return get


def one_evaluation(pkg, gpu, view, scenes, T, pose, intr, level=0, **kw):
    params = pkg.TrackSdfParams(no_hierarchy_levels=level + 1, run_till_level=level, max_evaluations=1, **kw)
    M, res = gpu.track_camera_sdf(view, scenes, T, pose, intr, params)
    return M, res, gpu.debug_track_sdf_sums()


def check_evaluation(pkg, gpu, loaded, f, pose, level=0, maps=None, min_valid=500, gate=0.75):
    """One evaluation of fixture f (its maps `maps`, default all) at `pose` on `level` against the reference."""
    scenes, view = loaded(f)
    pick = list(range(len(f.maps))) if maps is None else maps
    depth, intr = rt.pyramid(f.depth0, f.intr, level + 1)[level]
    ev = rt.evaluate([f.posed[i] for i in pick], depth, intr, rt.camera_to_world(pose, f.vs), gate=gate)
    M, res, sums = one_evaluation(pkg, gpu, view, [scenes[i] for i in pick], [f.T[i] for i in pick], pose, f.intr, level,
                                  residual_gate=gate)
    what = f"{f.name}, level {level}"
    used = ev.check_sums(sums, what)
    lo, hi = ev.cost_interval()
    print(f"{what}: {ev.candidates} candidates, {ev.valid} valid, {ev.ties} ties, {ev.maps_per_pixel:.2f} maps per pixel; the sums "
          f"use up to {used:.3f} of the bound; cost {res.cost_first:.6g} in [{lo:.6g}, {hi:.6g}]")
    assert res.candidates == ev.candidates and abs(res.valid_last - ev.valid) <= ev.ties
    assert lo <= res.cost_first <= hi and res.cost_last == res.cost_first
    assert res.evaluations == 1 and res.levels_stepped == 0 and res.stop_reason == (3 if res.valid_last < min_valid else 1)
    assert M.tobytes() == np.asarray(pose, np.float32).tobytes()
    return ev, res, sums


# ---------------------------------------------------------------------------------------------------------------------
# 1. single evaluations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_single_evaluation_against_the_reference(pkg, gpu, loaded, case):
    f, pose = fx.single_evaluations()[case]
    ev, _, sums = check_evaluation(pkg, gpu, loaded, f, pose)
    assert ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates
    if f is fx.ramp_spheres():
        # the two wrong weight laws lie far outside the interval the engine's sums were just found in
        for law in ("tap0", "unweighted"):
            wrong = rt.evaluate(f.posed, f.depth0, f.intr, rt.camera_to_world(pose, f.vs), weight_law=law)
            assert not (ev.lo[27] <= wrong.sums[27] <= ev.hi[27])
            assert abs(wrong.sums[27] - sums[27]) > 20 * (ev.hi[27] - ev.lo[27])


@pytest.mark.parametrize("gate", [0.1, 0.15])
def test_the_residual_gate_turns_pixels_away(pkg, gpu, loaded, gate):
    """One voxel from the truth the blended value is about a quarter of the band: a gate of 0.1 keeps one pixel in nine, one
    of 0.15 seven in ten, and the counts, the sums and the cost (every miss pays the gate) are the reference's."""
    f = fx.three_maps()
    ev, res, _ = check_evaluation(pkg, gpu, loaded, f, f.start(), gate=gate)
    assert 0.05 * ev.candidates < ev.valid < 0.8 * ev.candidates and ev.tie_share < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# 2. a miss contributes nothing
# ---------------------------------------------------------------------------------------------------------------------
def test_a_map_that_misses_contributes_nothing(pkg, gpu, loaded):
    f = fx.posed_box()
    (A,), view = loaded(f)
    pose = f.start(2.0, 0.3)
    empty = gpu.create_scene(f.maps[0].scene_params(pkg))
    far = upload_map(gpu, pkg, fx.identity_box().maps[0])
    T_far = rt.rigid(0.3, (0.2, 0.5, 0.1), (3.0, 0.0, 0.0)).astype(np.float32)
    _, r0, s0 = one_evaluation(pkg, gpu, view, [A], f.T, pose, f.intr)
    _, r1, s1 = one_evaluation(pkg, gpu, view, [A, empty], [f.T[0], T_far], pose, f.intr)
    _, r2, s2 = one_evaluation(pkg, gpu, view, [A, far], [f.T[0], T_far], pose, f.intr)
    _, r3, s3 = one_evaluation(pkg, gpu, view, [empty, A, far], [I4, f.T[0], T_far], pose, f.intr)
    assert r0.valid_last > 3000
    assert s0.tobytes() == s1.tobytes() == s2.tobytes() == s3.tobytes()
    assert bytes(r0) == bytes(r1) == bytes(r2) == bytes(r3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. pixel coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_pixel_coverage(pkg, gpu, loaded):
    """70 x 45 (partial waves and partial tiles); 416 x 320 = 133120 pixels, more than the launch's 131072 lanes, so the
    pixel loop takes a second trip; 70 x 45 again on the same engine (idle workgroups must overwrite the rows of the large
    run); a view that is all holes."""
    small, big = fx.identity_box(70, 45), fx.identity_box(416, 320)
    assert big.w * big.h > LANES and small.w % 8 and small.h % 8
    first = check_evaluation(pkg, gpu, loaded, small, small.start(2.0, 0.3))[2]
    ev, _, _ = check_evaluation(pkg, gpu, loaded, big, big.start(2.0, 0.3))
    assert ev.candidates > LANES * 0.99 and ev.valid > 0.5 * ev.candidates
    again = check_evaluation(pkg, gpu, loaded, small, small.start(2.0, 0.3))[2]
    assert first.tobytes() == again.tobytes()
    scenes, _ = loaded(small)
    holes = gpu.create_view(small.w, small.h)
    gpu.view_update(holes, np.zeros((small.h, small.w, 4), np.uint8), np.zeros((small.h, small.w), np.int16))
    pose = small.start()
    M, res = gpu.track_camera_sdf(holes, scenes, small.T, pose, small.intr)
    assert res.candidates == 0 and res.valid_last == 0 and res.stop_reason == 3 and res.evaluations == 3
    assert res.levels_stepped == 0 and res.conditioning == 0.0 and abs(res.cost_first - 0.5625) < 1e-6
    assert M.tobytes() == pose.tobytes() and not np.any(gpu.debug_track_sdf_sums())


# ---------------------------------------------------------------------------------------------------------------------
# 4. levels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", range(3))
def test_each_level_against_the_reference(pkg, gpu, loaded, level):
    f = fx.three_maps()
    ev, _, _ = check_evaluation(pkg, gpu, loaded, f, f.start(2.0, 0.3), level=level)
    assert ev.candidates == (f.w >> level) * (f.h >> level)


# ---------------------------------------------------------------------------------------------------------------------
# 5. whole runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["identity", "posed", "three"])
def test_whole_run_against_the_reference(pkg, gpu, loaded, which):
    f, M_ref, ref = fx.reference_run(which)
    scenes, view = loaded(f)
    start = f.start()
    M, res = gpu.track_camera_sdf(view, scenes, f.T, start, f.intr, pkg.TrackSdfParams(**fx.RUN_PARAMS))
    d_ref, d_gpu, apart = f.distance(M_ref), f.distance(M), rt.pose_distance(M, M_ref, f.corners, f.vs)
    # a decision whose cost difference is below the rounding bound of the two costs may fall either way in float32
    order = sorted(ref["per_level"], reverse=True)
    tie_at = next(((lv, k) for lv in order for k, t in enumerate(ref["per_level"][lv]["trace"])
                   if k > 0 and t["margin"] < t["cost_slack"]), None)
    print(f"{f.name}: reference {ref['evaluations']} evaluations (stop {ref['stop_reason']}), engine {res.evaluations} (stop "
          f"{res.stop_reason}); distance to the truth {f.distance(start):.4g} -> {d_ref:.4g} / {d_gpu:.4g} voxel, apart {apart:.4g}; "
          f"first decision within the bound: (level, evaluation) {tie_at}")
    assert d_ref < 0.25 * f.distance(start) and apart <= 4 * d_ref and d_gpu <= 2 * d_ref
    assert res.candidates == ref["candidates"]
    if tie_at is None:
        M_cap, cap, M_g, r_g = M_ref, ref, M, res
    else:
        # compare up to the evaluation before that decision: both runs capped there
        top = order[0]
        kw = dict(fx.RUN_PARAMS)
        kw.update(dict(run_till_level=top, max_evaluations=tie_at[1]) if tie_at[0] == top else dict(run_till_level=tie_at[0] + 1))
        assert tie_at != (top, 1)
        M_cap, cap = rt.track(f.posed, f.depth0, f.intr, start, **kw)
        M_g, r_g = gpu.track_camera_sdf(view, scenes, f.T, start, f.intr, pkg.TrackSdfParams(**kw))
    assert r_g.evaluations == cap["evaluations"] and r_g.stop_reason == cap["stop_reason"]
    assert r_g.levels_stepped == cap["levels_stepped"]
    assert abs(r_g.valid_last - cap["valid_last"]) <= max(cap["last"].ties, 1)
    assert abs(r_g.conditioning - cap["conditioning"]) <= 1e-3 * cap["conditioning"] + 1e-6
    # the same accepted steps: the poses differ by float32 rounding of the sums only
    assert rt.pose_distance(M_g, M_cap, f.corners, f.vs) <= max(4 * d_ref, 1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 6. maps fused from frames
# ---------------------------------------------------------------------------------------------------------------------
# S-tiny's keyframes per map and the held-out frame.  Maps fused from three frames at 2 cm voxels hold the surface to a
# few tenths of a voxel, and the camera's first frames see little more than two walls (conditioning 0.01); from frame 40 on
# the float64 reference brings the 1 voxel / 5 mrad offset below a quarter on both maps and on the first alone (measured on
# maps fused by the CPU oracle: 1.40 -> 0.20 and 0.25 voxel, conditioning 0.2).
KEYFRAMES, HELD_OUT = ((40, 44, 48), (42, 46, 50)), 47


def seen_corners(depth0, intr, M_true, vs):
    """The corners (metres, world) of the box around the points a frame sees from its true pose: what the distances of the
    fused-map tests are measured on, as the fixtures' are."""
    _, seen, _ = rt.world_points(depth0, intr, rt.camera_to_world(M_true, vs), vs)
    lo, hi = seen.min(0) * vs, seen.max(0) * vs
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])


def test_fused_maps_and_the_empty_current_map(pkg, gpu, synth):
    """S-tiny keyframes fused into two scenes, the second under a non-identity world -> map transform; a held-out frame is
    tracked from its true pose moved by 1 voxel / 5 mrad.  Then the motivating case: the current local map is still empty
    and its neighbour holds the surface."""
    wl = synth.s_tiny(96, 72)
    p = util.small_params(pkg, wl)
    T_b = rt.rigid(0.12, (0.42, -0.61, 0.67), (0.05, -0.03, 0.04)).astype(np.float32)
    T = [I4, T_b]
    view = gpu.create_view(wl.W, wl.H)
    made = []
    for k in range(2):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i in KEYFRAMES[k]:
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, (M.astype(np.float64) @ np.linalg.inv(T[k].astype(np.float64))).astype(np.float32), wl.intr)
        made.append(scene)
    rgba, mm, M_true = wl.frame(HELD_OUT)
    gpu.view_update(view, rgba, mm, timestamp=float(HELD_OUT))
    depth0 = gpu.download_view_depth(view)
    posed = [rt.PosedMap(rt.MapData.of_scene(gpu, s), t) for s, t in zip(made, T)]
    vs = posed[0].data.vs
    corners = seen_corners(depth0, wl.intr, M_true, vs)
    centre = (M_true.astype(np.float64) @ np.append(corners.mean(0), 1.0))[:3]
    D = rt.rigid(5e-3, (0.3, 0.8, -0.52), vs * np.array([0.6, -0.64, 0.48]), centre)
    start = (D @ M_true.astype(np.float64)).astype(np.float32)
    kw = dict(min_valid=100)   # level 2 of 96 x 72 has 432 pixels, below the default of 500
    M_ref, ref = rt.track(posed, depth0, wl.intr, start, **kw)
    M, res = gpu.track_camera_sdf(view, made, T, start, wl.intr, pkg.TrackSdfParams(**kw))
    d0, d_ref, d_gpu = (rt.pose_distance(X, M_true, corners, vs) for X in (start, M_ref, M))
    print(f"fused maps: {res.candidates} candidates, {res.valid_last} valid, {ref['last'].maps_per_pixel:.2f} maps per pixel; "
          f"{d0:.4g} voxel at the start, {d_ref:.4g} after the reference ({ref['evaluations']} evaluations), {d_gpu:.4g} after the "
          f"engine ({res.evaluations})")
    assert res.candidates == ref["candidates"] > 3000 and ref["last"].maps_per_pixel > 1.2
    assert d_ref < 0.25 * d0          # the reference recovers the offset ...
    assert d_gpu <= 2 * d_ref         # ... and so does the engine
    # the current local map holds nothing yet
    current = gpu.create_scene(p)
    T_c = rt.rigid(-0.07, (0.1, 0.9, 0.2), (-0.02, 0.01, 0.03)).astype(np.float32)
    M_alone, r_alone = gpu.track_camera_sdf(view, [current], [T_c], start, wl.intr, pkg.TrackSdfParams(**kw))
    assert r_alone.stop_reason == 3 and r_alone.valid_last == 0 and r_alone.levels_stepped == 0
    assert M_alone.tobytes() == start.tobytes()
    M_both, r_both = gpu.track_camera_sdf(view, [current, made[0]], [T_c, T[0]], start, wl.intr, pkg.TrackSdfParams(**kw))
    M_one, r_one = gpu.track_camera_sdf(view, [made[0]], [T[0]], start, wl.intr, pkg.TrackSdfParams(**kw))
    assert M_both.tobytes() == M_one.tobytes() and bytes(r_both) == bytes(r_one)
    M_ref1, _ = rt.track(posed[:1], depth0, wl.intr, start, **kw)
    d_ref1, d_both = rt.pose_distance(M_ref1, M_true, corners, vs), rt.pose_distance(M_both, M_true, corners, vs)
    print(f"empty current map + neighbour: {d0:.4g} -> {d_both:.4g} voxel (reference {d_ref1:.4g})")
    assert d_ref1 < 0.25 * d0 and d_both <= 2 * d_ref1


# ---------------------------------------------------------------------------------------------------------------------
# 7. side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    f = fx.three_maps()
    scenes = [upload_map(gpu, pkg, m) for m in f.maps]
    view = gpu.create_view(f.w, f.h)
    gpu.view_update(view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    before = [util.snapshot(gpu, s) for s in scenes]
    # a GetImage of the first map: the same view asked for again after the tracking calls is still the same image
    rs = gpu.create_render_state(scenes[0], f.w, f.h)
    M_map0 = (f.M_true.astype(np.float64) @ np.linalg.inv(f.T[0].astype(np.float64))).astype(np.float32)
    seen = gpu.get_image(scenes[0], rs, M_map0, f.intr, pkg.IMAGE_DEPTH).copy()
    params = pkg.TrackSdfParams(**fx.RUN_PARAMS)
    M1, r1 = gpu.track_camera_sdf(view, scenes, f.T, f.start(), f.intr, params)
    s1 = gpu.debug_track_sdf_sums()
    M2, r2 = gpu.track_camera_sdf(view, scenes, f.T, f.start(), f.intr, params)
    s2 = gpu.debug_track_sdf_sums()
    assert M1.tobytes() == M2.tobytes() and bytes(r1) == bytes(r2) and s1.tobytes() == s2.tobytes()
    assert r1.levels_stepped == 7 and f.distance(M1) < 0.25 * f.distance(f.start())
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
        M3, r3 = gpu.track_camera_sdf(view, scenes, f.T, f.start(), f.intr, params)
        s3 = gpu.debug_track_sdf_sums()
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert M3.tobytes() == M1.tobytes() and bytes(r3) == bytes(r1) and s3.tobytes() == s1.tobytes()
    for s, snap in zip(scenes, before):
        util.assert_same_state(snap, util.snapshot(gpu, s), "a tracked map")
        assert snap["stats"] == gpu.stats(s)


# ---------------------------------------------------------------------------------------------------------------------
# 8. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_pose_untouched(pkg, gpu, loaded):
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
    start, T = f.start(), f.T[0]
    nan, skew = start.copy(), start.copy()
    nan[1, 3] = np.nan
    skew[:3, :3] *= 1.01
    T_nan, T_skew = T.copy(), T.copy()
    T_nan[0, 0] = np.inf
    T_skew[0, 1] += 0.01
    fptr = C.POINTER(C.c_float)

    def call(v=view, scenes=(A,), Ts=(T,), pose=start, intr=f.intr, params=None, result=True, n=None, null=()):
        P = pkg.mat_to_abi(pose).copy()
        keep = P.copy()
        ptrs = (C.c_void_p * max(len(scenes), 1))(*[None if s is None else s.ptr for s in scenes])
        t_abi = np.concatenate([pkg.mat_to_abi(t) for t in Ts]) if len(Ts) else np.zeros(16, np.float32)
        k = np.ascontiguousarray(intr, np.float32)
        res = pkg.TrackSdfResult()
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("track_camera_sdf", gpu._engine, None if "view" in null else v.ptr, None if "scenes" in null else ptrs,
                      None if "T" in null else t_abi.ctypes.data_as(fptr), C.c_int(len(scenes) if n is None else n),
                      None if "pose" in null else P.ctypes.data_as(fptr), None if "intr" in null else k.ctypes.data_as(fptr),
                      C.byref(params) if params is not None else None, C.byref(res) if result else None)
        assert P.tobytes() == keep.tobytes()

    for what in ("view", "scenes", "T", "pose", "intr"):
        call(null=(what,))
    call(result=False)
    call(scenes=(None,))
    call(n=0)
    call(n=pkg.MAX_RENDER_MAPS + 1)
    call(scenes=(A, A), Ts=(T, T))
    call(scenes=(A, foreign), Ts=(T, T))
    call(v=foreign_view)
    call(v=fresh_view)
    call(scenes=(A, other_vs), Ts=(T, T))
    call(scenes=(A, other_mu), Ts=(T, T))
    call(pose=nan)
    call(pose=skew)
    call(Ts=(T_nan,))
    call(scenes=(A, B), Ts=(T, T_skew))
    call(params=pkg.TrackSdfParams(no_hierarchy_levels=9))
    call(params=pkg.TrackSdfParams(no_hierarchy_levels=8))          # 96 x 72 has no level 7
    call(params=pkg.TrackSdfParams(no_hierarchy_levels=2, run_till_level=2))
    call(params=pkg.TrackSdfParams(run_till_level=3))               # the default has levels 0 .. 2
    for field in ("no_hierarchy_levels", "run_till_level", "max_evaluations", "min_valid", "residual_gate", "term_rotation",
                  "term_translation_voxels"):
        call(params=pkg.TrackSdfParams(**{field: -1}))
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("debug_track_sdf_sums", gpu._engine, None)
    # max_evaluations = 1 returns the start pose with stop reason 1
    M, res = gpu.track_camera_sdf(view, [A], [T], start, f.intr, pkg.TrackSdfParams(max_evaluations=1, min_valid=100))
    assert M.tobytes() == start.tobytes() and res.stop_reason == 1 and res.evaluations == 3 and res.levels_stepped == 0
    # NULL params are the defaults
    Md, rd = gpu.track_camera_sdf(view, [A], [T], start, f.intr)
    Me, re_ = gpu.track_camera_sdf(view, [A], [T], start, f.intr, pkg.TrackSdfParams(3, 0, 10, 500, 0.75, 1e-5, 1e-3))
    assert Md.tobytes() == Me.tobytes() and bytes(rd) == bytes(re_) and rd.levels_stepped == 3


# ---------------------------------------------------------------------------------------------------------------------
# 9. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
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


def test_mirror_track_all_local_maps_equals_abi(pkg, gpu, synth, tmp_path):
    """track_sdf_harness: two local maps fused from S-tiny keyframes (the second in a frame displaced by D, known to its
    estimatedGlobalPose) and a current local map that has just been created; TrackAllLocalMaps(current) moves the current
    map's pose_d exactly where track_camera_sdf on the same maps, re-fused through the C ABI, puts the camera."""
    wl = synth.s_tiny(80, 60)
    p = util.small_params(pkg, wl)
    vs = p.voxel_size
    frames = [wl.frame(i) for i in KEYFRAMES[0]]
    rgba, mm, M_true = wl.frame(HELD_OUT)
    start = (rt.rigid(5e-3, (0.3, 0.8, -0.52), vs * np.array([0.6, -0.64, 0.48]), (0.0, 0.0, 2.0)) @ M_true.astype(np.float64)).astype(np.float32)
    D = rt.rigid(0.12, (0.42, -0.61, 0.67), (0.05, -0.03, 0.04)).astype(np.float32)
    E = rt.rigid(-0.07, (0.1, 0.9, 0.2), (-0.02, 0.01, 0.03)).astype(np.float32)
    n = len(frames)
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n + 1))
        for a, b, M in frames + [(rgba, mm, start)]:
            f.write(a.tobytes()); f.write(b.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        f.write(pkg.mat_to_abi(D).tobytes()); f.write(pkg.mat_to_abi(E).tobytes())
    run = subprocess.run([HARNESS, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    T = [np.frombuffer(raw, np.float32, 16, 64 * k) for k in range(3)]
    before, after = (np.frombuffer(raw, np.float32, 16, 192 + 64 * k) for k in range(2))
    fused = np.frombuffer(raw, np.float32, 16 * 2 * n, 320).reshape(2, n, 4, 4).transpose(0, 1, 3, 2)
    tail = 320 + 64 * 2 * n
    assert len(raw) == tail + 36
    res_h = pkg.TrackSdfResult.from_buffer_copy(raw[tail:tail + 32])
    tracked, = struct.unpack_from("<i", raw, tail + 32)
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
    W0 = np.array(_rigid_product(_as_doubles(before), _as_doubles(T[2])), np.float64).astype(np.float32).reshape(4, 4).T
    M, res = gpu.track_camera_sdf(view, made, [t.reshape(4, 4).T for t in T], W0, wl.intr)
    print(f"mirror: {run.stdout.strip()}; C ABI: stop {res.stop_reason} after {res.evaluations} evaluations, levels {res.levels_stepped}")
    assert bytes(res) == bytes(res_h) and tracked == 1 and res.levels_stepped == 3
    want = _rigid_product(_as_doubles(pkg.mat_to_abi(M)), _rigid_inverse(_as_doubles(T[2])))
    assert np.array(want, np.float64).astype(np.float32).tobytes() == after.tobytes()
    assert after.tobytes() != before.tobytes()
    # and the camera moved towards the frame's true pose
    corners = seen_corners(gpu.download_view_depth(view), wl.intr, M_true, vs)
    assert rt.pose_distance(M, M_true, corners, vs) < rt.pose_distance(W0, M_true, corners, vs)
