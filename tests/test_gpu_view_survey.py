"""dslam_survey_views and dslam_select_view_maps on the MI355X against ref_view_survey.py: counts,
nearest and farthest depth are integers, so every comparison is for equality.  The fixture set with blocks placed against
the reference's own plane values, the table shapes at which the walk can go wrong, one launch whatever N, read-only-ness,
repeatability and the asynchronous engine, every rejection, and what the survey is for: the tracker's sums and the
composite's images are the same bits on the surveyed list as on the full one."""
import ctypes as C

import numpy as np
import pytest

import analytic_maps as am
import ref_view_survey as rv
import track_sdf_fixtures as tf
import util
import view_survey_fixtures as vf

pytestmark = pytest.mark.gpu

I4 = vf.I4


def upload_map(api, pkg, m):
    scene = api.create_scene(m.scene_params(pkg))
    am.upload(api, scene, m)
    return scene


def upload_table(api, pkg, raw):
    """A scene that holds the hand-made table `raw` (view_survey_fixtures.RawTable): the table alone, pools untouched."""
    scene = api.create_scene(raw.scene_params(pkg))
    api.upload_scene_state(scene, raw.hash)
    return scene


def abi_views(pkg, views):
    return [pkg.SurveyView.of(v.M, v.intr, v.width, v.height, float(v.near_m), float(v.far_m)) for v in views]


def check_survey(pkg, gpu, what, tables, handles, T, views, margin=0.0, vs=vf.VS):
    """One survey against the reference, exactly.  Returns the reference's (live, reach, nearest, farthest)."""
    T = np.asarray(T, np.float32)
    got = gpu.survey_views(handles, T, abi_views(pkg, views), pkg.ViewSurveyParams(margin) if margin else None)
    want = rv.survey(tables, T, vs, views, margin)
    small = len(handles) <= 8
    print(f"{what}: live {got[0].tolist() if small else '...'}, reach {got[1].tolist() if small else got[1].sum(axis=1).tolist()}")
    for name, g, w in zip(("live", "reach", "nearest", "farthest"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, name, g, w)
    return want


@pytest.fixture(scope="module")
def fixture_scenes(pkg, gpu):
    fs = vf.fixture_set()
    return fs, [upload_map(gpu, pkg, m) for m in fs.maps]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the fixture set
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_set(pkg, gpu, fixture_scenes):
    fs, handles = fixture_scenes
    assert len(fs.maps) == 5 and len(fs.views) == 3 and np.array_equal(fs.T[1], I4) and fs.views[1].far_m == 0
    assert sum(np.array_equal(t, I4) for t in fs.T) == 1
    # of the fixture: the reference separates the two blocks of every boundary pair, and every plane of every view has one
    rho = rv.rho_of(0.0)
    planes = [rv.frustum_planes(v, vf.VS) for v in fs.views]
    covered = set()
    for i, v, k, b_in, b_out in fs.notes["boundary"]:
        p = rv.world_points(np.array([b_in, b_out]), fs.T[i], vf.VS)
        s = rv.plane_values(planes[v], p)[0]
        assert -rho <= s[0, k] < -rho + np.float32(0.25) and -rho - np.float32(0.25) < s[1, k] < -rho
        assert rv.reaching(planes[v], p, rho)[0].tolist() == [True, False]
        covered.add((v, k))
    assert covered == {(v, k) for v in range(3) for k in range(6)} - {(1, 5)}, covered
    assert {i for i, *_ in fs.notes["boundary"]} == set(range(5))
    for m in fs.maps:
        assert m.max_chain >= 3 and np.abs(m.block_pos).max() == 32768
    # ... and some reaching block lives in the excess area of every map
    for m, t in zip(fs.maps, fs.T):
        e = m.hash[m.num_buckets:]
        e = e[e["ptr"] >= 0]
        assert rv.reaching(planes[0], rv.world_points(e["pos"], t, vf.VS), rho)[0].any()
    # the entry made non-resident would reach: with it the reference counts one more, and the library does not count it
    i, entry = fs.notes["not_resident"]
    assert fs.maps[i].hash["ptr"][entry] == -1
    live, reach, nearest, farthest = check_survey(pkg, gpu, "fixture set", fs.tables, handles, fs.T, fs.views)
    with_it = fs.maps[i].hash.copy()
    with_it["ptr"][entry] = 5
    full = rv.survey([with_it], fs.T[i:i + 1], vf.VS, fs.views)
    assert full[0][0] == live[i] + 1 and full[1][0, 0] == reach[0, i] + 1
    assert (reach > 0).all() and (reach < live[None]).all()
    # a margin of its own, and nearest_out / farthest_out left out
    check_survey(pkg, gpu, "fixture set, margin 0.5", fs.tables, handles, fs.T, fs.views, margin=0.5)
    n, nv = 5, 3
    ptrs = (C.c_void_p * n)(*[s.ptr for s in handles])
    t_abi = np.ascontiguousarray(np.transpose(fs.T, (0, 2, 1))).reshape(-1)
    varr = (pkg.SurveyView * nv)(*abi_views(pkg, fs.views))
    live2, reach2 = np.zeros(n, np.int32), np.zeros((nv, n), np.int32)
    i32 = C.POINTER(C.c_int32)
    gpu._call("survey_views", gpu._engine, ptrs, t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(n), varr, C.c_int(nv), None,
              live2.ctypes.data_as(i32), reach2.ctypes.data_as(i32), None, None)
    assert np.array_equal(live2, live) and np.array_equal(reach2, reach)


# ---------------------------------------------------------------------------------------------------------------------
# 2. table shapes: the smallest at which the walk can go wrong
# ---------------------------------------------------------------------------------------------------------------------
def test_table_shapes(pkg, gpu, fixture_scenes):
    fs, handles = fixture_scenes
    views = vf.views3()
    # a table smaller than one tile of the walk; a map all of whose blocks reach; N = 1, V = 1
    inside = vf.blocks_map(vf.in_front(views[0], 40, 1))
    assert len(inside.hash) < 8192
    h_inside = upload_map(gpu, pkg, inside)
    live, reach, _, _ = check_survey(pkg, gpu, "all blocks reach", [inside.hash], [h_inside], [I4], views[:1])
    assert live.tolist() == [40] and reach.tolist() == [[40]]
    # 0x8000 + 0x1000 entries: two bit tiles, the second one short; entries at the tiles' ends and an empty stretch between
    raw = vf.two_tile_table()
    resident = np.flatnonzero(raw.hash["ptr"] >= 0)
    assert len(raw.hash) == 0x9000 and {0, 32767, 32768, 0x9000 - 1} <= set(resident.tolist())
    assert not ((resident > 8191) & (resident < 32767)).any()
    h_raw = upload_table(gpu, pkg, raw)
    live, reach, _, _ = check_survey(pkg, gpu, "two bit tiles", [raw.hash], [h_raw], [I4], views[:1])
    assert live.tolist() == [11] and reach.tolist() == [[9]]
    # an empty map, between two others
    empty = gpu.create_scene(inside.scene_params(pkg))
    empty_table = gpu.download_hash_table(empty)
    assert not (empty_table["ptr"] >= 0).any()
    live, reach, nearest, farthest = check_survey(pkg, gpu, "an empty map", [raw.hash, empty_table, inside.hash],
                                                  [h_raw, empty, h_inside], [I4, I4, I4], views)
    assert live[1] == 0 and not reach[:, 1].any() and (nearest[:, 1] == rv.INT32_MAX).all() and (farthest[:, 1] == rv.INT32_MIN).all()
    # the empty map alone, straight after: nothing of the call before is left in the result arrays
    check_survey(pkg, gpu, "nothing", [empty_table], [empty], [I4], views[:2])
    # one map with at least 95 % of all resident blocks
    big = vf.blocks_map(np.concatenate([vf.in_front(views[0], 700, 2), vf.lattice((60, -50, 40), 6)]), num_buckets=0x200)
    h_big = upload_map(gpu, pkg, big)
    tables, hs = [fs.tables[0], big.hash, fs.tables[3]], [handles[0], h_big, handles[3]]
    live, reach, _, _ = check_survey(pkg, gpu, "one large map", tables, hs, fs.T[[0, 1, 3]], views)
    assert live[1] >= 0.95 * live.sum() - 1 and live[1] > 2800
    assert 700 <= reach[0, 1] < live[1]


def test_seventy_maps_sixteen_views(pkg, gpu):
    """More maps than DSLAM_MAX_RENDER_MAPS and than most workgroups see, each of a few blocks, against the most views."""
    n, nv = 70, pkg.MAX_SURVEY_VIEWS
    assert n > pkg.MAX_RENDER_MAPS
    base = vf.views3()[0]
    rng = np.random.default_rng(70)
    maps = [vf.blocks_map(np.concatenate([vf.in_front(base, 3 + i % 4, 300 + i), [[0, 0, -200 - i]]])) for i in range(n)]
    T = np.stack([I4 if i == 7 else vf.rigid(rng, 0.3) for i in range(n)])
    views = []
    for k in range(nv):
        D = vf.rigid(rng, 0.2).astype(np.float64)
        D[:3, :3] = np.eye(3) if k == 0 else D[:3, :3]
        M = (np.linalg.inv(D) @ base.M.astype(np.float64) if k % 2 else base.M.astype(np.float64) @ D).astype(np.float32)
        # (the product of two float32 rotations, rounded: orthonormal to about 1e-7)
        views.append(rv.View(M, base.intr, base.width, base.height, 0.1 + 0.02 * k, 0.0 if k % 5 == 4 else 0.9 + 0.1 * k))
    handles = [upload_map(gpu, pkg, m) for m in maps]
    live, reach, nearest, farthest = check_survey(pkg, gpu, "70 maps, 16 views", [m.hash for m in maps], handles, T, views)
    assert (live == np.array([4 + i % 4 for i in range(n)])).all()
    assert (reach > 0).sum() > n and (reach == 0).any() and len({tuple(r) for r in reach.tolist()}) == nv
    # from the survey to a list the other calls take
    keep, res = gpu.select_view_maps(reach, nearest, pkg.ViewSelectParams(always_keep=69))
    want, counts = rv.select(reach.tolist(), nearest.tolist(), always_keep=69)
    assert keep.tolist() == want and res.as_dict() == counts and res.selected <= pkg.MAX_RENDER_MAPS < res.reaching
    for h in handles:
        h.close()


def test_an_entry_emptied_behind_the_bitmap_is_not_resident(pkg, gpu):
    """The walk follows the scene's bitmap of resident entries, but the law is about the entry: ptr >= 0.  An entry whose
    ptr is set to -1 through the raw device pointer, without dslam_scene_table_changed, keeps its bit -- and is counted
    nowhere, because the kernel looks at the entry it was sent to."""
    view = vf.views3()[0]
    m = vf.blocks_map(vf.in_front(view, 40, 1))
    scene = upload_map(gpu, pkg, m)
    table = m.hash.copy()
    victim = int(np.flatnonzero(table["ptr"] >= 0)[7])
    table["ptr"][victim] = -1
    gpu.synchronize()
    gpu.lib.dslam_scene_hash_table_dev.restype = C.c_void_p
    base = gpu.lib.dslam_scene_hash_table_dev(scene.ptr)
    gone = C.c_int32(-1)
    hip_memcpy = gpu.lib.hipMemcpy          # (the HIP runtime the library is bound to)
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip_memcpy(C.c_void_p(base + 16 * victim + 12), C.byref(gone), 4, 1) == 0      # hipMemcpyHostToDevice
    assert np.array_equal(gpu.download_hash_table(scene), table)
    live, reach, _, _ = check_survey(pkg, gpu, "one entry emptied behind the bitmap", [table], [scene], [I4], [view])
    assert live.tolist() == [39] and reach.tolist() == [[39]]


# ---------------------------------------------------------------------------------------------------------------------
# 3. one launch whatever N
# ---------------------------------------------------------------------------------------------------------------------
def test_one_launch(pkg, gpu):
    views = vf.views3()
    m = vf.blocks_map(vf.in_front(views[0], 5, 9))
    handles = [upload_map(gpu, pkg, m) for _ in range(70)]
    T = np.stack([I4] * 70)
    deltas = []
    for n in (2, 70):
        before = gpu.debug_stream_launches(), gpu.debug_survey_views_launches()
        gpu.survey_views(handles[:n], T[:n], abi_views(pkg, views))
        deltas.append((gpu.debug_stream_launches() - before[0], gpu.debug_survey_views_launches() - before[1]))
    print(f"launches across a call, N = 2 and N = 70: {deltas}")
    # dslam_debug_stream_launches counts fusion launches only: the survey adds none; its own counter says one kernel each
    assert deltas[0] == deltas[1] == (0, 1)
    for h in handles:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. read-only, repeatable, asynchronous
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    fs = vf.fixture_set()
    handles = [upload_map(gpu, pkg, m) for m in fs.maps[:3]]
    before = [util.snapshot(gpu, s) for s in handles]
    T = fs.T[:3]
    views = abi_views(pkg, fs.views)

    def run(hs=handles, Ts=T, vs_=views):
        return tuple(a.tobytes() for a in gpu.survey_views(hs, Ts, vs_))

    first, second = run(), run()
    assert first == second
    assert first == tuple(a.astype(np.int32).tobytes() for a in rv.survey(fs.tables[:3], T, vf.VS, fs.views))
    for s, snap, what in zip(handles, before, ("map 0", "map 1", "map 2")):
        util.assert_same_state(snap, util.snapshot(gpu, s), what)
        assert snap["stats"] == gpu.stats(s), what
    # an asynchronous engine with a fusion in flight on one of the surveyed scenes: the survey sees the state after it
    wl = synth.s_tiny()
    fused = gpu.create_scene(util.small_params(pkg, wl))
    rs = gpu.create_render_state(fused, wl.W, wl.H)
    view = gpu.create_view(wl.W, wl.H)
    cam = [pkg.SurveyView.of(wl.frame(2)[2], wl.intr, wl.W, wl.H, 0.1, 0.0)]
    ref_cam = [rv.View(wl.frame(2)[2], wl.intr, wl.W, wl.H, 0.1, 0.0)]
    vs = fused.params.voxel_size
    try:
        gpu.set_async(True)
        for i in range(3):
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(fused, view, rs, M, wl.intr)
        third = gpu.survey_views([fused], [I4], cam)
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    table = gpu.download_hash_table(fused)
    want = rv.survey([table], [I4], vs, ref_cam)
    print(f"asynchronous: {third[0].tolist()} live blocks after three frames in flight, {third[1].tolist()} reach the last camera")
    assert third[0][0] > 100 and third[1][0, 0] > 50
    for g, w in zip(third, want):
        assert np.array_equal(g, w)
    again = gpu.survey_views([fused], [I4], cam)
    assert all(np.array_equal(a, b) for a, b in zip(third, again))


# ---------------------------------------------------------------------------------------------------------------------
# 5. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_outputs_untouched(pkg, gpu, fixture_scenes):
    fs, good = fixture_scenes
    good, start = good[:3], fs.T[:3]
    other_vs = gpu.create_scene(fs.maps[2].scene_params(pkg, voxel_size=0.006))
    other_mu = gpu.create_scene(fs.maps[2].scene_params(pkg, mu=0.03))
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = second.create_scene(fs.maps[2].scene_params(pkg))
    i32 = C.POINTER(C.c_int32)
    views = fs.views

    def call(handles=good, T0=start, vws=views, n_maps=None, n_views=None, margin=None, null=()):
        n, nv = len(handles), len(vws)
        t_abi = np.ascontiguousarray(np.transpose(np.asarray(T0, np.float32), (0, 2, 1))).reshape(-1).copy()
        ptrs = (C.c_void_p * n)(*[None if s is None else s.ptr for s in handles])
        varr = (pkg.SurveyView * nv)(*abi_views(pkg, vws))
        params = None if margin is None else pkg.ViewSurveyParams(margin)
        outs = [np.full(n, -7, np.int32)] + [np.full((nv, n), -7, np.int32) for _ in range(3)]
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("survey_views", gpu._engine, None if "scenes" in null else ptrs,
                      None if "T" in null else t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(n if n_maps is None else n_maps),
                      None if "views" in null else varr, C.c_int(nv if n_views is None else n_views),
                      C.byref(params) if params is not None else None,
                      None if "live" in null else outs[0].ctypes.data_as(i32), None if "reach" in null else outs[1].ctypes.data_as(i32),
                      outs[2].ctypes.data_as(i32), outs[3].ctypes.data_as(i32))
        assert all((o == -7).all() for o in outs)

    def view_with(**kw):
        v = fs.views[0]
        v = rv.View(v.M.copy(), v.intr.copy(), v.width, v.height, v.near_m, v.far_m)
        for k, val in kw.items():
            setattr(v, k, val)
        return [views[1], v]

    for what in ("scenes", "T", "views", "live", "reach"):
        call(null=(what,))
    call(handles=[good[0], None, good[2]])
    call(n_maps=0)
    call(n_maps=pkg.MAX_SURVEY_MAPS + 1)
    call(n_views=0)
    call(n_views=pkg.MAX_SURVEY_VIEWS + 1)
    call(handles=[good[0], good[1], good[0]])
    call(handles=[good[0], good[1], foreign])
    call(handles=[good[0], good[1], other_vs])
    call(handles=[good[0], good[1], other_mu])
    nan, inf, skew = start.copy(), start.copy(), start.copy()
    nan[1, 1, 3] = np.nan
    inf[2, 0, 3] = np.inf
    skew[2, :3, :3] *= 1.001
    call(T0=nan)
    call(T0=inf)
    call(T0=skew)
    M_nan, M_skew = fs.views[0].M.copy(), fs.views[0].M.copy()
    M_nan[0, 3] = np.nan
    M_skew[:3, :3] *= 1.001
    intr_inf, intr_fx, intr_fy = (fs.views[0].intr.copy() for _ in range(3))
    intr_inf[3], intr_fx[0], intr_fy[1] = np.inf, 0.0, -1.0
    for bad in (dict(M=M_nan), dict(M=M_skew), dict(intr=intr_inf), dict(intr=intr_fx), dict(intr=intr_fy), dict(width=0), dict(height=0),
                dict(near_m=np.float32(-0.1)), dict(far_m=np.float32(-1.0)), dict(near_m=np.float32(np.nan)),
                dict(near_m=np.float32(0.6), far_m=np.float32(0.6)), dict(near_m=np.float32(0.6), far_m=np.float32(0.3))):
        call(vws=view_with(**bad))
    call(margin=-0.5)
    call(margin=float("nan"))
    call(margin=float("inf"))
    # ... and the engine still answers
    assert gpu.survey_views(good, start, abi_views(pkg, views))[0].tolist() == [int((t["ptr"] >= 0).sum()) for t in fs.tables[:3]]


# ---------------------------------------------------------------------------------------------------------------------
# 6. / 7. what the survey is for: the surveyed list gives the full list's bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def four_maps(pkg, gpu):
    """The two ramp-sphere maps of track_sdf_fixtures.py and two maps that cannot be reached from its camera -- one behind
    it, one 40 blocks to the side -- in the list order [A, behind, B, to the side]; the fixture's view at its start pose."""
    f = tf.ramp_spheres()
    behind = vf.blocks_map(vf.lattice((0, 0, -28), 2))
    aside = vf.blocks_map(vf.lattice((40, 0, 11), 2))
    scenes = [upload_map(gpu, pkg, m) for m in (f.maps[0], behind, f.maps[1], aside)]
    T = np.stack([f.T[0], vf.I4, f.T[1], vf.I4])
    view = gpu.create_view(f.w, f.h)
    gpu.view_update(view, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
    start = f.start()
    assert f.depth0.max() < 3.0
    cam = pkg.SurveyView.of(start, f.intr, f.w, f.h, 0.05, 3.0)
    live, reach, nearest, farthest = gpu.survey_views(scenes, T, [cam])
    keep, res = gpu.select_view_maps(reach, nearest, pkg.ViewSelectParams(always_keep=0))
    print(f"survey at the start pose: live {live.tolist()}, reach {reach.tolist()}, nearest {nearest.tolist()}; kept {keep.tolist()}")
    assert live.tolist() == [len(f.maps[0].block_pos), 125, len(f.maps[1].block_pos), 125]
    assert reach[0, 1] == 0 and reach[0, 3] == 0 and reach[0, 0] > 0 and reach[0, 2] > 0
    assert keep.tolist() == [0, 2] and (res.reaching, res.selected) == (2, 2)
    return f, scenes, T, view, start, keep.tolist()


def test_tracker_identity(pkg, gpu, four_maps):
    f, scenes, T, view, start, keep = four_maps
    sub, T_sub = [scenes[i] for i in keep], T[keep]
    one = pkg.TrackSdfParams(no_hierarchy_levels=1, run_till_level=0, max_evaluations=1)
    results = []
    for hs, Ts in ((scenes, T), (sub, T_sub)):
        M, res = gpu.track_camera_sdf(view, hs, Ts, start, f.intr, one)
        results.append((M.tobytes(), bytes(res), gpu.debug_track_sdf_sums().tobytes()))
        assert res.valid_last > 100
    assert results[0] == results[1], "one evaluation: the 33 sums differ between the full and the surveyed list"
    for params in (None, pkg.TrackSdfParams(**tf.RUN_PARAMS)):
        runs = []
        for hs, Ts in ((scenes, T), (sub, T_sub)):
            M, res = gpu.track_camera_sdf(view, hs, Ts, start, f.intr, params)
            runs.append((M.tobytes(), bytes(res)))
        print(f"whole run: stop {res.stop_reason} after {res.evaluations} evaluations, levels {res.levels_stepped}")
        assert runs[0] == runs[1] and res.evaluations > 3 and runs[0][0] != start.tobytes()


def test_composite_identity(pkg, gpu, four_maps):
    f, scenes, T, view, start, keep = four_maps
    sub, T_sub = [scenes[i] for i in keep], T[keep]
    rs = gpu.create_render_state(max(scenes, key=lambda s: s.params.num_local_blocks), f.w, f.h)
    for kind in (pkg.IMAGE_DEPTH, pkg.IMAGE_SHADED):
        full = gpu.get_image_multi(scenes, T, rs, start, f.intr, kind).copy()
        part = gpu.get_image_multi(sub, T_sub, rs, start, f.intr, kind).copy()
        assert full.tobytes() == part.tobytes(), kind
        assert np.count_nonzero(full) > 1000


# ---------------------------------------------------------------------------------------------------------------------
# 8. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
KEYFRAMES, HELD_OUT = (40, 44, 48), 47       # S-tiny frames (as test_gpu_track_sdf.py)


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


def test_mirror_survey_and_track_visible_local_maps(pkg, gpu, synth, tmp_path):
    """view_survey_harness: two local maps fused from S-tiny keyframes, a third fused in the first one's frame whose
    estimatedGlobalPose then moves its content 30 m away, and a current local map that holds nothing.  SurveyLocalMapsInView gives
    the C ABI's bytes on the same maps re-fused through the C ABI; TrackVisibleLocalMaps lists maps 0, 1 and the current
    one and leaves pose_d exactly where TrackAllLocalMaps leaves it, which is where dslam_track_camera_sdf puts the camera."""
    import os
    import struct
    import subprocess

    import ref64_track_sdf as rt

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    harness = os.path.join(root, "denseslam-global-consistency-h_amd", "itmlib", "tests", "view_survey_harness")
    wl = synth.s_tiny(80, 60)
    p = util.small_params(pkg, wl)
    vs = p.voxel_size
    frames = [wl.frame(i) for i in KEYFRAMES]
    rgba, mm, M_true = wl.frame(HELD_OUT)
    start = (rt.rigid(5e-3, (0.3, 0.8, -0.52), vs * np.array([0.6, -0.64, 0.48]), (0.0, 0.0, 2.0)) @ M_true.astype(np.float64)).astype(np.float32)
    D = rt.rigid(0.12, (0.42, -0.61, 0.67), (0.05, -0.03, 0.04)).astype(np.float32)
    E = rt.rigid(-0.07, (0.1, 0.9, 0.2), (-0.02, 0.01, 0.03)).astype(np.float32)
    F = rt.rigid(0.3, (0.2, -0.5, 0.84), (30.0, 2.0, -1.0)).astype(np.float32)
    near_m, far_m = 0.0, 12.0       # every depth pixel is covered, and what lies 30 m away is beyond the far plane
    assert 0 < mm.max() * 1e-3 <= far_m
    n, n_maps = len(frames), 4
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n + 1))
        for a, b, M in frames + [(rgba, mm, start)]:
            f.write(a.tobytes()); f.write(b.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        for X in (D, E, F):
            f.write(pkg.mat_to_abi(X).tobytes())
        f.write(struct.pack("<2f", near_m, far_m))
    run = subprocess.run([harness, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    at = 0

    def take(count, dtype=np.float32):
        nonlocal at
        a = np.frombuffer(raw, dtype, count, at)
        at += a.nbytes
        return a

    T = take(16 * n_maps).reshape(n_maps, 4, 4).transpose(0, 2, 1)
    before, after_all, after_vis = take(16), take(16), take(16)
    fused = take(16 * 3 * n).reshape(3, n, 4, 4).transpose(0, 1, 3, 2)
    W0 = take(16)
    reach_h, nearest_h = take(n_maps, np.int32), take(n_maps, np.int32)
    kept_count, = take(1, np.int32)
    kept = take(4, np.int32)[:kept_count]
    res_all = pkg.TrackSdfResult.from_buffer_copy(raw[at:at + 32]); at += 32
    res_vis = pkg.TrackSdfResult.from_buffer_copy(raw[at:at + 32]); at += 32
    tracked_all, tracked_vis = take(2, np.int32)
    kept_img = take(5, np.int32)
    kept_none = take(5, np.int32)
    img_all, img_vis, img_none = (take(wl.W * wl.H).reshape(wl.H, wl.W) for _ in range(3))
    assert at == len(raw)
    print(f"mirror: {run.stdout.strip()}")
    # the same maps through the C ABI
    view = gpu.create_view(wl.W, wl.H)
    made = []
    for k in range(3):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (a, b, _) in enumerate(frames):
            gpu.view_update(view, a, b, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    made.append(gpu.create_scene(p))
    gpu.view_update(view, rgba, mm, timestamp=float(n))
    assert np.array(_rigid_product(_as_doubles(before), _as_doubles(pkg.mat_to_abi(T[3]))), np.float64).astype(np.float32).tobytes() == W0.tobytes()
    W0m = W0.reshape(4, 4).T
    live, reach, nearest, _ = gpu.survey_views(made, T, [pkg.SurveyView.of(W0m, wl.intr, wl.W, wl.H, near_m, far_m)])
    assert reach[0].tobytes() == reach_h.tobytes() and nearest[0].tobytes() == nearest_h.tobytes()
    assert reach[0, 0] > 0 and reach[0, 1] > 0 and reach[0, 2] == 0 and reach[0, 3] == 0 and live[2] > 0 and live[3] == 0
    keep, _ = gpu.select_view_maps(reach, nearest, pkg.ViewSelectParams(always_keep=3))
    assert keep.tolist() == kept.tolist() == [0, 1, 3]
    # TrackVisibleLocalMaps is TrackAllLocalMaps ...
    assert after_vis.tobytes() == after_all.tobytes() != before.tobytes()
    assert bytes(res_vis) == bytes(res_all) and tracked_all == tracked_vis == 1
    # ... which is dslam_track_camera_sdf, on either list
    for pick in (list(range(4)), keep.tolist()):
        M, res = gpu.track_camera_sdf(view, [made[i] for i in pick], T[pick], W0m, wl.intr)
        assert bytes(res) == bytes(res_all)
        want = _rigid_product(_as_doubles(pkg.mat_to_abi(M)), _rigid_inverse(_as_doubles(pkg.mat_to_abi(T[3]))))
        assert np.array(want, np.float64).astype(np.float32).tobytes() == after_all.tobytes()
    # GetImageVisibleLocalMaps draws the sub-list the survey leaves: maps 0 and 1 from the start (the empty current map
    # reaches nothing and is not kept here), and map 0 when nothing reaches
    keep_img, _ = gpu.select_view_maps(reach, nearest)
    assert kept_img[1:1 + kept_img[0]].tolist() == keep_img.tolist() == [0, 1] and kept_none[:2].tolist() == [1, 0]
    rs = gpu.create_render_state(made[0], wl.W, wl.H)
    for pick, pose, img in ((list(range(4)), W0m, img_all), ([0, 1], W0m, img_vis)):
        want = gpu.get_image_multi([made[i] for i in pick], T[pick], rs, pose, wl.intr, pkg.IMAGE_DEPTH)
        assert want.tobytes() == img.tobytes(), pick
    assert np.count_nonzero(img_vis) > 1000
    print(f"depth pixels that differ between GetImageAllLocalMaps and GetImageVisibleLocalMaps: {int((img_all.view(np.uint32) != img_vis.view(np.uint32)).sum())}")
    W_far = W0m.copy()
    W_far[2, 3] += np.float32(1000.0)
    far_reach = gpu.survey_views(made, T, [pkg.SurveyView.of(W_far, wl.intr, wl.W, wl.H, near_m, far_m)])[1]
    assert not far_reach.any()
    assert gpu.get_image_multi([made[0]], T[:1], rs, W_far, wl.intr, pkg.IMAGE_DEPTH).tobytes() == img_none.tobytes()
