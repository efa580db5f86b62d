"""dslam_register_graph on the MI355X against the float64 reference of ref64_register_graph.py: one joint evaluation sum by
sum within the derived rounding bound, one pair against the pairwise call bit for bit, the split of the grid over pairs of
very different sizes, whole runs (nested triangle, large variant, ring), stop reason 3, inactive pairs and argument errors,
read-only-ness and repeatability, and the ITMLib mirror (AlignLocalMaps)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_register as rr
import ref64_register_graph as rg
import register_fixtures as fx
import register_graph_fixtures as gf
import util

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "register_graph_harness")


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


@pytest.fixture(scope="module")
def scenes(pkg, gpu):
    """Uploaded fixture maps, one scene per (map, copy), shared by the tests of this file (none of them writes a map)."""
    cache = {}

    def get(m, copy=0):
        if (id(m), copy) not in cache:
            cache[(id(m), copy)] = (m, upload_map(gpu, pkg, m))
        return cache[(id(m), copy)][1]

    return get


def pair_transforms(T, pairs, vs):
    """X~_p (float64, not yet rounded) of every pair at the poses T [N, 4, 4] float32, as the law composes them."""
    Tt = np.stack([rr.voxel_transform(np.asarray(t, np.float32).astype(np.float64), vs) for t in T])
    return [rg.pair_transform(Tt, s, d) for s, d in pairs]


def check_joint_evaluation(pkg, gpu, what, data, handles, T0, pairs, anchor):
    """One joint evaluation (max_evaluations = 1): every pair's 33 sums, the pair results and the joint cost against
    ref64_register.evaluate at the stated X~_p.  Returns (reference evaluations, result, pair results)."""
    T0 = np.asarray(T0, np.float32)
    T, res, pres = gpu.register_graph(handles, T0, pairs, anchor, pkg.RegisterParams(max_evaluations=1))
    evs = [rr.evaluate(data[s], data[d], X) for (s, d), X in zip(pairs, pair_transforms(T0, pairs, data[0].vs))]
    active = {}
    for p, (ev, pr) in enumerate(zip(evs, pres)):
        sums = gpu.debug_register_graph_sums(p)
        used = ev.check_sums(sums, f"{what}, pair {pairs[p]}")
        lo, hi = ev.cost_interval()
        print(f"{what}, pair {pairs[p]}: {ev.candidates} candidates, {ev.valid} valid, {ev.ties} ties; the sums use up to "
              f"{used:.3f} of the bound; cost {pr.cost_first:.6g} in [{lo:.6g}, {hi:.6g}]")
        assert pr.candidates == ev.candidates and abs(pr.valid_first - ev.valid) <= ev.ties
        assert pr.valid_last == pr.valid_first and lo <= pr.cost_first <= hi and pr.cost_last == pr.cost_first
        assert abs(ev.valid - 500) > ev.ties   # (whether the pair is active does not hang on a tie)
        assert pr.active == int(ev.valid >= 500)
        if pr.active:
            active[p] = ev
    je = rg.JointEvaluation(active, {}, evs[0].gate)
    lo, hi = je.cost_interval()
    assert lo <= res.cost_first <= hi and res.cost_last == res.cost_first, (lo, res.cost_first, hi)
    assert res.evaluations == 1 and res.active_pairs == len(active)
    assert T.tobytes() == T0.tobytes()
    return evs, res, pres


# ---------------------------------------------------------------------------------------------------------------------
# 1. one joint evaluation
# ---------------------------------------------------------------------------------------------------------------------
def test_single_joint_evaluation_against_the_reference(pkg, gpu, scenes):
    ms = gf.map_set("small")
    handles = [scenes(m) for m in ms.maps]
    evs, res, _ = check_joint_evaluation(pkg, gpu, "nested triangle", ms.data, handles, gf.off_lattice_starts(), gf.TRIANGLE, 0)
    assert res.stop_reason == 1 and res.active_pairs == 3 and res.conditioning > 0.05
    assert all(ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates for ev in evs)
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu.debug_register_graph_sums(3)


# ---------------------------------------------------------------------------------------------------------------------
# 2. one pair is the pairwise call
# ---------------------------------------------------------------------------------------------------------------------
def test_one_pair_equals_the_pairwise_call(pkg, gpu, scenes):
    """Two maps, the pair (0, 1), anchor 0, T_0 the identity: X~ = T~_1 exactly, the free map is the destination, and the
    run is dslam_register_maps(src 0, dst 1, X = T_1) step for step."""
    ms = gf.map_set("small")
    a, b = scenes(ms.maps[0]), scenes(ms.maps[1])
    X, pw = gpu.register_maps(a, b, I4)
    sums_pw = gpu.debug_register_sums()
    T, res, pres = gpu.register_graph([a, b], gf.identity_starts(2), [(0, 1)], 0)
    sums = gpu.debug_register_graph_sums(0)
    print(f"pairwise: {pw.as_dict()}; graph: {res.as_dict()}, {pres[0].as_dict()}")
    assert pw.stop_reason == 0
    assert T[1].tobytes() == X.tobytes() and T[0].tobytes() == I4.tobytes()
    assert (res.evaluations, res.stop_reason) == (pw.evaluations, pw.stop_reason)
    assert (pres[0].candidates, pres[0].valid_last) == (pw.candidates, pw.valid_last)
    for name in ("cost_first", "cost_last"):
        assert np.float32(getattr(res, name)).tobytes() == np.float32(getattr(pw, name)).tobytes(), name
        assert np.float32(getattr(pres[0], name)).tobytes() == np.float32(getattr(pw, name)).tobytes(), name
    assert abs(res.conditioning - pw.conditioning) <= 1e-6 * pw.conditioning
    assert sums.tobytes() == sums_pw.tobytes()
    assert res.active_pairs == 1 and pres[0].active == 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. the split of the grid
# ---------------------------------------------------------------------------------------------------------------------
def test_work_split(pkg, gpu, scenes):
    """Sources of 585 and of 5 live blocks in one call (the small one's range has as many workgroups as blocks, the large
    one's fewer workgroups than blocks), then the 5-block pair alone on the same engine (507 idle workgroups must write
    zeros over the rows of the call before), then a source without a resident block."""
    big, box = fx.sphere_pair(), fx.box_pair("small")
    few = gf.few_map()
    assert len(big.dst_map.block_pos) == 585 and len(few.block_pos) == 5
    data = [big.dst, big.dst, rr.MapData.of_map(few), box.dst]
    handles = [scenes(big.dst_map), scenes(big.dst_map, 1), scenes(few), scenes(box.dst_map)]
    T0 = np.stack([I4, fx.off_lattice(1.5, 0.45), I4, fx.off_lattice()])
    evs, res, pres = check_joint_evaluation(pkg, gpu, "585 + 5 blocks", data, handles, T0, [(0, 1), (2, 3)], 0)
    assert evs[0].valid > 500 and evs[1].valid > 500 and [p.active for p in pres] == [1, 1]
    assert res.stop_reason == 3           # (no pair joins maps 2 and 3 to the anchor)
    check_joint_evaluation(pkg, gpu, "5 blocks alone", data[2:], handles[2:], T0[2:], [(0, 1)], 0)
    empty = gpu.create_scene(few.scene_params(pkg))
    T, res, pres = gpu.register_graph([empty, handles[3]], T0[2:], [(0, 1)], 0, pkg.RegisterParams(max_evaluations=1))
    assert not np.any(gpu.debug_register_graph_sums(0))
    assert (pres[0].candidates, pres[0].valid_first, pres[0].active) == (0, 0, 0)
    assert res.stop_reason == 3 and res.active_pairs == 0 and res.conditioning == 0.0 and T.tobytes() == T0[2:].tobytes()
    assert abs(res.cost_first - 0.5625) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. whole runs (the ring: free maps are sources, so its steps hang on the source-side Jacobian)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["triangle", "large", "ring"])
def test_whole_run_against_the_reference(pkg, gpu, scenes, case):
    name, pairs, anchor = gf.CASES[case]
    ms, T_ref, ref = gf.reference_run(case)
    handles = [scenes(m) for m in ms.maps]
    T, res, pres = gpu.register_graph(handles, gf.identity_starts(), pairs, anchor)
    free = [i for i in range(3) if i != anchor]
    # a decision whose cost difference is below the rounding bound of the two costs may fall either way in float32
    tie_at = next((k for k, t in enumerate(ref["trace"]) if k > 0 and t["margin"] < t["cost_slack"]), None)
    print(f"{case}: reference {ref['evaluations']} evaluations (stop {ref['stop_reason']}), engine {res.evaluations} (stop "
          f"{res.stop_reason}); first decision within the bound: evaluation {tie_at}; conditioning {res.conditioning:.4g} / "
          f"{ref['conditioning']:.4g}; cost {res.cost_first:.4g} -> {res.cost_last:.4g}")
    assert T[anchor].tobytes() == I4.tobytes()
    d_refs = {}
    for i in free:
        # (poses relative to the anchor: with anchor 0 this is the distance of T_i to map i's true pose)
        d_ref, d_gpu = ms.pair_distance(T_ref, anchor, i), ms.pair_distance(T, anchor, i)
        apart = rr.pose_distance(T[i], T_ref[i], ms.corners, am.VS)
        print(f"  map {i}: distance to the truth {d_ref:.4g} / {d_gpu:.4g} voxel, apart {apart:.4g}")
        assert d_gpu <= 2 * d_ref and apart <= 4 * d_ref
        d_refs[i] = d_ref
    assert [p.candidates for p in pres] == [p["candidates"] for p in ref["pairs"]]
    assert res.active_pairs == ref["active_pairs"] == len(pairs)
    if tie_at is None:
        upto, T_cap, cap, T_g, r_g, p_g = ref["evaluations"], T_ref, ref, T, res, pres
    else:
        # compare up to the evaluation before that decision: both runs capped there
        upto = tie_at
        _, T_cap, cap = gf.reference_run(case, max_evaluations=upto)
        T_g, r_g, p_g = gpu.register_graph(handles, gf.identity_starts(), pairs, anchor, pkg.RegisterParams(max_evaluations=upto))
    assert upto >= 3
    assert r_g.evaluations == cap["evaluations"] and r_g.stop_reason == cap["stop_reason"]
    for got, want in zip(p_g, cap["pairs"]):
        assert abs(got.valid_last - want["valid_last"]) <= want["last"].ties
    assert abs(r_g.conditioning - cap["conditioning"]) <= 1e-3 * cap["conditioning"]
    # the same accepted steps: the poses differ by float32 rounding of the sums only
    for i in free:
        assert rr.pose_distance(T_g[i], T_cap[i], ms.corners, am.VS) <= max(4 * d_refs[i], 1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 6. stop reason 3, inactive pairs, rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_unconnected_graphs_and_inactive_pairs(pkg, gpu, scenes):
    ms = gf.map_set("small")
    handles = [scenes(m) for m in ms.maps]
    start = gf.off_lattice_starts()
    T, res, pres = gpu.register_graph(handles, start, [(0, 1)], 0)
    assert res.stop_reason == 3 and res.evaluations == 1 and res.conditioning == 0.0 and res.active_pairs == 1
    assert T.tobytes() == start.tobytes() and pres[0].active == 1 and pres[0].valid_last == pres[0].valid_first
    assert res.cost_last == res.cost_first == pres[0].cost_first
    # connected on paper, but the pair that reaches map 2 is not active
    far = start.copy()
    far[2] = gf.FAR
    T, res, pres = gpu.register_graph(handles, far, [(0, 1), (1, 2)], 0)
    assert res.stop_reason == 3 and T.tobytes() == far.tobytes() and [p.active for p in pres] == [1, 0]
    assert pres[1].valid_first == 0 and pres[1].candidates == 48636 and abs(pres[1].cost_first - 0.5625) < 1e-6
    # map 0 against the sphere, 3 m away: reported, in nothing
    sphere = scenes(fx.sphere_pair().dst_map)
    start4 = np.concatenate([start, gf.FAR[None]])
    T_w, r_w, p_w = gpu.register_graph(handles + [sphere], start4, gf.TRIANGLE + [(0, 3)], 0)
    T_o, r_o, p_o = gpu.register_graph(handles + [sphere], start4, gf.TRIANGLE, 0)
    _, r_3, _ = gpu.register_graph(handles, start, gf.TRIANGLE, 0, pkg.RegisterParams(max_evaluations=1))
    assert (p_w[3].active, p_w[3].valid_first, p_w[3].valid_last, p_w[3].candidates) == (0, 0, 0, 25395)
    assert r_w.stop_reason == 3 and bytes(r_w) == bytes(r_o) and T_w.tobytes() == T_o.tobytes() == start4.tobytes()
    assert [bytes(p) for p in p_w[:3]] == [bytes(p) for p in p_o]
    assert np.float32(r_w.cost_first).tobytes() == np.float32(r_3.cost_first).tobytes()
    # an inactive pair between maps the others connect: the run without it, step for step
    name, pairs, anchor, params = gf.INACTIVE_BETWEEN
    rp = pkg.RegisterParams(**params)
    T_w, r_w, p_w = gpu.register_graph(handles, gf.identity_starts(), pairs, anchor, rp)
    s_w = [gpu.debug_register_graph_sums(p) for p in range(3)]
    T_o, r_o, p_o = gpu.register_graph(handles, gf.identity_starts(), pairs[1:], anchor, rp)
    s_o = [gpu.debug_register_graph_sums(p) for p in range(2)]
    _, ref = rg.register_graph(ms.data, gf.identity_starts(), pairs, anchor, **params)
    print(f"inactive between connected maps: valid at the start {[p.valid_first for p in p_w]}, {r_w.as_dict()}")
    assert [p.active for p in p_w] == [0, 1, 1] and (p_w[0].valid_first, p_w[0].valid_last) == (25395, 25395)
    assert [p.valid_first for p in p_w] == [p["valid_first"] for p in ref["pairs"]]      # (identity starts: no ties)
    assert r_w.evaluations == ref["evaluations"] and r_w.stop_reason == ref["stop_reason"] and r_w.cost_last < r_w.cost_first
    assert T_w.tobytes() == T_o.tobytes() and bytes(r_w) == bytes(r_o) and T_w[anchor].tobytes() == I4.tobytes()
    assert T_w[0].tobytes() != I4.tobytes() and T_w[2].tobytes() != I4.tobytes()
    assert [bytes(p) for p in p_w[1:]] == [bytes(p) for p in p_o]
    assert [s.tobytes() for s in s_w[1:]] == [s.tobytes() for s in s_o]
    # the inactive pair keeps the sums of the first evaluation
    assert s_w[0][28] == 25395 and s_w[0][32] == 25395


def test_invalid_arguments_leave_every_pose_untouched(pkg, gpu, scenes):
    ms = gf.map_set("small")
    good = [scenes(m) for m in ms.maps]
    other_vs = upload_map(gpu, pkg, ms.maps[2], voxel_size=0.006)
    other_mu = upload_map(gpu, pkg, ms.maps[2], mu=0.03)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = upload_map(second, pkg, ms.maps[2])
    start = gf.off_lattice_starts()

    def call(handles=good, T0=start, pairs=gf.TRIANGLE, anchor=0, params=None, n_maps=None, n_pairs=None, null=()):
        t_abi = np.ascontiguousarray(np.transpose(np.asarray(T0, np.float32), (0, 2, 1))).reshape(-1).copy()
        keep = t_abi.copy()
        ptrs = (C.c_void_p * len(handles))(*[None if s is None else s.ptr for s in handles])
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        res = pkg.RegisterGraphResult()
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("register_graph", gpu._engine, None if "scenes" in null else ptrs,
                      None if "T" in null else t_abi.ctypes.data_as(C.POINTER(C.c_float)),
                      C.c_int(len(handles) if n_maps is None else n_maps),
                      None if "pairs" in null else pr.ctypes.data_as(C.POINTER(C.c_int32)),
                      C.c_int(len(pr) if n_pairs is None else n_pairs), C.c_int(anchor),
                      C.byref(params) if params is not None else None, None if "result" in null else C.byref(res), None)
        assert t_abi.tobytes() == keep.tobytes()

    for what in ("scenes", "T", "pairs", "result"):
        call(null=(what,))
    call(handles=[good[0], None, good[2]])
    call(n_maps=1)
    call(n_maps=pkg.MAX_RENDER_MAPS + 1)
    call(n_pairs=0)
    call(n_pairs=pkg.MAX_REGISTER_PAIRS + 1)
    call(anchor=-1)
    call(anchor=3)
    call(pairs=[(0, 1), (0, 3)])
    call(pairs=[(0, 1), (-1, 2)])
    call(pairs=[(0, 1), (2, 2)])
    call(pairs=[(0, 1), (1, 2), (0, 1)])
    call(handles=[good[0], good[1], good[0]])
    call(handles=[good[0], good[1], foreign])
    call(handles=[good[0], good[1], other_vs])
    call(handles=[good[0], good[1], other_mu])
    nan, skew = start.copy(), start.copy()
    nan[1, 1, 3] = np.nan
    skew[2, :3, :3] *= 1.001
    call(T0=nan)
    call(T0=skew)
    for field in ("band", "residual_gate", "max_evaluations", "min_valid", "term_rotation", "term_translation_voxels"):
        call(params=pkg.RegisterParams(**{field: -1}))
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("debug_register_graph_sums", gpu._engine, C.c_int(0), None)
    # both orders of one pair are two pairs; NULL params are the defaults and NULL pair results are allowed
    T, res, _ = gpu.register_graph(good[:2], gf.identity_starts(2), [(0, 1), (1, 0)], 0, pkg.RegisterParams(max_evaluations=2))
    assert res.active_pairs == 2 and res.evaluations == 2
    Td, rd, _ = gpu.register_graph(good, gf.identity_starts(), gf.TRIANGLE, 0, pkg.RegisterParams(0.5, 0.75, 30, 500, 1e-5, 1e-3))
    t_abi = np.ascontiguousarray(np.transpose(gf.identity_starts(), (0, 2, 1))).reshape(-1).copy()
    ptrs = (C.c_void_p * 3)(*[s.ptr for s in good])
    pr = np.asarray(gf.TRIANGLE, np.int32)
    res = pkg.RegisterGraphResult()
    gpu._call("register_graph", gpu._engine, ptrs, t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(3),
              pr.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int(3), C.c_int(0), None, C.byref(res), None)
    assert bytes(res) == bytes(rd) and t_abi.tobytes() == np.ascontiguousarray(np.transpose(Td, (0, 2, 1))).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 7. read-only, repeatable, asynchronous
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    ms = gf.map_set("small")
    handles = [upload_map(gpu, pkg, m) for m in ms.maps]
    before = [util.snapshot(gpu, s) for s in handles]

    def run():
        T, res, pres = gpu.register_graph(handles, gf.identity_starts(), gf.TRIANGLE, 0)
        sums = np.stack([gpu.debug_register_graph_sums(p) for p in range(3)])
        return T.tobytes(), bytes(res), [bytes(p) for p in pres], sums.tobytes(), res

    first, second = run(), run()
    assert first[:4] == second[:4] and first[4].stop_reason == 0
    # an asynchronous engine with work in flight: frames being fused into a fourth scene
    wl = synth.s_tiny()
    other = gpu.create_scene(util.small_params(pkg, wl))
    rs = gpu.create_render_state(other, wl.W, wl.H)
    view = gpu.create_view(wl.W, wl.H)
    try:
        gpu.set_async(True)
        for i in range(3):
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(other, view, rs, M, wl.intr)
        third = run()
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert third[:4] == first[:4]
    for s, snap, what in zip(handles, before, ("map 0", "map 1", "map 2")):
        util.assert_same_state(snap, util.snapshot(gpu, s), what)
        assert snap["stats"] == gpu.stats(s), what


# ---------------------------------------------------------------------------------------------------------------------
# 8. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
MIRROR_FRAMES = dict(W=80, H=60, n_frames=4, stride=4)   # S-tiny keyframes 0, 4, 8, 12 (as test_gpu_register.py)


def test_mirror_align_local_maps_equals_abi(pkg, gpu, synth, tmp_path):
    """register_graph_harness: three local maps of the same keyframes, maps 1 and 2 displaced by D1 (5 mrad / 1 voxel) and
    D2 (4 mrad / 0.8 voxel) without their estimatedGlobalPoses knowing; AlignLocalMaps over the triangle gives the result
    the same call gives through _capi.py on the same maps, re-fused through the C ABI, and writes the poses back only on
    stop reason 0.  (Maps fused from frames mostly end with stop reason 1 or 2, DESIGN.md section 13: the result is held
    to a lower cost and to the reference's distance from the known offsets.)"""
    W, H, n_frames, stride = (MIRROR_FRAMES[k] for k in ("W", "H", "n_frames", "stride"))
    wl = synth.s_tiny(W, H)
    p = util.small_params(pkg, wl)
    vs = p.voxel_size
    D = [np.eye(4, dtype=np.float32),
         rr.rigid(5e-3, fx.AXIS, np.array([0.6, -0.64, 0.48]) * vs).astype(np.float32),
         rr.rigid(-4e-3, gf.AXIS2, 0.8 * vs * gf.DIR2 / np.linalg.norm(gf.DIR2)).astype(np.float32)]
    pairs, anchor = gf.TRIANGLE, 0
    frames = [wl.frame(stride * i) for i in range(n_frames)]
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for rgba, mm, M in frames:
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        f.write(pkg.mat_to_abi(D[1]).tobytes()); f.write(pkg.mat_to_abi(D[2]).tobytes())
        f.write(struct.pack("<2i", len(pairs), anchor))
        f.write(np.asarray(pairs, np.int32).tobytes())
    run = subprocess.run([HARNESS, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    T_before = np.frombuffer(raw, np.float32, 48, 0).reshape(3, 4, 4).transpose(0, 2, 1)
    T_after = np.frombuffer(raw, np.float32, 48, 192).reshape(3, 4, 4).transpose(0, 2, 1)
    fused = np.frombuffer(raw, np.float32, 16 * 3 * n_frames, 384).reshape(3, n_frames, 4, 4).transpose(0, 1, 3, 2)
    tail = 384 + 64 * 3 * n_frames
    assert len(raw) == tail + 24 + 24 * len(pairs) + 4
    res_h = pkg.RegisterGraphResult.from_buffer_copy(raw[tail:tail + 24])
    pres_h = [pkg.RegisterPairResult.from_buffer_copy(raw[tail + 24 + 24 * k:tail + 48 + 24 * k]) for k in range(len(pairs))]
    aligned, = struct.unpack_from("<i", raw, tail + 24 + 24 * len(pairs))
    # the same maps through the C ABI
    made = []
    view = gpu.create_view(wl.W, wl.H)
    for k in range(3):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (rgba, mm, _) in enumerate(frames):
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    T, res, pres = gpu.register_graph(made, T_before, pairs, anchor)
    print(f"mirror: {run.stdout.strip()}; C ABI: {res.as_dict()}")
    assert bytes(res) == bytes(res_h) and [bytes(a) for a in pres] == [bytes(b) for b in pres_h]
    assert T_before[1].tobytes() == T_before[2].tobytes() == T_before[0].tobytes()
    assert aligned == int(res.stop_reason == 0)
    assert T_after.tobytes() == (T if aligned else T_before).tobytes()
    assert res.active_pairs == 3 and res.cost_last < res.cost_first
    # where the maps really are: Dk times the anchor; the reference on the downloaded maps sets the limit
    data = [rr.MapData.of_scene(gpu, s) for s in made]
    T_ref, ref = rg.register_graph(data, T_before, pairs, anchor)
    corners = data[0].corners()
    for k in (1, 2):
        truth = D[k].astype(np.float64) @ T_before[0].astype(np.float64)
        start, d_ref, d_gpu = (rr.pose_distance(X[k], truth, corners, data[0].vs) for X in (T_before, T_ref, T))
        print(f"  map {k}: {start:.4g} voxel from its true pose at the start, {d_ref:.4g} after the reference (stop "
              f"{ref['stop_reason']}), {d_gpu:.4g} after the engine")
        assert d_ref < 0.5 * start and d_gpu <= 2 * d_ref
