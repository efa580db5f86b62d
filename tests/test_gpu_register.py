"""dslam_register_maps on the MI355X against the float64 reference of ref64_register.py: single evaluations sum by sum
within the derived rounding bound, the grid's coverage, whole runs, maps fused from frames, read-only-ness and
repeatability, stop reasons and argument errors, and the ITMLib mirror (AlignLocalMap)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_register as rr
import register_fixtures as fx
import util
import weighted_fixtures as wf

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "register_harness")


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


@pytest.fixture(scope="module")
def scenes(pkg, gpu):
    """Uploaded fixture maps, one scene per map, shared by the tests of this file (none of them writes a map)."""
    cache = {}

    def get(m):
        if id(m) not in cache:
            cache[id(m)] = (m, upload_map(gpu, pkg, m))
        return cache[id(m)][1]

    return get


def one_evaluation(pkg, gpu, src, dst, X0, **kw):
    X, res = gpu.register_maps(src, dst, X0, pkg.RegisterParams(max_evaluations=1, **kw))
    return X, res, gpu.debug_register_sums()


def check_evaluation(pkg, gpu, scenes, what, pair_src, pair_dst, src_map, dst_map, X0):
    ev = rr.evaluate(pair_src, pair_dst, rr.voxel_transform(np.asarray(X0, np.float32), pair_src.vs))
    X, res, sums = one_evaluation(pkg, gpu, scenes(src_map), scenes(dst_map), X0)
    used = ev.check_sums(sums, what)
    lo, hi = ev.cost_interval()
    print(f"{what}: {ev.candidates} candidates, {ev.valid} valid, {ev.ties} ties; the sums use up to {used:.3f} of the bound; "
          f"cost {res.cost_first:.6g} in [{lo:.6g}, {hi:.6g}]")
    assert res.candidates == ev.candidates and abs(res.valid_last - ev.valid) <= ev.ties
    assert lo <= res.cost_first <= hi and res.cost_last == res.cost_first
    assert res.evaluations == 1 and res.stop_reason == (3 if ev.valid < 500 else 1)
    assert X.tobytes() == np.asarray(X0, np.float32).tobytes()
    return ev, res, sums


# ---------------------------------------------------------------------------------------------------------------------
# 1. single evaluations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_single_evaluation_against_the_reference(pkg, gpu, scenes, case):
    what, pair, X0 = fx.single_evaluations()[case]
    ev, _, _ = check_evaluation(pkg, gpu, scenes, what, pair.src, pair.dst, pair.src_map, pair.dst_map, X0)
    assert ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates


def test_single_evaluation_with_scattered_voxels_without_weight(pkg, gpu, scenes):
    """The box-corner pair with w_depth 1 + texture and one voxel in 37 unobserved in both maps
    (weighted_fixtures.weighted_box_pair): the source's candidates and the destination's 8-tap gate both depend on single
    voxels' weights, and the counts and sums are the reference's."""
    pair, plain = wf.weighted_box_pair(), fx.box_pair("small")
    ev, res, _ = check_evaluation(pkg, gpu, scenes, "scattered zero weights", pair.src, pair.dst, pair.src_map, pair.dst_map,
                                  fx.near_truth(pair))
    assert ev.tie_share < 0.01
    assert 0.95 * plain.src.source_voxels()[2].astype(bool).sum() < pair.src.source_voxels()[2].astype(bool).sum()
    assert 0.7 * ev.candidates < ev.valid < 0.9 * ev.candidates      # 31 of 37 reads pass the gate


def test_exact_identity_on_a_map_registered_to_itself(pkg, gpu, scenes):
    pair = fx.box_pair("small")
    ev, res, sums = check_evaluation(pkg, gpu, scenes, "identity", pair.src, pair.src, pair.src_map, pair.src_map, I4)
    assert res.valid_last == res.candidates == 25395
    assert sums[27] == 0.0 and not np.any(sums[21:27]) and res.cost_first == 0.0
    # q = p exactly: the sums of q are sums of integers
    p, sdf, w = pair.src.source_voxels()
    cand = (w > 0) & (np.abs(sdf) < 16383)
    assert np.array_equal(sums[29:32], p[cand].sum(0).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# 2. grid coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_coverage(pkg, gpu, scenes):
    """More live blocks than workgroups (some make two trips, others one), then 5 blocks on the same engine (idle
    workgroups must write zeros over the rows of the large run), then a source without a resident block."""
    big = fx.sphere_pair()
    n_big = len(big.dst_map.block_pos)
    assert 512 < n_big < 1024                  # the grid has 512 workgroups
    X0 = fx.off_lattice(1.5, 0.45)
    check_evaluation(pkg, gpu, scenes, f"{n_big} blocks", big.dst, big.dst, big.dst_map, big.dst_map, X0)
    box = fx.box_pair("small")
    m = box.src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:5]   # 5 blocks the surface passes through
    few = am.Map(m.vs, m.mu, m.block_pos[pick], m.voxels[pick], 0x400, 0x100, 0x100, m.geom)
    ev, res, _ = check_evaluation(pkg, gpu, scenes, "5 blocks", rr.MapData.of_map(few), box.dst, few, box.dst_map, fx.off_lattice())
    assert ev.valid > 0 and len(few.block_pos) == 5
    empty = gpu.create_scene(m.scene_params(pkg))
    X, res, sums = one_evaluation(pkg, gpu, empty, scenes(box.dst_map), fx.off_lattice())
    assert res.candidates == 0 and res.valid_last == 0 and res.stop_reason == 3 and not np.any(sums)
    assert res.conditioning == 0.0 and X.tobytes() == fx.off_lattice().tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", [("box", "small"), ("box", "large"), ("box", "xl"), ("holes", None)])
def test_whole_run_against_the_reference(pkg, gpu, scenes, kind, name):
    pair, X_ref, ref = fx.reference_run(kind, name)
    src, dst = scenes(pair.src_map), scenes(pair.dst_map)
    X, res = gpu.register_maps(src, dst, I4)
    d_ref, d_gpu, apart = pair.distance(X_ref), pair.distance(X), rr.pose_distance(X, X_ref, pair.src.corners(), am.VS)
    # a decision whose cost difference is below the rounding bound of the two costs may fall either way in float32
    tie_at = next((k for k, t in enumerate(ref["trace"]) if k > 0 and t["margin"] < t["cost_slack"]), None)
    print(f"{kind} {name}: reference {ref['evaluations']} evaluations (stop {ref['stop_reason']}), engine {res.evaluations} "
          f"(stop {res.stop_reason}); distance to the truth {d_ref:.4g} / {d_gpu:.4g} voxel, apart {apart:.4g}; first decision "
          f"within the bound: evaluation {tie_at}; conditioning {res.conditioning:.4g} / {ref['conditioning']:.4g}")
    assert apart <= 4 * d_ref and d_gpu <= 2 * d_ref
    assert res.candidates == ref["candidates"]
    if tie_at is None:
        upto, X_cap, cap, X_g, r_g = ref["evaluations"], X_ref, ref, X, res
    else:
        # compare up to the evaluation before that decision: both runs capped there
        upto = tie_at
        X_cap, cap = rr.register(pair.src, pair.dst, I4, max_evaluations=upto)
        X_g, r_g = gpu.register_maps(src, dst, I4, pkg.RegisterParams(max_evaluations=upto))
    assert upto >= 3
    assert r_g.evaluations == cap["evaluations"] and r_g.stop_reason == cap["stop_reason"]
    assert abs(r_g.valid_last - cap["valid_last"]) <= max(cap["last"].ties, 1)
    assert abs(r_g.conditioning - cap["conditioning"]) <= 1e-3 * cap["conditioning"] + 1e-6
    # the same accepted steps: the poses differ by float32 rounding of the sums only
    assert rr.pose_distance(X_g, X_cap, pair.src.corners(), am.VS) <= max(4 * d_ref, 1e-3)
    if tie_at is None or ref["stop_reason"] == res.stop_reason:
        assert abs(res.valid_last - ref["valid_last"]) <= max(ref["last"].ties, 1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. maps fused from frames
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_maps_recover_a_known_offset(pkg, gpu, synth):
    """The same keyframes fused into two scenes, the second under poses composed with a known offset (1 voxel, 5 mrad):
    weights vary, zero-weight voxels exist, and the surface is whatever the fusion made of it."""
    wl = synth.s_tiny(96, 72)
    p = util.small_params(pkg, wl)
    D = rr.rigid(5e-3, fx.AXIS, np.array([0.6, -0.64, 0.48]) * p.voxel_size)
    Dinv = np.linalg.inv(D)
    made = []
    view = gpu.create_view(wl.W, wl.H)
    for k in range(2):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i in range(3):
            rgba, mm, M = wl.frame(5 * i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, (M.astype(np.float64) @ (Dinv if k else np.eye(4))).astype(np.float32), wl.intr)
        made.append(scene)
    A, B = (rr.MapData.of_scene(gpu, s) for s in made)
    wA = A.vba[A.ptr]["w_depth"]
    assert (wA == 0).any() and len(np.unique(wA)) >= 3
    params = dict(max_evaluations=6)
    X_ref, ref = rr.register(A, B, I4, **params)
    X, res = gpu.register_maps(made[0], made[1], I4, pkg.RegisterParams(**params))
    corners = A.corners()
    start, d_ref, d_gpu = (rr.pose_distance(T, D, corners, A.vs) for T in (I4, X_ref, X))
    print(f"fused maps: {len(A.block_pos)} / {len(B.block_pos)} blocks, {res.candidates} candidates, {res.valid_last} valid; offset "
          f"{start:.4g} voxel at the start, {d_ref:.4g} after the reference, {d_gpu:.4g} after the engine")
    assert res.candidates == ref["candidates"] > 20000
    assert d_ref < 0.25 * start          # the reference recovers the offset ...
    assert d_gpu <= 2 * d_ref            # ... and so does the engine


# ---------------------------------------------------------------------------------------------------------------------
# 5. read-only and repeatable
# ---------------------------------------------------------------------------------------------------------------------
def test_read_only_repeatable_and_asynchronous(pkg, gpu, synth):
    pair = fx.holes_pair()
    src, dst = upload_map(gpu, pkg, pair.src_map), upload_map(gpu, pkg, pair.dst_map)
    before = [util.snapshot(gpu, s) for s in (src, dst)]
    X1, r1 = gpu.register_maps(src, dst, I4)
    s1 = gpu.debug_register_sums()
    X2, r2 = gpu.register_maps(src, dst, I4)
    s2 = gpu.debug_register_sums()
    assert X1.tobytes() == X2.tobytes() and bytes(r1) == bytes(r2) and s1.tobytes() == s2.tobytes()
    assert r1.stop_reason == 0
    # an asynchronous engine with work in flight: frames being fused into a third scene
    wl = synth.s_tiny()
    third = gpu.create_scene(util.small_params(pkg, wl))
    rs = gpu.create_render_state(third, wl.W, wl.H)
    view = gpu.create_view(wl.W, wl.H)
    try:
        gpu.set_async(True)
        for i in range(3):
            rgba, mm, M = wl.frame(i)
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(third, view, rs, M, wl.intr)
        X3, r3 = gpu.register_maps(src, dst, I4)
        s3 = gpu.debug_register_sums()
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert X3.tobytes() == X1.tobytes() and bytes(r3) == bytes(r1) and s3.tobytes() == s1.tobytes()
    for s, snap, what in ((src, before[0], "source"), (dst, before[1], "destination")):
        util.assert_same_state(snap, util.snapshot(gpu, s), what)
        assert snap["stats"] == gpu.stats(s), what


# ---------------------------------------------------------------------------------------------------------------------
# 6. stop reasons and errors
# ---------------------------------------------------------------------------------------------------------------------
def test_stop_reasons(pkg, gpu, scenes):
    pair, X_ref, ref = fx.reference_run("box", "xxl")
    X, res = gpu.register_maps(scenes(pair.src_map), scenes(pair.dst_map), I4)
    print(f"xxl: stop {res.stop_reason} after {res.evaluations} evaluations ({ref['stop_reason']} after {ref['evaluations']}), "
          f"{res.valid_last} of {res.candidates} valid, conditioning {res.conditioning:.3g}")
    assert res.stop_reason != 0 and res.valid_last / res.candidates < 0.2 and res.conditioning < 1e-3
    # disjoint: the source 3 m from the destination
    small = fx.box_pair("small")
    far = rr.rigid(0.0, fx.AXIS, (3.0, 0.0, 0.0)).astype(np.float32)
    X, res = gpu.register_maps(scenes(small.src_map), scenes(small.dst_map), far)
    assert res.stop_reason == 3 and res.evaluations == 1 and res.valid_last == 0 and res.conditioning == 0.0
    assert res.candidates == 25395 and X.tobytes() == far.tobytes()
    assert abs(res.cost_first - 0.5625) < 1e-6
    # src == dst converges where it starts
    X, res = gpu.register_maps(scenes(small.src_map), scenes(small.src_map), I4)
    assert res.stop_reason in (0, 2) and res.valid_last == res.candidates
    assert rr.pose_distance(X, I4, small.src.corners(), am.VS) < 0.01


def test_invalid_arguments_leave_x_untouched(pkg, gpu, scenes):
    pair = fx.box_pair("small")
    src, dst = scenes(pair.src_map), scenes(pair.dst_map)
    other_vs = upload_map(gpu, pkg, pair.dst_map, voxel_size=0.006)
    other_mu = upload_map(gpu, pkg, pair.dst_map, mu=0.03)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = upload_map(second, pkg, pair.dst_map)
    start = fx.off_lattice()
    nan, sing = start.copy(), start.copy()
    nan[1, 3] = np.nan
    sing[:3, :3] = 0.0

    def call(s, d, X0, params=None, result=True, x_null=False):
        X = pkg.mat_to_abi(X0).copy()
        keep = X.copy()
        res = pkg.RegisterResult()
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu._call("register_maps", gpu._engine, s.ptr if s is not None else None, d.ptr if d is not None else None,
                      None if x_null else X.ctypes.data_as(C.POINTER(C.c_float)),
                      C.byref(params) if params is not None else None, C.byref(res) if result else None)
        assert X.tobytes() == keep.tobytes()

    call(None, dst, start)
    call(src, None, start)
    call(src, dst, start, result=False)
    call(src, dst, start, x_null=True)
    call(src, foreign, start)
    call(src, other_vs, start)
    call(src, other_mu, start)
    call(src, dst, nan)
    call(src, dst, sing)
    for field in ("band", "residual_gate", "max_evaluations", "min_valid", "term_rotation", "term_translation_voxels"):
        call(src, dst, start, params=pkg.RegisterParams(**{field: -1}))
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("debug_register_sums", gpu._engine, None)
    # NULL params are the defaults
    X = pkg.mat_to_abi(I4).copy()
    res = pkg.RegisterResult()
    gpu._call("register_maps", gpu._engine, src.ptr, dst.ptr, X.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(res))
    Xd, rd = gpu.register_maps(src, dst, I4, pkg.RegisterParams(0.5, 0.75, 30, 500, 1e-5, 1e-3))
    assert X.tobytes() == pkg.mat_to_abi(Xd).tobytes() and bytes(res) == bytes(rd)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the ITMLib mirror
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


MIRROR_FRAMES = dict(W=80, H=60, n_frames=4, stride=4)   # S-tiny keyframes 0, 4, 8, 12


def run_mirror(pkg, gpu, synth, tmp_path, D, W, H, n_frames, stride):
    """register_harness on S-tiny keyframes with the offset D, and the same maps re-fused through the C ABI.  Returns
    (T_dst, T_before, T_after as the harness wrote them, its result, its return value, the harness' output, the two
    scenes [dst, src], the scene parameters)."""
    wl = synth.s_tiny(W, H)
    p = util.small_params(pkg, wl)
    frames = [wl.frame(stride * i) for i in range(n_frames)]
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for rgba, mm, M in frames:
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
        f.write(pkg.mat_to_abi(D).tobytes())
    run = subprocess.run([HARNESS, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    T_dst, T_before, T_after = (np.frombuffer(raw, np.float32, 16, 64 * k) for k in range(3))
    fused = np.frombuffer(raw, np.float32, 16 * 2 * n_frames, 192).reshape(2, n_frames, 4, 4).transpose(0, 1, 3, 2)
    tail = 192 + 64 * 2 * n_frames
    assert len(raw) == tail + 36
    res_h = pkg.RegisterResult.from_buffer_copy(raw[tail:tail + 32])
    aligned, = struct.unpack_from("<i", raw, tail + 32)
    made = []
    view = gpu.create_view(wl.W, wl.H)
    for k in range(2):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (rgba, mm, _) in enumerate(frames):
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    return T_dst, T_before, T_after, res_h, aligned, run.stdout.strip(), made, p


@pytest.mark.parametrize("offset", ["within reach", "out of reach"])
def test_mirror_align_local_map_equals_abi(pkg, gpu, synth, tmp_path, offset):
    """register_harness: two local maps of the same keyframes, the second displaced by D without its estimatedGlobalPose
    knowing; AlignLocalMap(1, 0) moves that pose exactly where register_maps on the same maps, re-fused through the C ABI,
    puts it -- and leaves it alone when the registration does not converge.  (Maps fused from frames do not always end
    with stop reason 0; these keyframes are among those that do.)"""
    vs = synth.s_tiny().scene_kwargs["voxel_size"]
    if offset == "within reach":
        D = rr.rigid(5e-3, fx.AXIS, np.array([0.6, -0.64, 0.48]) * vs)
    else:
        D = rr.rigid(0.5, fx.AXIS, np.array([0.6, -0.64, 0.48]) * 40 * vs)
    D = D.astype(np.float32)
    T_dst, T_before, T_after, res_h, aligned, said, made, p = run_mirror(pkg, gpu, synth, tmp_path, D, **MIRROR_FRAMES)
    # the same registration through the C ABI (map 0 is the destination, map 1 the source)
    X0 = _rigid_product(_as_doubles(T_dst), _rigid_inverse(_as_doubles(T_before)))
    X0 = np.array(X0, np.float64).astype(np.float32).reshape(4, 4).T
    X, res = gpu.register_maps(made[1], made[0], X0)
    print(f"mirror, {offset}: {said}; C ABI: stop {res.stop_reason} after {res.evaluations} evaluations")
    assert bytes(res) == bytes(res_h)
    assert T_before.tobytes() == T_dst.tobytes()
    if offset == "within reach":
        assert res.stop_reason == 0 and aligned == 1
        want = _rigid_product(_rigid_inverse(_as_doubles(pkg.mat_to_abi(X))), _as_doubles(T_dst))
        assert np.array(want, np.float64).astype(np.float32).tobytes() == T_after.tobytes()
        # and it is where the map really is: D times the anchor
        truth = D.astype(np.float64) @ T_dst.reshape(4, 4).T.astype(np.float64)
        A = rr.MapData.of_scene(gpu, made[1])
        assert rr.pose_distance(T_after.reshape(4, 4).T, truth, A.corners(), A.vs) < 0.25
    else:
        assert res.stop_reason != 0 and aligned == 0
        assert T_after.tobytes() == T_before.tobytes()
