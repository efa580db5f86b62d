"""dslam_mesh_scene_multi on the MI355X: exact reductions to dslam_mesh_scene, one posed map, the blended single surface
of two overlapping maps and the seam of two maps side by side against the float64 reference of ref64_multimesh.py and
against closed-form geometry, and the interface (arguments, saturation, async mode, the mesh buffers)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import multimesh_fixtures as fx
import ref64_multimesh as r64
import util
import weighted_fixtures as wf

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "multimesh_harness")


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fused_room", "analytic"])
@pytest.mark.parametrize("colour", [False, True])
def test_exact_reduction_to_mesh_scene(pkg, gpu, synth, source, colour):
    if source == "fused_room":
        wl = synth.s_tiny()
        params = util.small_params(pkg, wl)
        A = util.run_sequence(gpu, pkg, wl, params, 4)[0]
        far = upload_map(gpu, pkg, am.build_map(am.Sphere((0.0, 0.0, 0.5), 0.3), params.voxel_size, params.mu,
                                                 (-0.35, -0.35, 0.15), (0.35, 0.35, 0.85)))
    else:
        m = am.colour_plane()
        params = m.scene_params(pkg)
        A = upload_map(gpu, pkg, m)
        far = upload_map(gpu, pkg, am.colour_plane())
    T_far = fx.pose(t=(100.0, 0.0, 0.0))
    want_p, want_c = gpu.mesh_scene(A, colour=colour)
    n = len(want_p)
    assert n > 5000

    def check(pos, col, what):
        assert same(pos, want_p), f"{what}: positions"
        if colour:
            assert same(col, want_c), f"{what}: colours"
        else:
            assert col is None

    pos, col, counts = gpu.mesh_scene_multi([A], [I4], colour=colour)
    assert list(counts) == [n]
    check(pos, col, "alone")
    again = gpu.mesh_scene_multi([A], [I4], colour=colour)
    check(again[0], again[1], "second run")
    empty = gpu.create_scene(params)
    pos, col, counts = gpu.mesh_scene_multi([A, empty], [I4, fx.pose(yaw=0.3, t=(0.1, 0.0, -0.2))], colour=colour)
    assert list(counts) == [n, 0]
    check(pos, col, "with an empty scene")
    pos, col, counts = gpu.mesh_scene_multi([A, far], [I4, T_far], colour=colour)
    assert counts[0] == n and counts[1] > 1000 and counts.sum() == len(pos)
    check(pos[:n], col[:n] if colour else None, "far map appended")
    pos2, col2, counts2 = gpu.mesh_scene_multi([far, A], [T_far, I4], colour=colour)
    assert counts2[1] == n and counts2[0] == counts[1] and counts2.sum() == len(pos2)
    check(pos2[counts2[0]:], col2[counts2[0]:] if colour else None, "far map prepended")
    assert same(pos2[:counts2[0]], pos[n:])
    twice = gpu.mesh_scene_multi([far, A], [T_far, I4], colour=colour)
    assert same(twice[0], pos2) and (not colour or same(twice[1], col2))


# ---------------------------------------------------------------------------------------------------------------------
# 2. one posed map
# ---------------------------------------------------------------------------------------------------------------------
def test_one_posed_map_is_the_posed_single_mesh(pkg, gpu):
    m = am.sphere_outside(colour=lambda x: 128.0 + 300.0 * (x - np.array([0.03, -0.02, 0.45])))
    A = upload_map(gpu, pkg, m)
    T = fx.pose(yaw=0.15, roll=0.05, t=(0.03, -0.02, 0.04))
    want_p, want_c = gpu.mesh_scene(A, colour=True)
    pos, col, counts = gpu.mesh_scene_multi([A], [T], colour=True)
    assert len(want_p) > 5000 and list(counts) == [len(want_p)] and pos.shape == want_p.shape
    Tinv = np.linalg.inv(T.astype(np.float64))
    expect = want_p.astype(np.float64).reshape(-1, 3) @ Tinv[:3, :3].T + Tinv[:3, 3]
    err = np.abs(pos.astype(np.float64).reshape(-1, 3) - expect).max() / am.VS
    assert err <= 1e-3, f"vertices up to {err:.3g} voxel from T^-1 of the single-map mesh"
    assert same(col, want_c)


# ---------------------------------------------------------------------------------------------------------------------
# 3. overlap: one blended surface
# ---------------------------------------------------------------------------------------------------------------------
def _triangle_areas(pos):
    p = pos.astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def test_overlap_gives_one_blended_surface(pkg, gpu):
    maps, c_world, r = fx.two_spheres()
    scenes = [upload_map(gpu, pkg, pm.m) for pm in maps]
    Ts = [pm.T for pm in maps]
    pos, col, counts = gpu.mesh_scene_multi(scenes, Ts, colour=True)
    assert counts.sum() == len(pos) > 10000
    # against the float64 reference, cube by cube
    ref = fx.reference("two_spheres")
    share = r64.tie_share(ref)
    assert share <= 0.02, f"tie share {share:.3%}"
    res = r64.compare(ref, pos, col, counts, am.VS)
    print(f"two spheres: {res['cubes']} cubes compared, vertices within {res['max_vertex']:.3g} voxel, colours within "
          f"{res['max_colour'] * 255:.3g} / 255, tie share {share:.3%}")
    assert res["cubes"] > 5000
    # geometry: one surface at the weighted consensus (5 d + 20 (d - 2)) / 25 = 0 -> d = 1.6 voxel outside r
    d = np.linalg.norm(pos.astype(np.float64).reshape(-1, 3) - c_world, axis=1) / am.VS
    off = np.abs(d - (r / am.VS + 1.6)).max()
    assert off <= 0.25, f"vertices up to {off:.3g} voxel from the blended radius"
    area = _triangle_areas(pos).sum()
    want_area = 4.0 * np.pi * (r + 1.6 * am.VS) ** 2
    assert abs(area / want_area - 1.0) <= 0.02, f"area {area / want_area:.4f} of the blended sphere's"
    assert counts[1] == 0   # the first map has no hole
    # colour: the w_color-weighted mean (1 : 3) of the two flat colours
    want = (np.array(fx.COLOUR_A) + 3.0 * np.array(fx.COLOUR_B)) / 4.0 / 255.0
    assert np.abs(col.astype(np.float64) - want).max() <= 1.0 / 255.0


def test_weight_fields_and_a_slab_without_weight(pkg, gpu):
    """The two spheres with w_depth = 1 + texture + ramp (1 .. 35), w_color = (2x + 3y + 5z) mod 4, and a slab of map 0, 12
    voxels thick, whose voxels hold their sdf and colour under the weight 0 (weighted_fixtures.mesh_spheres): cube by cube
    against the float64 reference that reads every voxel's own weights, with the tolerances and the tie handling of
    test_overlap_gives_one_blended_surface.  Inside the slab map 0 does not cover map 1, whose cubes leave their triangles;
    outside it does.  The colours compared are blends by w_color, zeros included."""
    maps = fx.fixture("weighted_spheres")
    scenes = [upload_map(gpu, pkg, pm.m) for pm in maps]
    pos, col, counts = gpu.mesh_scene_multi(scenes, [pm.T for pm in maps], colour=True)
    assert counts.sum() == len(pos) > 10000
    ref = fx.reference("weighted_spheres")
    share = r64.tie_share(ref)
    assert share <= 0.02, f"tie share {share:.3%}"
    res = r64.compare(ref, pos, col, counts, am.VS)
    print(f"weighted spheres: {res['cubes']} cubes compared, vertices within {res['max_vertex']:.3g} voxel, colours within "
          f"{res['max_colour'] * 255:.3g} / 255, tie share {share:.3%}")
    assert res["cubes"] > 5000
    # map 1's cubes by where their centre lies in map 0: well inside the slab, or well outside it, on a voxel map 0 holds
    r, A = ref[1], maps[0]
    to_world = np.linalg.inv(r["T"])
    centre = A.to_map((r["g"] + 0.5) @ to_world[:3, :3].T + to_world[:3, 3])
    v = centre[:, 1] - (A.T[:3, :3].astype(np.float64) @ wf.C_WORLD + A.T[:3, 3])[1] / am.VS
    held = A.m.lookup(np.floor(centre + 0.5).astype(np.int64))[2]
    got = np.bincount(r64.cubes_of_triangles(r, pos[counts[0]:], am.VS), minlength=len(r["g"]))
    off_tie = ~r["tie"] & r["produce"] & held
    lo, hi = wf.MESH_SLAB
    inside, outside = off_tie & (v > lo + 1.5) & (v < hi - 1.5), off_tie & ((v < lo - 1.5) | (v > hi + 1.5))
    print(f"weighted spheres: map 1 leaves {got[inside].sum()} triangles in {(got[inside] > 0).sum()} of {inside.sum()} cubes "
          f"inside the slab, {got[outside].sum()} in {outside.sum()} cubes outside it")
    assert inside.sum() > 1000 and (got[inside] > 0).all() and np.array_equal(got[inside], r["ntri"][inside])
    assert outside.sum() > 10000 and got[outside].sum() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. partial overlap: the seam
# ---------------------------------------------------------------------------------------------------------------------
def _hits_along_z(pos, pts):
    """How many triangles of `pos` each line (x, y) = pts[k], along z, passes through (no point lies on an edge)."""
    a, b, c = (pos[:, k, :2].astype(np.float64) for k in range(3))
    hits = np.zeros(len(pts), np.int64)
    for s in range(0, len(pts), 128):
        p = pts[s:s + 128, None, :]

        def side(u, v):
            return (v[None, :, 0] - u[None, :, 0]) * (p[..., 1] - u[None, :, 1]) - (v[None, :, 1] - u[None, :, 1]) * (p[..., 0] - u[None, :, 0])

        d0, d1, d2 = side(a, b), side(b, c), side(c, a)
        inside = ((d0 > 0) & (d1 > 0) & (d2 > 0)) | ((d0 < 0) & (d1 < 0) & (d2 < 0))
        hits[s:s + 128] = inside.sum(1)
    return hits


def test_partial_overlap_leaves_one_surface_and_a_seam(pkg, gpu):
    maps = fx.seam_planes()
    scenes = [upload_map(gpu, pkg, pm.m) for pm in maps]
    pos, col, counts = gpu.mesh_scene_multi(scenes, [pm.T for pm in maps], colour=True)
    assert counts[0] > 5000 and counts[1] > 3000 and counts.sum() == len(pos)
    off, edge = fx.seam_wall_offsets(pos)
    print(f"seam: vertices up to {off[~edge].max():.3g} voxel off the wall, {off[edge].max():.3g} within 2 voxels of a "
          f"map's edge ({edge.mean():.1%} of them)")
    assert edge.mean() < 0.25 and off[~edge].max() <= 0.25 and off[edge].max() <= 1.0   # (bounds: seam_wall_offsets)
    # lines along the wall's normal over its interior, off every voxel lattice by an irrational fraction of a voxel
    gx = np.arange(-0.28, 0.27, 0.011) + am.VS * 0.6180339887
    gy = np.arange(-0.12, 0.12, 0.006) + am.VS * 0.4142135624
    pts = np.stack(np.meshgrid(gx, gy, indexing="ij"), -1).reshape(-1, 2)
    assert 1800 <= len(pts) <= 2200
    hits = _hits_along_z(pos, pts)
    assert hits.max() <= 1, f"{(hits > 1).sum()} lines meet the mesh more than once"
    missed = pts[hits == 0]
    assert (np.abs(missed[:, 0] - fx.SEAM_X) <= 2.0 * am.VS).all(), \
        f"lines that miss the mesh up to {np.abs(missed[:, 0] - fx.SEAM_X).max() / am.VS:.3g} voxel from the seam"
    # both maps contribute: A left of the seam, B right of it
    assert (hits[pts[:, 0] < fx.SEAM_X - 2 * am.VS] == 1).all() and (hits[pts[:, 0] > fx.SEAM_X + 2 * am.VS] == 1).all()
    ref = fx.reference("seam_planes")
    share = r64.tie_share(ref)
    assert share <= 0.02, f"tie share {share:.3%}"
    res = r64.compare(ref, pos, col, counts, am.VS)
    print(f"seam: {res['cubes']} cubes compared, vertices within {res['max_vertex']:.3g} voxel, colours within "
          f"{res['max_colour'] * 255:.3g} / 255, tie share {share:.3%}")
    assert res["cubes"] > 5000


# ---------------------------------------------------------------------------------------------------------------------
# 5. interface
# ---------------------------------------------------------------------------------------------------------------------
def test_interface(pkg, gpu):
    m = am.sphere_outside()
    A = upload_map(gpu, pkg, m)
    B = upload_map(gpu, pkg, am.colour_plane())
    T_b = fx.pose(yaw=0.1, t=(100.0, 0.0, 0.0))
    single = gpu.mesh_scene(A, colour=True)
    n = len(single[0])
    other_vs = upload_map(gpu, pkg, am.sphere_outside(), voxel_size=0.006)
    other_mu = upload_map(gpu, pkg, am.sphere_outside(), mu=0.03)
    second = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_two_engines.py)
    foreign = upload_map(second, pkg, am.sphere_outside())
    cases = [
        ("voxel_size", [A, other_vs], [I4, I4]),
        ("mu", [A, other_mu], [I4, I4]),
        ("no maps", [], np.zeros((0, 4, 4), np.float32)),
        ("65 maps", [A] * 65, [I4] * 65),
        ("singular", [A, B], [I4, np.zeros((4, 4), np.float32)]),
        ("NULL scene", [A, None], [I4, I4]),
        ("another engine's scene", [A, foreign], [I4, T_b]),
    ]

    def previous_mesh_is_there(what):
        pos = np.empty((n, 3, 3), np.float32)
        col = np.empty((n, 3, 3), np.float32)
        gpu._call("mesh_download", gpu._engine, pos.ctypes.data_as(C.POINTER(C.c_float)),
                  col.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(n))
        assert same(pos, single[0]) and same(col, single[1]), what

    for what, scenes, poses in cases:
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu.mesh_scene_multi(scenes, poses, colour=True)
        previous_mesh_is_there(what)
    ptrs = (C.c_void_p * 1)(A.ptr)
    t_abi = np.ascontiguousarray(I4.T).reshape(-1)
    with pytest.raises(pkg.DslamError, match="status -1 "):
        gpu._call("mesh_scene_multi", gpu._engine, ptrs, t_abi.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(1),
                  C.c_int(0), C.c_int(1), None, None)
    previous_mesh_is_there("NULL out_num_triangles")
    # saturation at max_triangles - 1, over the map boundary too
    full = gpu.mesh_scene_multi([A, B], [I4, T_b])
    assert full[2][0] == n and full[2][1] > 100
    for cap, want in ((1, [0, 0]), (2, [1, 0]), (100, [99, 0]), (n + 11, [n, 10])):
        pos, _, counts = gpu.mesh_scene_multi([A, B], [I4, T_b], max_triangles=cap)
        assert list(counts) == want and len(pos) == sum(want) == max(cap - 1, 0)
        assert same(pos, full[0][:len(pos)])
    # 64 maps is the limit, not an error: the 63 copies behind the first are covered by it
    pos, _, counts = gpu.mesh_scene_multi([A] * 64, [I4] * 64)
    assert counts[1:].sum() == 0 and abs(int(counts[0]) - n) <= 0.01 * n and len(pos) == counts[0]
    # a mesh made without colours cannot be downloaded with them
    buf = np.empty((n + 1, 3, 3), np.float32)
    with pytest.raises(pkg.DslamError):
        gpu._call("mesh_download", gpu._engine, buf.ctypes.data_as(C.POINTER(C.c_float)),
                  buf.ctypes.data_as(C.POINTER(C.c_float)), C.c_int(len(buf)))
    # an asynchronous engine gives the same bytes
    want = gpu.mesh_scene_multi([A, B], [fx.pose(yaw=0.2, t=(0.01, 0.0, 0.0)), T_b], colour=True)
    try:
        gpu.set_async(True)
        got = gpu.mesh_scene_multi([A, B], [fx.pose(yaw=0.2, t=(0.01, 0.0, 0.0)), T_b], colour=True)
        gpu.synchronize()
    finally:
        gpu.set_async(False)
    assert same(got[0], want[0]) and same(got[1], want[1]) and np.array_equal(got[2], want[2])
    # dslam_mesh_scene directly after a composite call still equals its own earlier result
    after = gpu.mesh_scene(A, colour=True)
    assert same(after[0], single[0]) and same(after[1], single[1])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_save_all_local_maps_equals_abi(pkg, gpu, synth, tmp_path):
    """multimesh_harness: 2 local maps (a new one every 3 keyframes, anchored at that keyframe's pose), then
    SaveAllLocalMapsToMesh; the same maps built and meshed through the C ABI give the same vertices."""
    wl = synth.s_tiny()
    n_frames, K = 6, 3
    p = util.small_params(pkg, wl, num_local_blocks=0x800, num_buckets=0x1000, num_excess=0x400)
    frames = [wl.frame(i) for i in range(n_frames)]
    fin, fout, obj = tmp_path / "frames.bin", tmp_path / "out.bin", tmp_path / "all.obj"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for rgba, mm, M in frames:
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
    res = subprocess.run([HARNESS, str(fin), str(fout), str(K), str(obj)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = open(fout, "rb").read()
    n_maps, = struct.unpack_from("<i", raw, 0)
    assert n_maps == 2
    T = np.frombuffer(raw, np.float32, 16 * n_maps, 4).reshape(n_maps, 4, 4).transpose(0, 2, 1)
    fused = np.frombuffer(raw, np.float32, 16 * n_frames, 4 + 64 * n_maps).reshape(n_frames, 4, 4).transpose(0, 2, 1)
    scenes = [gpu.create_scene(p) for _ in range(n_maps)]
    rss = [gpu.create_render_state(s, wl.W, wl.H) for s in scenes]
    v = gpu.create_view(wl.W, wl.H)
    for i, (rgba, mm, _) in enumerate(frames):
        gpu.view_update(v, rgba, mm, timestamp=float(i))
        gpu.process_frame(scenes[i // K], v, rss[i // K], fused[i], wl.intr)
    pos, col, counts = gpu.mesh_scene_multi(scenes, T, colour=True)   # (the mirror's settings default to meshWithColour)
    assert len(pos) > 5000 and counts[0] > 0
    lines = open(obj).read().splitlines()
    verts = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")])
    faces = sum(ln.startswith("f ") for ln in lines)
    assert faces == len(pos) and len(verts) == 3 * len(pos) and verts.shape[1] == 6
    flat = np.concatenate([pos.reshape(-1, 3), col.reshape(-1, 3)], axis=1).astype(np.float64)
    for k in (0, -1):
        assert np.abs(verts[k] - flat[k]).max() <= 1e-6, (verts[k], flat[k])   # (the file carries six decimals)
