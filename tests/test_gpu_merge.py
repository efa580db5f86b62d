"""dslam_merge_maps on the MI355X against the sequential restatement of its law in ref_merge.py.  In every case the
destination's hash table, both free lists with their tops, every voxel block and every field of the result are compared
byte for byte: the law is float32 with a fixed operation order and contraction is off on both sides, so there is no
tolerance anywhere in this file."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_register as rr
import ref_merge as rm
import register_fixtures as fx
import util
import weighted_fixtures as wf

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "merge_harness")
W, H = 80, 60
INTR = (100.0, 100.0, 40.0, 30.0)


def scene_of(pkg, gpu, st):
    scene = gpu.create_scene(st.scene_params(pkg))
    st.upload(gpu, scene)
    return scene


def check_merge(pkg, gpu, what, src, dst, X, max_passes=0, with_colour=1, engine=None):
    """One merge on the device and in the reference; returns (result, reference result, merged state, scenes)."""
    api = engine or gpu
    s_src, s_dst = scene_of(pkg, api, src), scene_of(pkg, api, dst)
    params = pkg.MergeParams(max_passes=max_passes, with_colour=with_colour) if (max_passes or not with_colour) else None
    res = api.merge_maps(s_src, s_dst, X, params).as_dict()
    got = rm.State.download(api, s_dst, dst)
    want = dst.copy()
    ref = rm.merge(src, want, X, max_passes=max_passes, with_colour=with_colour)
    print(f"{what}: {ref}")
    diff = want.differences(got)
    assert not diff, f"{what}: the destination differs from the reference in {diff}"
    assert res == ref, f"{what}: result {res}, reference {ref}"
    after = rm.State.download(api, s_src, src)
    assert not src.differences(after), f"{what}: the source changed"
    return res, ref, got, (s_src, s_dst)


def empty_like(m, num_buckets=0x400):
    n = len(m.block_pos)
    return rm.State.empty(num_buckets, max(0x100, 2 * n) + (-(num_buckets + max(0x100, 2 * n))) % 16, 4 * n)


@functools.lru_cache(maxsize=None)
def state_of(kind, side):
    pair = {"box": lambda: fx.box_pair("small"), "holes": fx.holes_pair, "negative": fx.negative_pair}[kind]()
    return rm.State.of_map(pair.src_map if side == "src" else pair.dst_map)


def X_of(kind):
    pair = {"box": lambda: fx.box_pair("small"), "holes": fx.holes_pair, "negative": fx.negative_pair}[kind]()
    return pair.X_true.astype(np.float32)


def follow_up(pkg, gpu, what, s_dst, merged):
    """ProcessFrame + GetImage on the merged scene against the same calls on a fresh scene loaded with the downloaded
    state: equal only if the merge left alloc_bits and the memo / front-end upkeep as an upload leaves them."""
    fresh = scene_of(pkg, gpu, merged)
    rgba = np.full((H, W, 4), 200, np.uint8)
    depth = np.full((H, W), 480, np.int16)
    out = []
    for scene in (s_dst, fresh):
        rs, view = gpu.create_render_state(scene, W, H), gpu.create_view(W, H)
        before = gpu.get_image(scene, rs, I4, INTR, pkg.IMAGE_DEPTH).copy()
        gpu.view_update(view, rgba, depth)
        gpu.process_frame(scene, view, rs, I4, INTR)
        image = gpu.get_image(scene, rs, I4, INTR, pkg.IMAGE_DEPTH).copy()
        out.append((before, image, rm.State.download(gpu, scene, merged), gpu.download_visible_ids(rs)))
    (b0, i0, st0, v0), (b1, i1, st1, v1) = out
    assert (b0 > 0).sum() > 100, f"{what}: the camera does not see the merged map"
    assert b0.tobytes() == b1.tobytes(), f"{what}: GetImage of the merged scene differs from the reloaded one"
    assert not st1.differences(st0), f"{what}: ProcessFrame after the merge differs: {st1.differences(st0)}"
    assert np.array_equal(v0, v1) and i0.tobytes() == i1.tobytes(), f"{what}: image after ProcessFrame differs"


# ---------------------------------------------------------------------------------------------------------------------
# 1. / 2. identity
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_onto_an_empty_destination(pkg, gpu):
    src = state_of("box", "src")
    res, ref, got, _ = check_merge(pkg, gpu, "identity onto empty", src, empty_like(fx.box_pair("small").src_map), I4)
    a, b = src.voxels_by_position(), got.voxels_by_position()
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert res["blocks_allocated"] == res["src_blocks"] == 268 and res["voxels_changed"] == res["src_candidates"]


def _colour(x):
    return 128.0 + (x - np.array([0.0, 0.0, 0.4])) @ np.array([[300.0, 0.0, 40.0], [0.0, 250.0, -60.0], [60.0, 80.0, 0.0]])


@functools.lru_cache(maxsize=None)
def plane_maps():
    geom = am.Plane((0.1, 0.05, -1.0), -0.40)
    a = am.build_map(geom, am.VS, am.MU, (-0.15, -0.10, 0.2), (0.10, 0.10, 0.62), colour=_colour, w_depth=3)
    b = am.build_map(geom, am.VS, am.MU, (-0.05, -0.10, 0.2), (0.20, 0.10, 0.62), w_depth=99)
    return a, b


@pytest.mark.parametrize("coloured", ["source", "destination"])
def test_identity_onto_an_overlapping_destination_clamp_and_idle_colour(pkg, gpu, coloured):
    a, b = plane_maps()
    src, dst = (rm.State.of_map(a), rm.State.of_map(b)) if coloured == "source" else (rm.State.of_map(b), rm.State.of_map(a))
    res, ref, got, _ = check_merge(pkg, gpu, f"identity, colour in the {coloured}", src, dst, I4)
    assert got.vba["w_depth"].max() == 100 and res["blocks_allocated"] > 0 and res["blocks_touched"] > res["blocks_allocated"]
    if coloured == "destination":   # the source has no colour to give: every colour half idles
        assert got.vba["clr"].tobytes() == dst.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == dst.vba["w_color"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole-voxel translations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [(8, 0, 0), (3, -5, 2)])
def test_whole_voxel_translation(pkg, gpu, shift):
    X = np.eye(4, dtype=np.float32)
    X[:3, 3] = np.asarray(shift, np.float64) * am.VS
    Xt, Yt, identity = rm.transforms(X, am.VS)
    assert not identity and np.array_equal(Xt[:, 3], np.asarray(shift, np.float32)) and np.array_equal(Yt[:, 3], -Xt[:, 3])
    src = state_of("box", "src")
    res, ref, got, _ = check_merge(pkg, gpu, f"translation by {shift} voxels", src, state_of("box", "dst"), X)
    assert res["voxels_changed"] > 50000


# ---------------------------------------------------------------------------------------------------------------------
# 4. rigid transforms; 6. the follow-up
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "holes", "negative"])
def test_rigid_transform(pkg, gpu, kind):
    res, ref, got, (s_src, s_dst) = check_merge(pkg, gpu, kind, state_of(kind, "src"), state_of(kind, "dst"), X_of(kind))
    assert res["passes"] >= 2 and res["exhausted"] == 0 and res["blocks_allocated"] > 100
    if kind == "box":
        follow_up(pkg, gpu, kind, s_dst, got)


# ---------------------------------------------------------------------------------------------------------------------
# 5. chains
# ---------------------------------------------------------------------------------------------------------------------
def test_64_buckets_take_several_passes(pkg, gpu):
    m = fx.box_pair("small").dst_map
    n = len(m.block_pos)
    chained = am.Map(m.vs, m.mu, m.block_pos, m.voxels, 0x40, 2 * n + (-(0x40 + 2 * n)) % 16, 4 * n, m.geom)
    assert chained.max_chain >= 8
    res, ref, got, _ = check_merge(pkg, gpu, "64 buckets", state_of("box", "src"), rm.State.of_map(chained), X_of("box"))
    assert ref["passes"] >= 3 and res["passes"] == ref["passes"]


# ---------------------------------------------------------------------------------------------------------------------
# 6. pools that run dry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["blocks", "excess"])
def test_pool_exhaustion(pkg, gpu, short):
    dst = state_of("box", "dst").copy()
    full = rm.merge(state_of("box", "src"), dst.copy(), X_of("box"))
    if short == "blocks":
        dst.last_free = full["blocks_allocated"] - 7 - 1          # 7 blocks short
    else:
        dst.last_free_ex = 10 - 1                                 # 10 excess slots, more than enough blocks
    res, ref, got, (s_src, s_dst) = check_merge(pkg, gpu, f"pool short of {short}", state_of("box", "src"), dst, X_of("box"))
    assert res["exhausted"] == 1 and res["requests_unserved"] == ref["requests_unserved"] > 0
    if short == "blocks":
        assert got.last_free == -1 and res["blocks_allocated"] == full["blocks_allocated"] - 7
    else:
        assert got.last_free_ex == -1 and got.last_free >= 0
    follow_up(pkg, gpu, f"pool short of {short}", s_dst, got)


# ---------------------------------------------------------------------------------------------------------------------
# 7. grid coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_more_touched_blocks_than_the_grid_then_five(pkg, gpu):
    big = fx.sphere_pair()
    n_big = len(big.dst_map.block_pos)
    assert 512 < n_big < 1024                  # the block kernel's grid has 512 workgroups
    whole = rm.State.of_map(big.dst_map)
    X = fx.off_lattice(1.5, 0.45)
    res, ref, got, _ = check_merge(pkg, gpu, f"{n_big} blocks", whole, whole.copy(), X)
    assert res["blocks_touched"] > 512
    m = fx.box_pair("small").src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:5]
    few = am.Map(m.vs, m.mu, m.block_pos[pick], m.voxels[pick], 0x400, 0x100, 0x100, m.geom)
    res, ref, got, _ = check_merge(pkg, gpu, "5 blocks", rm.State.of_map(few), rm.State.of_map(few), I4)
    assert res["blocks_touched"] == 5 and res["blocks_allocated"] == 0 and res["passes"] == 1 and res["voxels_changed"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. repeatability, the asynchronous engine
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_an_asynchronous_engine_give_the_same_bytes(pkg, gpu, synth):
    src, dst, X = state_of("holes", "src"), state_of("holes", "dst"), X_of("holes")
    _, _, first, _ = check_merge(pkg, gpu, "first", src, dst, X)
    _, _, second, _ = check_merge(pkg, gpu, "second", src, dst, X)
    assert not first.differences(second)
    eng = pkg.open_engine(0)
    try:
        eng.set_async(True)
        wl = synth.s_tiny()
        busy = eng.create_scene(pkg.SceneParams(num_local_blocks=0x2000, num_buckets=0x4000, num_excess=0x800, **wl.scene_kwargs))
        rs, view = eng.create_render_state(busy, wl.W, wl.H), eng.create_view(wl.W, wl.H)
        rgba, mm, M = wl.frame(0)
        eng.view_update(view, rgba, mm)
        s_src, s_dst = scene_of(pkg, eng, src), scene_of(pkg, eng, dst)
        eng.process_frame(busy, view, rs, M, wl.intr)          # a fusion in flight when the merge is called
        res = eng.merge_maps(s_src, s_dst, X).as_dict()
        third = rm.State.download(eng, s_dst, dst)
        assert not first.differences(third)
        assert res == rm.merge(src, dst.copy(), X)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. rejections
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_the_destination_alone(pkg, gpu):
    src, dst = state_of("box", "src"), state_of("box", "dst")
    s_src, s_dst = scene_of(pkg, gpu, src), scene_of(pkg, gpu, dst)
    X = X_of("box")
    skew = X.copy()
    skew[:3, 0] *= 1.001
    nan = X.copy()
    nan[0, 3] = np.nan
    other_vs = gpu.create_scene(src.scene_params(pkg, voxel_size=np.nextafter(np.float32(am.VS), np.float32(1.0))))
    other_mu = gpu.create_scene(src.scene_params(pkg, mu=np.nextafter(np.float32(am.MU), np.float32(1.0))))
    swapping = gpu.create_scene(src.scene_params(pkg, use_swapping=1))
    sharded = gpu.create_scene(src.scene_params(pkg))
    gpu._call("scene_set_shard", sharded.ptr, 0, 2, 256)
    cases = [("src == dst", s_dst, s_dst, X), ("voxel_size", other_vs, s_dst, X), ("mu", other_mu, s_dst, X),
             ("swapping source", swapping, s_dst, X), ("sharded source", sharded, s_dst, X),
             ("not orthonormal", s_src, s_dst, skew), ("not finite", s_src, s_dst, nan)]
    for what, a, b, T in cases:
        with pytest.raises(pkg.DslamError):
            gpu.merge_maps(a, b, T)
        assert not dst.differences(rm.State.download(gpu, s_dst, dst)), f"{what}: the destination changed"
    for what, target in (("swapping destination", swapping), ("sharded destination", sharded)):
        before = rm.State.download(gpu, target, src)
        with pytest.raises(pkg.DslamError):
            gpu.merge_maps(s_src, target, X)
        assert not before.differences(rm.State.download(gpu, target, src)), f"{what}: the destination changed"
    with pytest.raises(pkg.DslamError):
        gpu.merge_maps(s_src, s_dst, X, pkg.MergeParams(max_passes=-1))
    assert not dst.differences(rm.State.download(gpu, s_dst, dst))


# ---------------------------------------------------------------------------------------------------------------------
# 10. with_colour = 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("identity", [True, False])
def test_without_colour_every_colour_half_stays(pkg, gpu, identity):
    a, b = plane_maps()
    src, dst = rm.State.of_map(a), rm.State.of_map(a).copy()
    dst.vba["clr"][:, :, 1] = 77
    X = I4 if identity else fx.off_lattice(1.5, 0.45)
    res, ref, got, _ = check_merge(pkg, gpu, "with_colour = 0", src, dst, X, with_colour=0)
    assert got.vba["clr"].tobytes() == dst.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == dst.vba["w_color"].tobytes()
    assert res["voxels_changed"] > 10000
    res, ref, got2, _ = check_merge(pkg, gpu, "with_colour = 1", src, dst, X)
    assert got2.vba["clr"].tobytes() != dst.vba["clr"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 10b. weights that vary from voxel to voxel: the smallest of the taps' weights, the 8-tap gate, the colour gate
# ---------------------------------------------------------------------------------------------------------------------
def _shift(v):
    X = np.eye(4, dtype=np.float32)
    X[:3, 3] = np.asarray(v, np.float64) * am.VS
    return X


@pytest.mark.parametrize("with_colour", [1, 0])
@pytest.mark.parametrize("how", ["identity", "translation", "off_lattice"])
def test_weights_that_vary_per_voxel(pkg, gpu, how, with_colour):
    """The plane pair re-weighted (weighted_fixtures.weighted_planes): source w_depth 1 .. 7 with one voxel in 37 unobserved
    inside its blocks and w_color 0 .. 3, destination w_depth up to 99.  Byte for byte against ref_merge.py as every case,
    and on the merged bytes themselves the weight law voxel by voxel (weighted_fixtures.merge_outcomes): w_depth' =
    min(w_dst + the smallest of the taps' w_depth, max_w), nothing where a tap weighs nothing, the colour half live exactly
    where every tap has a w_color -- with at least 1000 voxels of each outcome, so none can go missing."""
    a, b = wf.weighted_planes()
    X = {"identity": I4, "translation": _shift((3, -5, 2)), "off_lattice": fx.off_lattice(1.5, 0.45)}[how]
    src, dst = rm.State.of_map(a), rm.State.of_map(b)
    res, ref, got, _ = check_merge(pkg, gpu, f"weighted planes, {how}, with_colour = {with_colour}", src, dst, X,
                                   with_colour=with_colour)
    counts = wf.merge_outcomes(a, dst, got, X, with_colour)
    print(counts)
    assert counts["changed"] == res["voxels_changed"] and counts["clamped"] > 0 and got.vba["w_depth"].max() == 100
    assert counts["changed"] >= 1000 and counts["gated"] >= 1000
    if with_colour:
        assert counts["colour_live"] >= 1000 and counts["colour_idle"] >= 1000
    else:
        assert counts["colour_live"] == 0
        assert got.vba["clr"].tobytes() == dst.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == dst.vba["w_color"].tobytes()


def test_targets_outside_the_table_are_counted_and_skipped(pkg, gpu):
    m = fx.box_pair("small").src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:6]
    pos = np.array([[32767 - i, -32768 + i, 100 + (i & 1)] for i in range(6)])   # a diagonal that ends in the table's corner
    edge = am.Map(m.vs, m.mu, pos, m.voxels[pick], 0x400, 0x100, 0x100, m.geom)
    for shift in ((8, 0, 0), (0, -9, 0), (3, -5, 2)):
        X = np.eye(4, dtype=np.float32)
        X[:3, 3] = np.asarray(shift, np.float64) * am.VS
        res, ref, got, _ = check_merge(pkg, gpu, f"edge of the table, shift {shift}", rm.State.of_map(edge), rm.State.of_map(edge), X)
        assert 0 < res["out_of_range"] < res["src_candidates"]


def test_max_passes_stops_the_loop(pkg, gpu):
    res, ref, got, _ = check_merge(pkg, gpu, "max_passes = 2", state_of("box", "src"), state_of("box", "dst"), X_of("box"), max_passes=2)
    assert res["passes"] == 2 and res["exhausted"] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 11. / 12. the ITMLib mirror, and the merged map against the composite image
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


def test_mirror_merge_local_map_equals_abi(pkg, gpu, synth, tmp_path):
    """merge_harness: two S-tiny maps of the same keyframes, the second displaced by D without its estimatedGlobalPose
    knowing; AlignLocalMap(1, 0), then MergeLocalMap(1, 0).  Map 0 afterwards holds the bytes the same calls give through
    the Python binding on maps re-fused through the C ABI.  Recorded, not thresholded beyond "finite and covered": the
    merged map's depth image against the composite image of both maps before the merge."""
    Wm, Hm, n_frames, stride = 80, 60, 4, 4
    wl = synth.s_tiny(Wm, Hm)
    p = util.small_params(pkg, wl)
    vs = wl.scene_kwargs["voxel_size"]
    D = rr.rigid(5e-3, fx.AXIS, np.array([0.6, -0.64, 0.48]) * vs).astype(np.float32)
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
    T_dst, T_src = (np.frombuffer(raw, np.float32, 16, 64 * k) for k in range(2))
    fused = np.frombuffer(raw, np.float32, 16 * 2 * n_frames, 128).reshape(2, n_frames, 4, 4).transpose(0, 1, 3, 2)
    at = 128 + 64 * 2 * n_frames
    reg_h = pkg.RegisterResult.from_buffer_copy(raw[at:at + 32]); at += 32
    aligned, = struct.unpack_from("<i", raw, at); at += 4
    mres_h = pkg.MergeResult.from_buffer_copy(raw[at:at + 48]); at += 48
    merged_ok, = struct.unpack_from("<i", raw, at); at += 4
    npix = wl.W * wl.H
    depth_both = np.frombuffer(raw, np.float32, npix, at).reshape(wl.H, wl.W); at += 4 * npix
    depth_merged = np.frombuffer(raw, np.float32, npix, at).reshape(wl.H, wl.W); at += 4 * npix
    last_free, last_free_ex = struct.unpack_from("<2i", raw, at); at += 8
    n_entries = p.num_buckets + p.num_excess
    table = np.frombuffer(raw, am.HASH_ENTRY_DTYPE, n_entries, at); at += 16 * n_entries
    alloc = np.frombuffer(raw, np.int32, p.num_local_blocks, at); at += 4 * p.num_local_blocks
    excess = np.frombuffer(raw, np.int32, p.num_excess, at); at += 4 * p.num_excess
    vba = np.frombuffer(raw, am.VOXEL_DTYPE, p.num_local_blocks * 512, at); at += 8 * 512 * p.num_local_blocks
    assert at == len(raw)
    through_mirror = rm.State(table, alloc, last_free, excess, last_free_ex, vba, p.num_buckets, p.voxel_size, p.mu, p.max_w)
    assert aligned == 1 and reg_h.stop_reason == 0, run.stdout

    # the same calls through the Python binding (map 0 is the destination, map 1 the source)
    made = []
    view = gpu.create_view(wl.W, wl.H)
    for k in range(2):
        scene = gpu.create_scene(p)
        rs = gpu.create_render_state(scene, wl.W, wl.H)
        for i, (rgba, mm, _) in enumerate(frames):
            gpu.view_update(view, rgba, mm, timestamp=float(i))
            gpu.process_frame(scene, view, rs, fused[k, i], wl.intr)
        made.append(scene)
    X0 = np.array(_rigid_product(_as_doubles(T_dst), _rigid_inverse(_as_doubles(T_dst))), np.float64).astype(np.float32).reshape(4, 4).T
    X, reg = gpu.register_maps(made[1], made[0], X0)
    assert bytes(reg) == bytes(reg_h)
    T_after = np.array(_rigid_product(_rigid_inverse(_as_doubles(pkg.mat_to_abi(X))), _as_doubles(T_dst)), np.float64).astype(np.float32)
    assert T_after.tobytes() == T_src.tobytes()
    Xm = np.array(_rigid_product(_as_doubles(T_dst), _rigid_inverse(_as_doubles(T_after))), np.float64).astype(np.float32).reshape(4, 4).T
    src_state = rm.State.download(gpu, made[1], through_mirror)
    before = rm.State.download(gpu, made[0], through_mirror)
    mres = gpu.merge_maps(made[1], made[0], Xm)
    through_abi = rm.State.download(gpu, made[0], through_mirror)
    assert bytes(mres) == bytes(mres_h) and merged_ok == 1 and mres.exhausted == 0
    assert not through_mirror.differences(through_abi)
    assert mres.blocks_touched > 100 and mres.voxels_changed > 10000
    # ... and both are what the law says for these maps
    want = before.copy()
    ref = rm.merge(src_state, want, Xm)
    assert not want.differences(through_abi) and ref == mres.as_dict()

    # 12. the merged map alone against both maps in one image, from the first keyframe's pose
    assert np.isfinite(depth_both).all() and np.isfinite(depth_merged).all()
    both = (depth_both > 0) & (depth_merged > 0)
    share = both.mean()
    delta = np.abs(depth_both[both] - depth_merged[both]) / p.voxel_size
    print(f"{run.stdout.strip()}\nmerged map against the composite image: {share:.3f} of the pixels in both "
          f"({(depth_both > 0).mean():.3f} composite, {(depth_merged > 0).mean():.3f} merged), median |depth difference| "
          f"{np.median(delta):.4f} voxels, 95th percentile {np.percentile(delta, 95):.4f}")
    assert share > 0.5 * (depth_both > 0).mean() > 0.05
