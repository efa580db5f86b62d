"""dslam_unmerge_maps and dslam_remerge_maps on the MI355X against the sequential restatement of their law in
ref_unmerge.py.  In every case the destination's hash table, both free lists with their tops, every voxel block and every
field of the result are compared byte for byte: the law is float32 with a fixed operation order and contraction is off on
both sides, so there is no tolerance anywhere in this file.  The round trip merge -> unmerge is held, on the device's bytes,
to the bound ref_unmerge.py derives."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64_register as rr
import ref_merge as rm
import ref_unmerge as ru
import register_fixtures as fx
import unmerge_fixtures as uf
import util

pytestmark = pytest.mark.gpu

I4 = fx.I4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "unmerge_harness")
W, H = 80, 60
INTR = (100.0, 100.0, 40.0, 30.0)
PAIRS = {"box": lambda: fx.box_pair("small"), "holes": fx.holes_pair, "negative": fx.negative_pair}


def scene_of(pkg, api, st):
    scene = api.create_scene(st.scene_params(pkg))
    st.upload(api, scene)
    return scene


def check_unmerge(pkg, gpu, what, src, dst, X, with_colour=1, engine=None):
    """One unmerge on the device and in the reference; returns (result, reference result, the state after, scenes)."""
    api = engine or gpu
    s_src, s_dst = scene_of(pkg, api, src), scene_of(pkg, api, dst)
    params = None if with_colour else pkg.UnmergeParams(with_colour=0)
    res = api.unmerge_maps(s_src, s_dst, X, params).as_dict()
    got = rm.State.download(api, s_dst, dst)
    want = dst.copy()
    ref = ru.unmerge(src, want, X, with_colour=with_colour)
    print(f"{what}: {ref}")
    diff = want.differences(got)
    assert not diff, f"{what}: the destination differs from the reference in {diff}"
    assert res == ref, f"{what}: result {res}, reference {ref}"
    assert not src.differences(rm.State.download(api, s_src, src)), f"{what}: the source changed"
    # nothing but voxel blocks may have been written
    assert got.hash.tobytes() == dst.hash.tobytes() and got.alloc_list.tobytes() == dst.alloc_list.tobytes()
    assert got.excess_list.tobytes() == dst.excess_list.tobytes() and (got.last_free, got.last_free_ex) == (dst.last_free, dst.last_free_ex)
    return res, ref, got, (s_src, s_dst)


def shift(v):
    X = np.eye(4, dtype=np.float32)
    X[:3, 3] = np.asarray(v, np.float64) * am.VS
    return X


@functools.lru_cache(maxsize=None)
def state_of(kind, side):
    pair = PAIRS[kind]()
    return rm.State.of_map(pair.src_map if side == "src" else pair.dst_map)


def X_of(kind):
    return PAIRS[kind]().X_true.astype(np.float32)


def merged_with(src, dst, X, with_colour=1):
    """(a copy of `dst` with `src` merged in by the reference, the merge's result)."""
    out = dst.copy()
    return out, rm.merge(src, out, X, with_colour=with_colour)


def empty_like(m, num_buckets=0x400):
    n = len(m.block_pos)
    return rm.State.empty(num_buckets, max(0x100, 2 * n) + (-(num_buckets + max(0x100, 2 * n))) % 16, 4 * n)


# ---------------------------------------------------------------------------------------------------------------------
# 1. identity onto a destination the merge filled from empty; 13. the follow-up
# ---------------------------------------------------------------------------------------------------------------------
def test_identity_empties_what_the_merge_filled_and_the_follow_up(pkg, gpu):
    src = state_of("box", "src")
    before = empty_like(fx.box_pair("small").src_map)
    merged, mres = merged_with(src, before, I4)
    assert mres["blocks_allocated"] == 268
    s_src, s_dst = scene_of(pkg, gpu, src), scene_of(pkg, gpu, merged)
    rs_memo = gpu.create_render_state(s_dst, W, H)
    seen = gpu.get_image(s_dst, rs_memo, I4, INTR, pkg.IMAGE_DEPTH).copy()
    res = gpu.unmerge_maps(s_src, s_dst, I4).as_dict()
    got = rm.State.download(gpu, s_dst, merged)
    want = merged.copy()
    assert res == ru.unmerge(src, want, I4) and not want.differences(got)
    assert res["voxels_changed"] == res["src_candidates"] == 268 * 512 and res["blocks_touched"] == 268
    # every voxel is empty again, the blocks are still allocated, table and pools are the merged state's
    assert (got.vba.view(np.uint64) == np.uint64(32767)).all()
    assert got.hash.tobytes() == merged.hash.tobytes() and (got.last_free, got.last_free_ex) == (merged.last_free, merged.last_free_ex)
    assert got.alloc_list.tobytes() == merged.alloc_list.tobytes() and got.excess_list.tobytes() == merged.excess_list.tobytes()
    assert len(got.live()) == 268
    # GetImage with the same render state and pose: the memo was dropped
    gone = gpu.get_image(s_dst, rs_memo, I4, INTR, pkg.IMAGE_DEPTH).copy()
    assert (seen > 0).sum() > 100 and not (gone > 0).any()
    # ProcessFrame + GetImage on the unmerged scene against the same calls on a fresh scene loaded with the downloaded state
    fresh = scene_of(pkg, gpu, got)
    rgba = np.full((H, W, 4), 200, np.uint8)
    depth = np.full((H, W), 480, np.int16)
    out = []
    for scene in (s_dst, fresh):
        rs, view = gpu.create_render_state(scene, W, H), gpu.create_view(W, H)
        first = gpu.get_image(scene, rs, I4, INTR, pkg.IMAGE_DEPTH).copy()
        gpu.view_update(view, rgba, depth)
        gpu.process_frame(scene, view, rs, I4, INTR)
        image = gpu.get_image(scene, rs, I4, INTR, pkg.IMAGE_DEPTH).copy()
        out.append((first, image, rm.State.download(gpu, scene, got), gpu.download_visible_ids(rs)))
    (b0, i0, st0, v0), (b1, i1, st1, v1) = out
    assert b0.tobytes() == b1.tobytes() and not st1.differences(st0), f"ProcessFrame after the unmerge differs: {st1.differences(st0)}"
    assert np.array_equal(v0, v1) and i0.tobytes() == i1.tobytes() and (i0 > 0).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------
# 2. identity and whole-voxel translations onto an overlapping destination, colour on either side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coloured", ["source", "destination"])
@pytest.mark.parametrize("how", ["identity", (8, 0, 0), (3, -5, 2)])
def test_identity_and_whole_voxel_translations(pkg, gpu, how, coloured):
    a, b = uf.plane_maps(40)
    src, dst = (a, b) if coloured == "source" else (b, a)
    X = I4 if how == "identity" else shift(how)
    merged, mres = merged_with(src, dst, X)
    assert merged.vba["w_depth"].max() == 43 and mres["blocks_allocated"] > 0
    res, ref, got, _ = check_unmerge(pkg, gpu, f"{how}, colour in the {coloured}", src, merged, X)
    fig = ru.check_round_trip(f"{how}, colour in the {coloured}", src, dst, merged, got, X)
    assert res["voxels_changed"] == mres["voxels_changed"] > 10000 and fig["worst_sdf"] <= ru.depth_bound(3, 40)
    if coloured == "destination":   # the source has no colour to take out: every colour half idles
        assert got.vba["clr"].tobytes() == merged.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == merged.vba["w_color"].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rigid transforms after a merge on the device under the same X: the round trip on the device's bytes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "holes", "negative"])
def test_rigid_transform_round_trip(pkg, gpu, kind):
    src, dst, X = state_of(kind, "src"), state_of(kind, "dst"), X_of(kind)
    s_src, s_dst = scene_of(pkg, gpu, src), scene_of(pkg, gpu, dst)
    mres = gpu.merge_maps(s_src, s_dst, X).as_dict()
    merged = rm.State.download(gpu, s_dst, dst)
    want, ref_m = merged_with(src, dst, X)
    assert mres == ref_m and not want.differences(merged)
    res = gpu.unmerge_maps(s_src, s_dst, X).as_dict()
    got = rm.State.download(gpu, s_dst, dst)
    ref = ru.unmerge(src, want, X)
    assert not want.differences(got), f"{kind}: the destination differs from the reference in {want.differences(got)}"
    assert res == ref, f"{kind}: result {res}, reference {ref}"
    assert not src.differences(rm.State.download(gpu, s_src, src))
    fig = ru.check_round_trip(kind, src, dst, merged, got, X)
    print(f"{kind}: {res}\n  round trip on the device's bytes {fig}")
    assert res["candidates_without_block"] == res["depth_underweight"] == res["colour_underweight"] == 0
    assert res["voxels_changed"] == mres["voxels_changed"] and fig["worst_sdf"] <= 3 and fig["created"] > 200
    if kind == "holes":
        assert src.num_buckets == 0x40       # the source's chains


# ---------------------------------------------------------------------------------------------------------------------
# 4. weights that vary per voxel; 11. with_colour = 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colour", [1, 0])
@pytest.mark.parametrize("how", ["identity", "off_lattice"])
def test_weights_that_vary_per_voxel(pkg, gpu, how, with_colour):
    src, _, twin = uf.unclamped_planes()
    X = I4 if how == "identity" else fx.off_lattice(1.5, 0.45)
    merged, mres = merged_with(src, twin, X, with_colour)
    assert merged.vba["w_depth"].max() < 100
    what = f"weighted planes, {how}, with_colour = {with_colour}"
    res, ref, got, _ = check_unmerge(pkg, gpu, what, src, merged, X, with_colour=with_colour)
    fig = ru.check_round_trip(what, src, twin, merged, got, X, with_colour)
    print(fig)
    assert res["voxels_changed"] == mres["voxels_changed"] > 10000 and fig["observed"] > 10000
    if with_colour:
        assert fig["coloured"] > 10000 and got.vba["clr"].tobytes() != merged.vba["clr"].tobytes()
    else:                                   # every colour half as it was
        assert got.vba["clr"].tobytes() == merged.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == merged.vba["w_color"].tobytes()


def test_without_colour_a_merged_colour_stays(pkg, gpu):
    """Merged with colour, unmerged without: the depth halves return, every colour half stays as the merge left it."""
    src, _, twin = uf.unclamped_planes()
    X = fx.off_lattice(1.5, 0.45)
    merged, _ = merged_with(src, twin, X, 1)
    res, ref, got, _ = check_unmerge(pkg, gpu, "merged with colour, unmerged without", src, merged, X, with_colour=0)
    assert got.vba["clr"].tobytes() == merged.vba["clr"].tobytes() and got.vba["w_color"].tobytes() == merged.vba["w_color"].tobytes()
    assert np.array_equal(got.vba["w_depth"], twin.vba["w_depth"]) and res["voxels_changed"] > 10000


# ---------------------------------------------------------------------------------------------------------------------
# 5. no merge beforehand: a destination lighter than the source
# ---------------------------------------------------------------------------------------------------------------------
def test_a_lighter_destination_is_counted_and_left_alone(pkg, gpu):
    a, _ = uf.plane_maps(40)
    src, dst = a.copy(), a.copy()
    src.vba["w_depth"] = np.where(a.vba["w_depth"] > 0, 5, 0)
    src.vba["w_color"] = np.where(a.vba["w_depth"] > 0, 3, 0)
    lin = np.arange(512)[None, :]
    dst.vba["w_depth"] = np.where(a.vba["w_depth"] > 0, 2 + 6 * (lin % 2), 0)        # 2 (too light) and 8
    dst.vba["w_color"] = np.where(a.vba["w_depth"] > 0, 1 + 4 * ((lin >> 1) % 2), 0)   # 1 (too light) and 5
    for X in (I4, fx.off_lattice(1.5, 0.45)):
        res, ref, got, _ = check_unmerge(pkg, gpu, "lighter destination", src, dst, X)
        assert res["depth_underweight"] > 5000 and res["colour_underweight"] > 5000 and res["voxels_changed"] > 5000
        light = dst.vba["w_depth"] == 2
        assert got.vba["sdf"][light].tobytes() == dst.vba["sdf"][light].tobytes() and (got.vba["w_depth"][light] == 2).all()
        light = dst.vba["w_color"] == 1
        assert got.vba["clr"][light].tobytes() == dst.vba["clr"][light].tobytes() and (got.vba["w_color"][light] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a destination that lacks target blocks: nothing is allocated
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_target_blocks_are_counted_and_nothing_is_allocated(pkg, gpu):
    src, dst = uf.uniform(state_of("box", "src"), 1), uf.uniform(state_of("box", "dst"), 5)
    res, ref, got, _ = check_unmerge(pkg, gpu, "missing blocks", src, dst, X_of("box"))
    assert res["candidates_without_block"] > 1000 and res["blocks_touched"] == 448 - 124 and res["voxels_changed"] > 50000
    assert len(got.live()) == len(dst.live())


# ---------------------------------------------------------------------------------------------------------------------
# 7. targets outside the table
# ---------------------------------------------------------------------------------------------------------------------
def test_targets_outside_the_table_are_counted_and_skipped(pkg, gpu):
    m = fx.box_pair("small").src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:6]
    pos = np.array([[32767 - i, -32768 + i, 100 + (i & 1)] for i in range(6)])   # a diagonal that ends in the table's corner
    edge = rm.State.of_map(am.Map(m.vs, m.mu, pos, m.voxels[pick], 0x400, 0x100, 0x100, m.geom))
    for v in ((8, 0, 0), (0, -9, 0), (3, -5, 2)):
        res, ref, got, _ = check_unmerge(pkg, gpu, f"edge of the table, shift {v}", edge, uf.uniform(edge, 3), shift(v))
        assert 0 < res["out_of_range"] < res["src_candidates"]


# ---------------------------------------------------------------------------------------------------------------------
# 8. grid coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_more_touched_blocks_than_the_grid_then_five(pkg, gpu):
    big = fx.sphere_pair()
    n_big = len(big.dst_map.block_pos)
    assert 512 < n_big < 1024                  # the block kernel's grid has 512 workgroups
    whole = rm.State.of_map(big.dst_map)
    res, ref, got, _ = check_unmerge(pkg, gpu, f"{n_big} blocks", whole, uf.uniform(whole, 3), fx.off_lattice(1.5, 0.45))
    assert res["blocks_touched"] > 512 and res["voxels_changed"] > 100000
    m = fx.box_pair("small").src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:5]
    few = rm.State.of_map(am.Map(m.vs, m.mu, m.block_pos[pick], m.voxels[pick], 0x400, 0x100, 0x100, m.geom))
    res, ref, got, _ = check_unmerge(pkg, gpu, "5 blocks", few, uf.uniform(few, 2), I4)
    assert res["blocks_touched"] == 5 and res["voxels_changed"] == 5 * 512


# ---------------------------------------------------------------------------------------------------------------------
# 9. repeatability, the asynchronous engine
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_an_asynchronous_engine_give_the_same_bytes(pkg, gpu, synth):
    src, X = state_of("holes", "src"), X_of("holes")
    merged, _ = merged_with(src, state_of("holes", "dst"), X)
    _, ref, first, _ = check_unmerge(pkg, gpu, "first", src, merged, X)
    _, _, second, _ = check_unmerge(pkg, gpu, "second", src, merged, X)
    assert not first.differences(second)
    eng = pkg.open_engine(0)
    try:
        eng.set_async(True)
        wl = synth.s_tiny()
        busy = eng.create_scene(pkg.SceneParams(num_local_blocks=0x2000, num_buckets=0x4000, num_excess=0x800, **wl.scene_kwargs))
        rs, view = eng.create_render_state(busy, wl.W, wl.H), eng.create_view(wl.W, wl.H)
        rgba, mm, M = wl.frame(0)
        eng.view_update(view, rgba, mm)
        s_src, s_dst = scene_of(pkg, eng, src), scene_of(pkg, eng, merged)
        eng.process_frame(busy, view, rs, M, wl.intr)          # a fusion in flight when the unmerge is called
        res = eng.unmerge_maps(s_src, s_dst, X).as_dict()
        third = rm.State.download(eng, s_dst, merged)
        assert not first.differences(third) and res == ref
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. rejections
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
            gpu.unmerge_maps(a, b, T)
        with pytest.raises(pkg.DslamError):
            gpu.remerge_maps(a, b, T, X)
        with pytest.raises(pkg.DslamError):
            gpu.remerge_maps(a, b, I4, T)          # the second half is checked before the first half runs
        assert not dst.differences(rm.State.download(gpu, s_dst, dst)), f"{what}: the destination changed"
    for what, target in (("swapping destination", swapping), ("sharded destination", sharded)):
        before = rm.State.download(gpu, target, src)
        with pytest.raises(pkg.DslamError):
            gpu.unmerge_maps(s_src, target, X)
        with pytest.raises(pkg.DslamError):
            gpu.remerge_maps(s_src, target, I4, X)
        assert not before.differences(rm.State.download(gpu, target, src)), f"{what}: the destination changed"
    with pytest.raises(pkg.DslamError):
        gpu.remerge_maps(s_src, s_dst, I4, X, pkg.MergeParams(max_passes=-1))
    assert not dst.differences(rm.State.download(gpu, s_dst, dst))


# ---------------------------------------------------------------------------------------------------------------------
# 12. the remerge
# ---------------------------------------------------------------------------------------------------------------------
def test_remerge_from_a_wrong_transform_to_the_truth(pkg, gpu):
    pair = fx.box_pair("small")
    src, dst = state_of("box", "src"), state_of("box", "dst")
    X_new = X_of("box")
    X_old = (pair.X_true @ fx.off_lattice().astype(np.float64)).astype(np.float32)
    merged, _ = merged_with(src, dst, X_old)
    s_src, s_one, s_two = scene_of(pkg, gpu, src), scene_of(pkg, gpu, merged), scene_of(pkg, gpu, merged)
    un, re = gpu.remerge_maps(s_src, s_one, X_old, X_new)
    one = rm.State.download(gpu, s_one, merged)
    want = merged.copy()
    ref_un, ref_re = ru.remerge(src, want, X_old, X_new)
    print(f"remerge: {ref_un}\n  {ref_re}")
    assert not want.differences(one), f"the remerged destination differs from the reference in {want.differences(one)}"
    assert un.as_dict() == ref_un and re.as_dict() == ref_re
    un2 = gpu.unmerge_maps(s_src, s_two, X_old)
    re2 = gpu.merge_maps(s_src, s_two, X_new)
    two = rm.State.download(gpu, s_two, merged)
    assert not one.differences(two) and bytes(un) == bytes(un2) and bytes(re) == bytes(re2)
    assert un.voxels_changed > 50000 and re.voxels_changed > 50000 and re.blocks_allocated > 0
    assert not src.differences(rm.State.download(gpu, s_src, src))
    # with_colour = 0 goes to both halves
    s_three = scene_of(pkg, gpu, merged)
    un3, re3 = gpu.remerge_maps(s_src, s_three, X_old, X_new, pkg.MergeParams(with_colour=0))
    want = merged.copy()
    ref_un, ref_re = ru.remerge(src, want, X_old, X_new, with_colour=0)
    assert not want.differences(rm.State.download(gpu, s_three, merged)) and un3.as_dict() == ref_un and re3.as_dict() == ref_re
    # bit-identical transforms: nothing is done
    un0, re0 = gpu.remerge_maps(s_src, s_one, X_new, X_new.copy())
    assert un0.as_dict() == ru.ZERO_UNMERGE and re0.as_dict() == ru.ZERO_MERGE
    assert not one.differences(rm.State.download(gpu, s_one, merged))


# ---------------------------------------------------------------------------------------------------------------------
# 14. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_unmerge_and_remerge_equal_abi(pkg, gpu, synth, tmp_path):
    """unmerge_harness: two S-tiny maps of the same keyframes, the second displaced by D without its estimatedGlobalPose
    knowing; MergeLocalMap(1, 0), UnmergeLocalMap(1, 0, X_old); merged again, the pose corrected, RemergeLocalMap(1, 0,
    X_old).  Map 0 holds, both times, the bytes the same calls give through the Python binding on maps re-fused through
    the C ABI."""
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
    n_entries = p.num_buckets + p.num_excess

    def read_map(at):
        last_free, last_free_ex = struct.unpack_from("<2i", raw, at); at += 8
        table = np.frombuffer(raw, am.HASH_ENTRY_DTYPE, n_entries, at); at += 16 * n_entries
        alloc = np.frombuffer(raw, np.int32, p.num_local_blocks, at); at += 4 * p.num_local_blocks
        excess = np.frombuffer(raw, np.int32, p.num_excess, at); at += 4 * p.num_excess
        vba = np.frombuffer(raw, am.VOXEL_DTYPE, p.num_local_blocks * 512, at); at += 8 * 512 * p.num_local_blocks
        return rm.State(table, alloc, last_free, excess, last_free_ex, vba, p.num_buckets, p.voxel_size, p.mu, p.max_w), at

    X_old = np.frombuffer(raw, np.float32, 16, 0).reshape(4, 4).T
    fused = np.frombuffer(raw, np.float32, 16 * 2 * n_frames, 64).reshape(2, n_frames, 4, 4).transpose(0, 1, 3, 2)
    at = 64 + 64 * 2 * n_frames
    m1_h = pkg.MergeResult.from_buffer_copy(raw[at:at + 48]); at += 48
    u1_h = pkg.UnmergeResult.from_buffer_copy(raw[at:at + 56]); at += 56
    unmerged_ok, = struct.unpack_from("<i", raw, at); at += 4
    mirror_unmerged, at = read_map(at)
    X_new = np.frombuffer(raw, np.float32, 16, at).reshape(4, 4).T; at += 64
    u2_h = pkg.UnmergeResult.from_buffer_copy(raw[at:at + 56]); at += 56
    m2_h = pkg.MergeResult.from_buffer_copy(raw[at:at + 48]); at += 48
    remerged_ok, = struct.unpack_from("<i", raw, at); at += 4
    mirror_remerged, at = read_map(at)
    assert at == len(raw)
    assert X_old.tobytes() != X_new.tobytes()

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
    src_state = rm.State.download(gpu, made[1], mirror_unmerged)
    before = rm.State.download(gpu, made[0], mirror_unmerged)
    m1 = gpu.merge_maps(made[1], made[0], X_old)
    merged = rm.State.download(gpu, made[0], mirror_unmerged)
    u1 = gpu.unmerge_maps(made[1], made[0], X_old)
    abi_unmerged = rm.State.download(gpu, made[0], mirror_unmerged)
    assert bytes(m1) == bytes(m1_h) and bytes(u1) == bytes(u1_h) and unmerged_ok == 1
    assert not mirror_unmerged.differences(abi_unmerged)
    assert u1.blocks_touched > 100 and u1.voxels_changed == m1.voxels_changed > 10000
    fig = ru.check_round_trip("mirror", src_state, before, merged, abi_unmerged, X_old)
    print(f"{run.stdout.strip()}\nround trip of the fused maps: {fig}")
    gpu.merge_maps(made[1], made[0], X_old)
    u2, m2 = gpu.remerge_maps(made[1], made[0], X_old, X_new)
    abi_remerged = rm.State.download(gpu, made[0], mirror_unmerged)
    assert bytes(u2) == bytes(u2_h) and bytes(m2) == bytes(m2_h) and remerged_ok == 1 and m2.exhausted == 0
    assert not mirror_remerged.differences(abi_remerged)
    assert m2.voxels_changed > 10000
