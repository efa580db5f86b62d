"""dslam_get_image_multi on the MI355X: exact reductions to dslam_get_image, one posed map, the blending law against
the float64 reference of ref64_multimap.py, maps side by side, argument checks, the GetImage memo and async mode, and
the ITMLib mirror's GetImageAllLocalMaps."""
import os
import struct
import subprocess

import numpy as np
import pytest

import analytic_maps as am
import ref64
import ref64_checks as rc
import ref64_multimap as rm
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "denseslam-global-consistency-h_amd", "itmlib", "tests", "multimap_harness")
TYPES = ("IMAGE_SHADED", "IMAGE_COLOUR_FROM_VOLUME", "IMAGE_COLOUR_FROM_NORMAL", "IMAGE_DEPTH")
I4 = np.eye(4, dtype=np.float32)


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """A rigid world -> map transform (metres)."""
    R = np.linalg.inv(rc.camera(8, 8, yaw=yaw, pitch=pitch, roll=roll)[0].astype(np.float64))[:3, :3]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


def fused_room(api, pkg, synth):
    wl = synth.s_tiny()
    scene, rs, _ = util.run_sequence(api, pkg, wl, util.small_params(pkg, wl), 5)
    return wl, scene, rs


def far_map(api, pkg, m):
    """Map `m` placed 100 m to the side of every camera of these tests."""
    return upload_map(api, pkg, m), pose(t=(100.0, 0.0, 0.0))


def roomiest(api, scenes, W, H):
    """A render state whose visible-list capacity covers every scene of the list."""
    return api.create_render_state(max(scenes, key=lambda s: s.params.num_local_blocks), W, H)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact reductions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fused_room", "analytic"])
@pytest.mark.parametrize("extra", ["alone", "empty", "far"])
def test_exact_reduction_to_get_image(pkg, gpu, synth, source, extra):
    if source == "fused_room":
        wl, A, rs = fused_room(gpu, pkg, synth)
        W, H = wl.W, wl.H
        M, intr = wl.frame(4)[2], wl.intr
        params = util.small_params(pkg, wl)
    else:
        W, H = 96, 72
        m = am.colour_plane()
        A = upload_map(gpu, pkg, m)
        rs = gpu.create_render_state(A, W, H)
        M, intr = rc.camera(W, H, yaw=0.05, pitch=0.03)
        params = m.scene_params(pkg)
    scenes, poses = [A], [I4]
    if extra == "empty":
        scenes.append(gpu.create_scene(params))
        poses.append(pose(yaw=0.3, t=(0.1, 0.0, -0.2)))
    elif extra == "far":
        if source == "fused_room":  # same voxel_size / mu as the room
            s, T = far_map(gpu, pkg, am.build_map(am.Sphere((0.0, 0.0, 0.5), 0.3), params.voxel_size, params.mu,
                                                  (-0.35, -0.35, 0.15), (0.35, 0.35, 0.85)))
        else:
            s, T = far_map(gpu, pkg, am.colour_plane())
        scenes.append(s)
        poses.append(T)
    rs2 = roomiest(gpu, scenes, W, H)
    for name in TYPES:
        t = getattr(pkg, name)
        want = gpu.get_image(A, rs, M, intr, t)
        got = gpu.get_image_multi(scenes, poses, rs2, M, intr, t)
        assert np.array_equal(want.view(np.uint8), got.view(np.uint8)), f"{name}: {np.sum(want != got)} pixels differ"
        if t == pkg.IMAGE_DEPTH:
            assert (got > 0).sum() > 0.1 * W * H


# ---------------------------------------------------------------------------------------------------------------------
# 2. one posed map
# ---------------------------------------------------------------------------------------------------------------------
def test_one_posed_map_equals_map_camera(pkg, gpu):
    W, H = 96, 72
    m = am.sphere_outside()
    A = upload_map(gpu, pkg, m)
    rs = gpu.create_render_state(A, W, H)
    M, intr = rc.camera(W, H, yaw=-0.1)
    T = pose(yaw=0.15, roll=0.05, t=(0.03, -0.02, 0.04))
    got = gpu.get_image_multi([A], [T], rs, M, intr, pkg.IMAGE_DEPTH).astype(np.float64)
    want = gpu.get_image(A, rs, rm.camera_of(M, T), intr, pkg.IMAGE_DEPTH).astype(np.float64)
    tie = rm.cast_rays([rm.Posed(m, T)], M, intr, W, H)["tie"]
    hit = got > 0
    assert np.array_equal(hit[~tie], (want > 0)[~tie])
    both = hit & (want > 0)
    assert both.sum() > 0.1 * W * H
    err = np.abs(got - want) / m.vs
    big = both & (err > 1e-3)
    assert not (big & ~tie).any(), f"|ddepth| up to {err[big & ~tie].max():.3g} voxel off a tie"
    assert big.sum() <= 0.01 * both.sum()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the blending law
# ---------------------------------------------------------------------------------------------------------------------
def _two_spheres():
    """One sphere seen by two local maps: radii two voxels apart, w_depth 5 / 20, w_color 1 / 3, a colour each, each
    built in its own frame under a non-trivial pose."""
    c_world, r = np.array([0.03, -0.02, 0.45]), 0.16
    T_a = pose(yaw=0.2, pitch=-0.1, t=(0.05, 0.02, -0.03))
    T_b = pose(yaw=-0.15, roll=0.2, t=(-0.04, 0.01, 0.06))
    maps = []
    for T, dr, wd, wc, clr in ((T_a, 0.0, 5, 1, (220.0, 40.0, 30.0)), (T_b, 2 * am.VS, 20, 3, (30.0, 90.0, 230.0))):
        c = T[:3, :3].astype(np.float64) @ c_world + T[:3, 3]
        m = am.build_map(am.Sphere(c, r + dr), am.VS, am.MU, c - 0.2, c + 0.2,
                         colour=lambda x, clr=clr: np.broadcast_to(np.array(clr), x.shape))
        maps.append(rm.Posed(rm.set_weights(m, wd, wc), T))
    return maps, c_world, r


def test_blending_law_against_float64(pkg, gpu):
    W, H = 96, 72
    maps, c_world, r = _two_spheres()
    scenes = [upload_map(gpu, pkg, pm.m) for pm in maps]
    Ts = [pm.T for pm in maps]
    rs = roomiest(gpu, scenes, W, H)
    M, intr = rc.camera(W, H, yaw=0.04)
    vs = am.VS
    ref = rm.cast_rays(maps, M, intr, W, H)
    depth = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_DEPTH).astype(np.float64)
    hit, tie = depth > 0, ref["tie"]
    assert np.array_equal(hit[~tie], ref["hit"][~tie])
    both = hit & ref["hit"]
    assert both.sum() > 0.1 * W * H
    dref = ref64.camera_depth(M, ref["p"], vs)
    err = np.abs(depth - dref) / vs
    big = both & (err > 1e-3)
    assert not (big & ~tie).any(), f"|ddepth| up to {err[big & ~tie].max():.3g} voxel off a tie"
    assert big.sum() <= 0.01 * both.sum()
    # the other laws a kernel could have: min of the depths, first map wins, unweighted mean -- each is far off
    single = []
    for pm in maps:
        Mi = rm.camera_of(M, pm.T)
        single.append(ref64.camera_depth(Mi, ref64.cast_rays(pm.m, Mi, intr, W, H)["p"], vs))
    sel = both & ~tie
    for name, alt in (("min of depths", np.minimum(*single)), ("first map wins", single[0])):
        assert np.median(np.abs(depth - alt)[sel]) / vs > 0.3, name
    eq = [rm.Posed(pm.m, pm.T) for pm in maps]
    for pm in eq:
        pm.w_depth = 1.0
    unweighted = ref64.camera_depth(M, rm.cast_rays(eq, M, intr, W, H)["p"], vs)
    assert np.median(np.abs(depth - unweighted)[sel]) / vs > 0.3, "unweighted mean"
    # shading and colour of the combined reads
    p_hit = ref["p"][sel]
    cand = ref["cand"][sel]
    n = rm.normals(maps, cand, p_hit)
    light = ref64.light_of(M)
    grey_ref = ref64.shaded_grey(n @ light)
    grey = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_SHADED)[sel][:, 0].astype(np.float64)
    ok = (n @ light) > 0.05
    assert ok.sum() > 0.5 * sel.sum()
    assert np.abs(grey - grey_ref)[ok].max() <= 2.0, np.abs(grey - grey_ref)[ok].max()
    clr_ref = np.trunc(rm.colours(maps, cand, p_hit))
    clr = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME)[sel][:, :3].astype(np.float64)
    assert np.abs(clr - clr_ref)[ok].max() <= 1.0, np.abs(clr - clr_ref)[ok].max()
    # the colour is the w_color-weighted mean (1 : 3) where both maps hold every tap
    both_maps = cand.all(1) & ok
    want = np.trunc((np.array([220.0, 40.0, 30.0]) + 3 * np.array([30.0, 90.0, 230.0])) / 4.0)
    assert (np.abs(clr[both_maps] - want) <= 1.0).all(axis=1).mean() > 0.9


# ---------------------------------------------------------------------------------------------------------------------
# 4. maps side by side
# ---------------------------------------------------------------------------------------------------------------------
def test_disjoint_maps_match_single_map_renders(pkg, gpu):
    W, H = 256, 128
    M, intr = rc.camera(W, H, f_scale=0.5)
    maps = []
    geom_world = am.Plane((0.0, 0.0, -1.0), -0.5)
    for k, x0 in enumerate((-0.5, -0.1, 0.3)):   # 0.2 m patches of one wall, 0.2 m apart
        T = pose(yaw=0.05 * k, t=(0.02 * k, 0.0, 0.01 * k))
        R = T[:3, :3].astype(np.float64)
        n = R @ geom_world.n
        c = geom_world.c + n @ T[:3, 3]
        corners = np.array([[x, y, z] for x in (x0, x0 + 0.2) for y in (-0.2, 0.2) for z in (0.45, 0.55)])
        local = corners @ R.T + T[:3, 3]
        m = am.build_map(am.Plane(n, c), am.VS, am.MU, local.min(0), local.max(0))
        maps.append(rm.Posed(m, T))
    scenes = [upload_map(gpu, pkg, pm.m) for pm in maps]
    rs = roomiest(gpu, scenes, W, H)
    depth = gpu.get_image_multi(scenes, [pm.T for pm in maps], rs, M, intr, pkg.IMAGE_DEPTH)
    _, mask = rm.front_end(maps, M, intr, W, H)
    nbits = mask.sum(-1)
    seam = nbits > 1
    band = seam.copy()  # a one-cell band around every cell two maps share
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            band |= np.roll(seam, (dy, dx), axis=(0, 1))
    checked = 0
    for i, pm in enumerate(maps):
        cells = mask[..., i] & (nbits == 1) & ~band
        px = np.kron(cells, np.ones((8, 8), bool))[:H, :W]
        rs_i = gpu.create_render_state(scenes[i], W, H)
        single = gpu.get_image(scenes[i], rs_i, rm.camera_of(M, pm.T), intr, pkg.IMAGE_DEPTH)
        agree = (depth[px] > 0) == (single[px] > 0)
        assert agree.mean() > 0.995
        h = px & (depth > 0) & (single > 0)
        assert np.percentile(np.abs(depth[h] - single[h]), 99) / am.VS < 1e-3
        checked += h.sum()
    assert checked > 0.15 * W * H


# ---------------------------------------------------------------------------------------------------------------------
# 5. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, gpu):
    W, H = 64, 48
    m = am.sphere_outside()
    A = upload_map(gpu, pkg, m)
    rs = gpu.create_render_state(A, W, H)
    M, intr = rc.camera(W, H)
    before = util.snapshot(gpu, A, rs)
    other_vs = upload_map(gpu, pkg, am.sphere_outside(), voxel_size=0.006)
    other_mu = upload_map(gpu, pkg, am.sphere_outside(), mu=0.03)
    small = gpu.create_scene(m.scene_params(pkg, num_local_blocks=m.num_local_blocks // 2))
    small_rs = gpu.create_render_state(small, W, H)
    cases = [
        ("voxel_size", [A, other_vs], [I4, I4], rs),
        ("mu", [A, other_mu], [I4, I4], rs),
        ("no maps", [], np.zeros((0, 4, 4), np.float32), rs),
        ("65 maps", [A] * 65, [I4] * 65, rs),
        ("singular", [A], [np.zeros((4, 4), np.float32)], rs),
        ("NULL scene", [A, None], [I4, I4], rs),
        ("render state too small", [A], [I4], small_rs),
    ]
    for what, scenes, poses, r in cases:
        with pytest.raises(pkg.DslamError, match="status -1 "):
            gpu.get_image_multi(scenes, poses, r, M, intr, pkg.IMAGE_DEPTH)
        util.assert_same_state(before, util.snapshot(gpu, A, rs), what)
    # 64 maps is the limit, not an error
    gpu.get_image_multi([A] * 64, [I4] * 64, rs, M, intr, pkg.IMAGE_DEPTH)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the GetImage memo, determinism, async mode
# ---------------------------------------------------------------------------------------------------------------------
def test_memo_determinism_and_async(pkg, gpu):
    W, H = 96, 72
    m = am.colour_plane()
    A = upload_map(gpu, pkg, m)
    B, T_b = far_map(gpu, pkg, am.colour_plane())
    M, intr = rc.camera(W, H, yaw=0.05)
    M2, _ = rc.camera(W, H, yaw=-0.08, t=(0.02, 0.0, 0.0))
    rs = gpu.create_render_state(A, W, H)
    first = gpu.get_image(A, rs, M, intr, pkg.IMAGE_SHADED)
    # a composite from another pose: a following get_image of the first view must march again
    gpu.get_image_multi([A, B], [I4, pose(yaw=0.1, t=(0.01, 0.0, 0.0))], rs, M2, intr, pkg.IMAGE_DEPTH)
    again = gpu.get_image(A, rs, M, intr, pkg.IMAGE_SHADED)
    fresh = gpu.get_image(A, gpu.create_render_state(A, W, H), M, intr, pkg.IMAGE_SHADED)
    assert np.array_equal(again, fresh) and np.array_equal(first, fresh)
    # two identical composite calls
    Ta = pose(yaw=0.1, t=(0.01, 0.0, 0.0))
    a = gpu.get_image_multi([A, B], [Ta, T_b], rs, M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME)
    b = gpu.get_image_multi([A, B], [Ta, T_b], rs, M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME)
    assert np.array_equal(a, b) and (a[..., 3] > 0).sum() > 0.1 * W * H
    want = gpu.get_image_multi([A, B], [Ta, T_b], rs, M, intr, pkg.IMAGE_DEPTH)
    # async engine, page-locked output: the kernel writes the image, the caller waits on the engine
    out = gpu.host_alloc((H, W), np.float32)
    try:
        gpu.set_async(True)
        gpu.get_image_multi([A, B], [Ta, T_b], rs, M, intr, pkg.IMAGE_DEPTH, out=out)
        gpu.synchronize()
        assert np.array_equal(np.asarray(out), want)
    finally:
        gpu.set_async(False)
        gpu.host_free(out)


def test_page_locked_output_equals_pageable(pkg, gpu, synth):
    """The composite render stored by the kernel itself into a page-locked caller image (host_alloc) against the same call
    into a pageable array (rendered into the render state's image, copied behind the kernel): the same bytes for all four
    image types, on the synchronous engine and on the async engine behind a fence.  Two fused maps of the 70 x 45 room (a
    width that is no multiple of the 8-pixel tile), the second under a rigid pose."""
    wl = synth.s_room(70, 45)
    W, H = wl.W, wl.H
    A, _, _ = util.run_sequence(gpu, pkg, wl, util.small_params(pkg, wl), 3)
    B, _, _ = util.run_sequence(gpu, pkg, wl, util.small_params(pkg, wl), 2)
    scenes, poses = [A, B], [I4, pose(yaw=0.04, t=(0.03, 0.0, -0.02))]
    M, intr = wl.frame(2)[2], wl.intr
    rs = roomiest(gpu, scenes, W, H)
    want = {name: gpu.get_image_multi(scenes, poses, rs, M, intr, getattr(pkg, name)).copy() for name in TYPES}
    assert (want["IMAGE_DEPTH"] > 0).sum() > 0.1 * W * H and (want["IMAGE_SHADED"][..., 3] > 0).sum() > 0.1 * W * H
    pinned = {name: gpu.host_alloc((H, W) if name == "IMAGE_DEPTH" else (H, W, 4),
                                   np.float32 if name == "IMAGE_DEPTH" else np.uint8) for name in TYPES}
    fence = gpu.fence_create()
    try:
        for is_async in (False, True):
            gpu.set_async(is_async)
            for name in TYPES:
                out = pinned[name]
                out[...] = 0
                gpu.get_image_multi(scenes, poses, rs, M, intr, getattr(pkg, name), out=out)
                if is_async:
                    gpu.fence_record(fence)
                    gpu.fence_wait(fence)
                got = np.asarray(out)
                assert np.array_equal(got.view(np.uint8), want[name].view(np.uint8)), \
                    f"{name}, async={is_async}: {np.sum(got != want[name])} values differ"
    finally:
        gpu.set_async(False)
        gpu.synchronize()
        for out in pinned.values():
            gpu.host_free(out)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the ITMLib mirror
# ---------------------------------------------------------------------------------------------------------------------
def test_mirror_all_local_maps_equals_abi(pkg, gpu, synth, tmp_path):
    """multimap_harness: 3 local maps (a new one every 3 keyframes, anchored at that keyframe's pose), then
    GetImageAllLocalMaps from the last pose; the same maps built and drawn through the C ABI give the same bytes."""
    wl = synth.s_tiny()
    n_frames, K = 9, 3
    p = util.small_params(pkg, wl, num_local_blocks=0x800, num_buckets=0x1000, num_excess=0x400)
    frames = [wl.frame(i) for i in range(n_frames)]
    fin, fout = tmp_path / "frames.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", wl.W, wl.H, n_frames))
        for rgba, mm, M in frames:
            f.write(rgba.tobytes()); f.write(mm.tobytes()); f.write(pkg.mat_to_abi(M).tobytes())
        f.write(np.asarray(wl.intr, np.float32).tobytes())
        f.write(struct.pack("<4f", p.voxel_size, p.mu, p.frustum_min, p.frustum_max))
        f.write(struct.pack("<4i", p.max_w, p.num_local_blocks, p.num_buckets, p.num_excess))
    res = subprocess.run([HARNESS, str(fin), str(fout), str(K)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = open(fout, "rb").read()
    n_maps, = struct.unpack_from("<i", raw, 0)
    assert n_maps == 3
    off = 4
    T = np.frombuffer(raw, np.float32, 16 * n_maps, off).reshape(n_maps, 4, 4).transpose(0, 2, 1)
    off += 64 * n_maps
    fused = np.frombuffer(raw, np.float32, 16 * n_frames, off).reshape(n_frames, 4, 4).transpose(0, 2, 1)
    off += 64 * n_frames
    npx = wl.W * wl.H
    g_depth = np.frombuffer(raw, np.float32, npx, off).reshape(wl.H, wl.W)
    g_shaded = np.frombuffer(raw, np.uint8, npx * 4, off + npx * 4).reshape(wl.H, wl.W, 4)
    scenes = [gpu.create_scene(p) for _ in range(n_maps)]
    rss = [gpu.create_render_state(s, wl.W, wl.H) for s in scenes]
    v = gpu.create_view(wl.W, wl.H)
    for i, (rgba, mm, _) in enumerate(frames):
        gpu.view_update(v, rgba, mm, timestamp=float(i))
        gpu.process_frame(scenes[i // K], v, rss[i // K], fused[i], wl.intr)
    rs = gpu.create_render_state(scenes[0], wl.W, wl.H)
    M_last = frames[-1][2]
    depth = gpu.get_image_multi(scenes, T, rs, M_last, wl.intr, pkg.IMAGE_DEPTH)
    shaded = gpu.get_image_multi(scenes, T, rs, M_last, wl.intr, pkg.IMAGE_SHADED)
    assert (depth > 0).sum() > 500
    assert np.array_equal(g_depth, depth) and np.array_equal(g_shaded, shaded)
