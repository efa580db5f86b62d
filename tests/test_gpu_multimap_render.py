"""dslam_get_image_multi on the MI355X: exact reductions to dslam_get_image, one posed map, the blending law against
the float64 reference of ref64_multimap.py on maps of one weight each and on maps whose weights vary per voxel, maps side
by side, argument checks, the GetImage memo and async mode, and
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
import weighted_fixtures as wf

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
# 3b. the blending law on maps whose weights vary from voxel to voxel (weighted_fixtures.py)
# ---------------------------------------------------------------------------------------------------------------------
def _render_all(gpu, pkg, maps, M, intr, order=None):
    """(depth float64, shaded grey float64 [H, W], colour float64 [H, W, 3]) of the composite of `maps` (in `order`)."""
    order = list(range(len(maps))) if order is None else order
    scenes = [upload_map(gpu, pkg, maps[i].m) for i in order]
    Ts = [maps[i].T for i in order]
    rs = roomiest(gpu, scenes, wf.W, wf.H)
    depth = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_DEPTH).astype(np.float64)
    grey = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_SHADED)[..., 0].astype(np.float64)
    clr = gpu.get_image_multi(scenes, Ts, rs, M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME)[..., :3].astype(np.float64)
    return depth, grey, clr, scenes


def _against_float64(what, maps, M, intr, ref, depth, grey, clr, min_gradient=0.0):
    """The acceptance of test_blending_law_against_float64: hits equal off ties, |ddepth| <= 1e-3 voxel off ties and on at
    most 1 % of the pixels beyond, grey within 2, colour within 1 on the lit pixels.  Returns the pixels compared (hit in
    both, off ties) and the lit ones among them.  A pixel is lit when n . l > 0.05, as there, and -- on the slab fixture
    only, which passes min_gradient = 1e-3 -- its combined gradient is longer than that: a ray that
    passed a surface without weight can stop deep inside, where every sdf is clamped to -1 and the gradient is 0 up to
    rounding -- 2e-16 in float64, which normalises to some direction, exactly 0 in float32, which draws nothing.  The stored
    sdf has steps of 3e-5 and a float32 gradient component carries 1e-7 of rounding, so at 1e-3 the direction is good to
    1e-4, 0.02 grey levels."""
    vs = am.VS
    hit, tie = depth > 0, ref["tie"]
    assert np.array_equal(hit[~tie], ref["hit"][~tie]), f"{what}: {(hit != ref['hit'])[~tie].sum()} pixels off a tie differ in hit"
    both = hit & ref["hit"]
    assert both.sum() > 0.1 * wf.W * wf.H
    err = np.abs(depth - ref64.camera_depth(M, ref["p"], vs)) / vs
    sel = both & ~tie
    p_hit, cand = ref["p"][sel], ref["cand"][sel]
    n, length = rm.normals(maps, cand, p_hit, magnitude=True)
    ndl = n @ ref64.light_of(M)
    ok = (ndl > 0.05) & (length > min_gradient)
    d_grey = np.abs(grey[sel] - ref64.shaded_grey(ndl))[ok]
    d_clr = np.abs(clr[sel] - np.trunc(rm.colours(maps, cand, p_hit)))[ok]
    print(f"{what}: {sel.sum()} pixels off a tie ({(tie & ref['hit']).sum() / ref['hit'].sum():.2%} of the hits are ties), "
          f"|ddepth| <= {err[sel].max():.3g} voxel, grey within {d_grey.max():.3g}, colour within {d_clr.max():.3g} "
          f"({ok.sum()} lit pixels)")
    big = both & (err > 1e-3)
    assert not (big & ~tie).any(), f"{what}: |ddepth| up to {err[big & ~tie].max():.3g} voxel off a tie"
    assert big.sum() <= 0.01 * both.sum()
    assert ok.sum() > 0.5 * sel.sum()
    assert d_grey.max() <= 2.0, f"{what}: grey {d_grey.max()}"
    assert d_clr.max() <= 1.0, f"{what}: colour {d_clr.max()}"
    lit = np.zeros(sel.shape, bool)
    lit[sel] = ok
    return sel, lit


def test_weight_fields_against_float64(pkg, gpu):
    """Two spheres with radii two voxels apart under the two poses of _two_spheres, w_depth = texture x ramp, w_color =
    (2x + 3y + 5z) mod 4 (weighted_fixtures.ramp_spheres): depth, hits, shading and colour against the float64 reference
    that reads every voxel's own weights, and far from the references that blend with each map's mean weight or give a
    trilinear read its nearest tap's weight."""
    maps, M, intr, ref = wf.render_reference("ramp")
    depth, grey, clr, _ = _render_all(gpu, pkg, maps, M, intr)
    sel, _ = _against_float64("texture x ramp", maps, M, intr, ref, depth, grey, clr)
    for name, alt in (("per-map mean weights", wf.mean_weight_maps(maps)), ("nearest tap's weight", wf.nearest_weight_maps(maps))):
        other = ref64.camera_depth(M, rm.cast_rays(alt, M, intr, wf.W, wf.H)["p"], am.VS)
        med = np.median(np.abs(depth - other)[sel]) / am.VS
        print(f"texture x ramp: median {med:.3f} voxel from the reference with {name}")
        assert med > 0.3, name
    # the colour confidence is w_color, not w_depth: where both maps hold every tap, the w_depth-weighted colour is far
    p_hit, cand = ref["p"][sel], ref["cand"][sel]
    by_depth = [rm.Posed(pm.m, pm.T) for pm in maps]
    for pm in by_depth:
        pm.colour_weight = "w_depth"
    wrong = np.trunc(rm.colours(by_depth, cand, p_hit))
    far = np.abs(clr[sel] - wrong).max(axis=1)
    print(f"texture x ramp: median colour distance {np.median(far):.1f} from the w_depth-weighted colour")
    assert np.median(far) > 10.0


def test_zero_weight_slabs(pkg, gpu):
    """weighted_fixtures.slab_spheres: the image against the float64 reference, and region by region what the law says.
    Where only one map carries a weight the hit lies on that map's sphere, within 0.5 voxel (the other's is 2 voxels away;
    the two refinement steps of a march leave up to 0.2 voxel at grazing rays, in a single-map render too), and the depth
    is that map's own render's within 1e-3 voxel wherever the float64 references of the two agree -- not everywhere: in
    front of the surface one map's blocks reach further than the other's, there it alone is found and its sdf of 1.0 takes
    the 1 mu step where the single-map march takes the block step, and a march that stops elsewhere is refined to a
    slightly different point.  Where both maps hold the surface under the
    weight 0 the sum of the weights is 0, the read gives sdf 1.0 and the ray passes the surface both maps hold (it may stop
    deeper, at a voxel only one map holds: one found map's value counts whatever it weighs); where neither map has a
    w_color but both have a w_depth, the colour is the first contributor's, so the order of the list decides it."""
    maps, M, intr, ref = wf.render_reference("slab")
    depth, grey, clr, scenes = _render_all(gpu, pkg, maps, M, intr)
    sel, lit = _against_float64("zero slabs", maps, M, intr, ref, depth, grey, clr, min_gradient=1e-3)
    vs = am.VS
    d = ref["dir"].reshape(-1, 3)
    single = wf.single_references("slab")
    flat = lambda a: a.reshape(-1)

    ys, xs = (a.reshape(-1).astype(np.float64) for a in np.mgrid[0:wf.H, 0:wf.W])

    def regions(p, along):
        """slab_regions that hold for the points p and for the points `along` voxels from them on their rays"""
        rs = [wf.slab_regions(maps, p + k * d) for k in along]
        return [{key: rs[0][i][key] & rs[1][i][key] & rs[2][i][key] for key in rs[0][i]} for i in range(2)]

    # only one map weighted: that map's surface, and that map's single-map render
    rA, rB = regions(ref["p"].reshape(-1, 3), (-12.0, 0.0, 4.0))
    dref = ref64.camera_depth(M, ref["p"], vs)
    for i, (mine, other) in enumerate(((rA, rB), (rB, rA))):
        px = flat(sel) & mine["weighted"] & (other["keep"] | other["unobserved"])
        world = np.stack([flat(depth) * ((xs - float(intr[2])) / float(intr[0])), flat(depth) * ((ys - float(intr[3])) / float(intr[1])),
                          flat(depth)], -1)
        world = ref64.mat_vec_f64(np.linalg.inv(np.asarray(M, np.float64)), world)
        off = np.abs(np.linalg.norm(world - wf.C_WORLD, axis=1) / vs - (wf.RADIUS / vs + 2.0 * i))[px]
        rs_i = gpu.create_render_state(scenes[i], wf.W, wf.H)
        own = gpu.get_image(scenes[i], rs_i, rm.camera_of(M, maps[i].T), intr, pkg.IMAGE_DEPTH).astype(np.float64)
        same = px & flat(own > 0) & ~flat(single[i]["tie"]) & flat(single[i]["hit"]) & (np.abs(flat(dref) - flat(single[i]["depth"])) < 1e-4 * vs)
        err = np.abs(flat(depth) - flat(own))[same] / vs
        print(f"zero slabs: only map {i} weighted on {px.sum()} pixels, hits within {off.max():.3g} voxel of its sphere; "
              f"{same.sum()} of them where the law gives its own render's depth, |ddepth| <= {err.max() if same.any() else 0:.3g} voxel there")
        assert px.sum() >= 100 and off.max() <= 0.5
        # (in front of map 0's blocks map 1's reach further, so nearly every ray of map 0's half marches differently
        # from map 0's own render: 2 pixels of its half agree in the float64 references, 326 of map 1's)
        assert same.sum() >= (1, 100)[i] and err.max() <= 1e-3
    # neither weighted, both hold the surface
    pA = single[0]["p_world"].reshape(-1, 3)
    rA, rB = regions(pA, (-12.0, 0.0, 16.0))
    px = flat(single[0]["hit"] & single[1]["hit"]) & rA["keep"] & rB["keep"] & ~flat(ref["tie"])
    surface = np.maximum(flat(single[0]["depth"]), flat(single[1]["depth"]))
    passed = (flat(depth) == 0) | (flat(depth) > surface + am.MU)
    print(f"zero slabs: neither map weighted on {px.sum()} pixels, {(flat(depth) == 0)[px].sum()} without a hit, the others "
          f"{((flat(depth) - surface)[px & (flat(depth) > 0)] / vs).min() if (px & (flat(depth) > 0)).any() else 0:.3g} voxels and more behind the surface")
    assert px.sum() >= 100 and passed[px].all()
    assert np.array_equal((flat(depth) > 0)[px], flat(ref["hit"])[px])
    # w_color 0 in both maps (their voxels observed, so they hold their colour bytes): the first contributor's colour,
    # whichever map that is and whatever its w_depth
    rA, rB = regions(ref["p"].reshape(-1, 3), (-1.0, 0.0, 1.0))
    px = flat(sel) & rA["no_colour"] & rB["no_colour"] & rA["off_unobserved"] & rB["off_unobserved"] & flat(ref["cand"].all(-1))
    def first_colour(px, image, ordered, r, want, what):
        """On the pixels of px where the float64 law gives the first contributor's whole colour (all 8 of its taps hold
        it; a ray that stopped deep behind the surface may find only the other map), the image shows it."""
        law = np.trunc(rm.colours(ordered, r["cand"].reshape(-1, 2)[px], r["p"].reshape(-1, 3)[px]))
        whole = np.zeros(len(px), bool)
        whole[px] = (np.abs(law - np.trunc(np.array(want))) <= 1.0).all(axis=1)
        print(f"zero slabs, {what}: neither map has a w_color on {px.sum()} pixels, the first map's colour on {whole.sum()}")
        assert whole.sum() >= 200
        assert (np.abs(image.reshape(-1, 3)[whole] - np.trunc(np.array(want))) <= 1.0).all()

    first_colour(px & flat(lit), clr, maps, ref, wf.COLOUR_A, "A first")
    swapped = [maps[1], maps[0]]
    ref2 = rm.cast_rays(swapped, M, intr, wf.W, wf.H, sharp_ties=True)
    depth2, grey2, clr2, _ = _render_all(gpu, pkg, maps, M, intr, order=[1, 0])
    sel2, lit2 = _against_float64("zero slabs, B first", swapped, M, intr, ref2, depth2, grey2, clr2, min_gradient=1e-3)
    first_colour(px & flat(lit2), clr2, swapped, ref2, wf.COLOUR_B, "B first")

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
