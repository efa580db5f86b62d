"""Check bodies shared by test_oracle_reference64.py (CPU oracle) and test_gpu_reference64.py (HIP engine): each takes
an `api` (either engine, same wrapper class), runs the real entry points and compares them with the float64
references of ref64.py, on the synthetic sequences and on the exact maps of analytic_maps.py."""
import numpy as np

import analytic_maps as am
import ref64
import test_mc_tables as mct
import util

TIE_LIMIT = 1e-3  # fraction of updated voxels allowed to sit on a float32 / float64 branch tie
# Far from the origin (ref64.Scale), in units of u, float32's spacing at the largest voxel coordinate:
C_TIE = 8.0        # how far a float32 march position may lie from the float64 one when a branch is taken
C_RAY = 27.0       # a hit's position, and its depth, against the float64 march on rays that are no tie: twice the 13.4 u
                   # the float32 restatement of the march (ref32_march.py) shows at the worst (test_placement_fixtures.py)
C_TAPS = 1.5       # the direction of a 6-tap normal: each tap's position is rounded once (u / 2 per component, sqrt(3) u / 2
                   # per tap, sqrt(3) u on the difference of two taps two voxels apart: sqrt(3) u / 2 relative, times
                   # sqrt(3) for the three components)
C_MESH = 0.5       # a mesh vertex a + t (b - a) in voxels: one addition at the size of a (the product by the voxel
                   # size is the output ulp the check already counts)
C_MESH_SURFACE = 1.5 * np.sqrt(3.0)  # both roundings, (0.5 + 1) u per component, along a unit normal


# ---------------------------------------------------------------------------------------------------------------------
# integration, one step at a time
# ---------------------------------------------------------------------------------------------------------------------
def _entries(api, scene, rs):
    h = api.download_hash_table(scene)
    vis = api.download_visible_ids(rs)
    e = h[vis]
    e = e[e["ptr"] >= 0]
    return e["ptr"].astype(np.int64), e["pos"].astype(np.int64)


def _pool(api, scene, slots=None):
    """The voxel pool as (voxels, slots): every slot (slots None), or -- for a pool too large to bring to the host -- the
    blocks of `slots` (ascending), downloaded one contiguous run at a time."""
    if slots is None:
        return api.download_voxel_blocks(scene), None
    import highslot_fixtures as hs
    return hs.download_blocks(api, scene, slots), slots


def _live_slots(api, scene):
    h = api.download_hash_table(scene)
    return np.sort(h["ptr"][h["ptr"] >= 0].astype(np.int64))


def _places(slots, ptrs):
    """Rows of a _pool download that hold the blocks `ptrs`."""
    if slots is None:
        return ptrs
    at = np.searchsorted(slots, ptrs)
    assert np.array_equal(slots[at], ptrs), "a visible block is not a live block"
    return at


def _compare_step(before, after, ptrs, pos, ref, what):
    """`before`, `after`: the pool, or the rows of the live blocks with `ptrs` already mapped to rows (_places)."""
    got = after[ptrs]
    assert np.array_equal(got["w_depth"], ref["w_depth"]), f"{what}: depth weights differ ({(got['w_depth'] != ref['w_depth']).sum()} voxels)"
    assert np.array_equal(got["w_color"], ref["w_color"]), f"{what}: colour weights differ ({(got['w_color'] != ref['w_color']).sum()} voxels)"
    ds = np.abs(got["sdf"].astype(np.int64) - ref["sdf"])
    assert ds.max() <= 1, f"{what}: sdf off by {ds.max()} LSB"
    dc = np.abs(got["clr"].astype(np.int64) - ref["clr"])
    assert dc.max() <= 1, f"{what}: colour off by {dc.max()} LSB"
    rest = np.ones(len(before), bool)
    rest[ptrs] = False
    assert np.array_equal(before[rest].view(np.uint64), after[rest].view(np.uint64)), f"{what}: a block outside the visible list changed"


def check_integration(api, pkg, wl, frames, params, M_rgb_of=None, intr_rgb=None, wp=None, deintegrate=(), alloc_list=None,
                      live_only=False):
    """Fuse `frames` one at a time; before each integrate the voxels are downloaded and the float64 update A.5 is
    applied to them.  Frames listed in `deintegrate` are then taken out again (A.11) and checked the same way.
    Returns (updated voxel count, tie count, ties of axis-aligned poses) summed over the steps.
    `alloc_list`: a full allocation list the fresh scene starts from, in place of the ascending one.  `live_only`: the
    pool is too large for the host; each step downloads the live blocks by slot run, and "every other block unchanged"
    then speaks of the live blocks outside the visible list."""
    if wp is not None:
        api.set_fusion_weight_params(*wp)
    try:
        scene = api.create_scene(params)
        if alloc_list is not None:
            api.upload_scene_state(scene, allocation_list=alloc_list, last_free_block_id=len(alloc_list) - 1)
        rs = api.create_render_state(scene, wl.W, wl.H)
        view = api.create_view(wl.W, wl.H)
        vs, mu, mw, stop = params.voxel_size, params.mu, params.max_w, bool(params.stop_integrating_at_max_w)
        n_upd = n_tie = n_tie_aligned = 0
        steps = [(i, False) for i in frames] + [(i, True) for i in deintegrate]
        for i, de in steps:
            rgba, mm, M = wl.frame(i)
            M_rgb = None if M_rgb_of is None else M_rgb_of(M)
            api.view_update(view, rgba, mm, timestamp=float(i))
            depth = api.download_view_depth(view)
            assert np.array_equal(depth, ref64.depth_to_float(mm).astype(np.float32)), "depth conversion (A.3)"
            if de:
                before, slots = _pool(api, scene, _live_slots(api, scene) if live_only else None)
                api.deprocess_frame(scene, view, rs, M, wl.intr, M_rgb=M_rgb, intr_rgb=intr_rgb)
            else:
                api.allocate_scene_from_depth(scene, view, rs, M, wl.intr)
                before, slots = _pool(api, scene, _live_slots(api, scene) if live_only else None)
                api.integrate_into_scene(scene, view, rs, M, wl.intr, M_rgb=M_rgb, intr_rgb=intr_rgb)
            after, _ = _pool(api, scene, slots)
            ptrs, pos = _entries(api, scene, rs)
            ptrs = _places(slots, ptrs)
            ref, ties = ref64.integrate(before[ptrs], pos, depth, rgba, M, wl.intr, vs, mu, mw, M_rgb=M_rgb,
                                        intr_rgb=intr_rgb, stop_at_max=stop, wp=wp, deintegrate=de)
            what = f"{wl.name} frame {i}{' de-integrated' if de else ''}"
            _compare_step(before, after, ptrs, pos, ref, what)
            upd = int((ref.view(np.uint64) != before[ptrs].view(np.uint64)).sum())
            assert upd > 1000, f"{what}: only {upd} voxels updated"
            # an axis-aligned pose puts voxel centres exactly on pixel boundaries and the colour gate |eta| = mu / 4
            # (= one voxel at the S-room parameters): float32 decides those ties by design, so they are counted apart
            if np.array_equal(M[:3, :3], np.eye(3, dtype=M.dtype)):
                n_tie_aligned += ties
                continue
            n_upd += upd
            n_tie += ties
        assert n_tie <= TIE_LIMIT * n_upd, f"{n_tie} tie voxels of {n_upd} updated"
        return n_upd, n_tie, n_tie_aligned
    finally:
        if wp is not None:
            api.set_fusion_weight_params()


# ---------------------------------------------------------------------------------------------------------------------
# view filter
# ---------------------------------------------------------------------------------------------------------------------
def filter_input(W, H, seed=0):
    """Depth (mm) with the filter's edges: holes (0 and > 32000) next to valid pixels, depth jumps, regions below
    0.4 m, and a far rough patch (29 / 31 m checkerboard)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    mm = 900 + 2 * xx + yy + rng.integers(-3, 4, (H, W))
    mm[:, W // 2:] += 400  # a depth jump
    mm[: H // 3, : W // 4] = 250 + rng.integers(-2, 3, (H // 3, W // 4))  # below 0.4 m
    # 1-3 mm: sigma_z is small enough there that neighbours differing by 100 % keep a range weight near 1, so the
    # output depends on the spatial weights (sigma_L) far above float32 rounding
    mm[H // 3: H // 2, : W // 4] = rng.integers(1, 4, (H // 2 - H // 3, W // 4))
    far = (yy >= 2 * H // 3) & (xx < W // 3)
    mm[far] = np.where((xx + yy)[far] % 2 == 0, 29000, 31000)
    mm[rng.random((H, W)) < 0.04] = 0  # holes
    mm[H // 2, 3:9] = 0
    mm[H // 2 + 1, 5] = 32500  # out of range = hole
    return mm.astype(np.int16)


def check_view_filter(api, W, H, rel_tol):
    mm = filter_input(W, H)
    v = api.create_view(W, H)
    api.view_update(v, np.zeros((H, W, 4), np.uint8), mm, bilateral=True)
    got = api.download_view_depth(v).astype(np.float64)
    want = ref64.bilateral_update_view(ref64.depth_to_float(mm).astype(np.float32))
    border = np.ones((H, W), bool)
    border[2:H - 2, 2:W - 2] = False
    assert np.array_equal(got[border], want[border]), "border differs from upstream's zero floatImage border"
    inner = ~border
    assert np.array_equal(got[inner] == -1.0, want[inner] == -1.0), "holes differ"
    ok = inner & (want > 0)
    rel = np.abs(got[ok] - want[ok]) / want[ok]
    assert rel.max() <= rel_tol, f"bilateral filter: relative error {rel.max():.3g}"
    return float(rel.max())


# ---------------------------------------------------------------------------------------------------------------------
# raycast on the analytic maps
# ---------------------------------------------------------------------------------------------------------------------
def camera(W, H, yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0), f_scale=1.0):
    """(M world->camera float32, intr) for a camera at t whose axes are rotated by yaw (about y), pitch (x), roll (z)."""
    intr = np.array([0.75 * W * f_scale, 0.75 * W * f_scale, (W - 1) / 2.0, (H - 1) / 2.0], np.float32)
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
         @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return np.linalg.inv(T).astype(np.float32), intr


def load_map(api, pkg, m, W, H):
    scene = api.create_scene(m.scene_params(pkg))
    am.upload(api, scene, m)
    rs = api.create_render_state(scene, W, H)
    return scene, rs


def world_points_from_depth(M, intr, depth):
    H, W = depth.shape
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy, cx, cy = (float(v) for v in intr)
    pc = np.stack([depth * (xs - cx) / fx, depth * (ys - cy) / fy, depth], -1)
    invM = np.linalg.inv(np.asarray(M, np.float64))
    return pc @ invM[:3, :3].T + invM[:3, 3]


def tier_b_bound(m, cos_t, d0, s0):
    """Largest distance (voxels, along the surface normal) of a hit from the surface, given the distance d0 of the
    point where the march stopped and the read s0 (voxels) that stopped it, both from the float64 march.
    * Each refinement step moves the read distance along the RAY, which changes the distance along the normal by
      cos(theta) of it (theta: angle between the ray and the normal): d1 = d0 - s0 cos(theta), then, the second
      read being trilinear and so exact, d2 = d1 (1 - cos theta).  When s0 was a trilinear read too (s0 = d0) this
      is |d0| (1 - cos theta)^2; a nearest-voxel read (below the [-0.5, 0.1] window) can be sqrt(3)/2 voxel off.
      (The march only bounds d0 loosely: a step of 8 voxels through a missing block can land up to 8 cos(theta)
      minus the band's depth behind the surface.)
    * Reads are exact for a plane up to the int16 quantisation (trunc: < 1 LSB = mu/vs/32767 voxel per corner;
      3 reads).  For a sphere of radius r voxels the trilinear interpolant of |x - c| is off by at most
      (h^2/8) * trace(Hessian) = 1/(4r) per read, and a step of <= 1 voxel along the ray leaves the tangent plane by
      <= 1/(2r): together <= 3/(4r) + 1/(2r) over the refinements."""
    q = 3.0 * (m.mu / m.vs) / 32767.0 + 1e-5
    b = np.abs(d0 - s0 * cos_t) * (1.0 - cos_t) + q
    if isinstance(m.geom, am.Sphere):
        r = m.geom.r / m.vs
        b = b + 3.0 / (4.0 * r) + 1.0 / (2.0 * r)
    return b


def reference_rays(m, M, intr, W, H, scale=ref64.ORIGIN):
    """The float64 march with the tie tolerance of the fixture's size (at the origin: cast_rays' own default)."""
    return ref64.cast_rays(m, M, intr, W, H, tie_tol=scale(1e-4, C_TIE), by_outcome=scale.u > 0)


def check_raycast(api, pkg, m, M, intr, W, H, colour=False, icp=True, scale=ref64.ORIGIN, ref=None, extras=False):
    """Tier (a): the kernel against the float64 castRay on the same uploaded map.  Tier (b): the kernel's hit points
    against the closed-form surface.  Returns measured figures.  `scale`: the size of the fixture's coordinates;
    `ref`: reference_rays of the same arguments, where a caller has them already.  `extras`: the raycast result
    (positions in voxels) against the float64 march too, and get_depth_image_int16 against (int16)(depth * 1000)."""
    scene, rs = load_map(api, pkg, m, W, H)
    ref = reference_rays(m, M, intr, W, H, scale) if ref is None else ref
    thr_a = scale(1e-3, C_RAY)
    depth = api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH).astype(np.float64)
    hit = depth > 0
    tie = ref["tie"]
    assert np.array_equal(hit[~tie], ref["hit"][~tie]), f"hit masks differ on {(hit != ref['hit'])[~tie].sum()} non-tie pixels"
    both = hit & ref["hit"]
    assert both.sum() > 0.1 * W * H, f"only {both.sum()} hits"
    dref = ref64.camera_depth(M, ref["p"], m.vs)
    err = np.abs(depth - dref) / m.vs  # voxels
    big = both & (err > thr_a)
    assert not (big & ~tie).any(), f"tier (a): |ddepth| up to {err[big & ~tie].max():.3g} voxel with no threshold tie"
    assert big.sum() <= 0.01 * both.sum(), f"tier (a): {big.sum()} of {both.sum()} hits beyond {thr_a:.3g} voxel"
    out = dict(hits=int(both.sum()), ties=int((tie & both).sum()), a_max=float(err[both & ~tie].max()),
               a_p99=float(np.percentile(err[both], 99)))
    if extras:
        res = api.download_raycast_result(rs)
        assert np.array_equal(res[..., 3] > 0, hit), "the raycast result and the depth image disagree on the hits"
        rerr = np.abs(res[..., :3].astype(np.float64) - ref["p"]).max(-1)
        assert rerr[both & ~tie].max() <= thr_a, f"raycast result {rerr[both & ~tie].max():.3g} voxel from the float64 march"
        mm = api.get_depth_image_int16(scene, rs, M, intr, 1000)
        want = (depth.astype(np.float32) * np.float32(1000)).astype(np.int32).astype(np.int16)
        assert np.array_equal(mm, want), "get_depth_image_int16 is not (int16)(depth * 1000)"
        out["result_max"] = float(rerr[both & ~tie].max())
    # tier (b): distance of the kernel's hit along the normal
    xw = world_points_from_depth(M, intr, depth)
    dist = np.abs(m.geom.sdf(xw)) / m.vs
    nrm = m.geom.normal(xw)
    cos_t = np.abs(np.sum(nrm * ref["dir"], -1))
    d0 = m.geom.sdf(ref["p_stop"] * m.vs) / m.vs
    # (far from the origin the engine's ray lies up to C_RAY u beside the float64 ray the depth is put back on)
    bound = tier_b_bound(m, cos_t, d0, ref["sdf_stop"] * (m.mu / m.vs)) + scale(0.0, C_RAY)
    # the reads are linear in the distance only while every corner of their cells lies inside the truncation band:
    # a stop point more than mu/vs - sqrt(3) voxels behind the surface (after an 8-voxel step through a missing
    # block) reads clamped values, and the derivation above does not apply to it
    # (d0 and s0 describe the kernel's march only where the float64 march took the same branches: not on tie rays)
    sel = both & ~tie & ~ref["miss_cell"] & (np.abs(d0) + np.sqrt(3.0) < m.mu / m.vs)
    if isinstance(m.geom, am.BoxCorner):  # the field is linear only away from the walls' meeting lines
        g = np.sort(m.geom.k - xw, -1)
        sel &= (g[..., 1] - g[..., 0]) > 3.0 * m.vs
    assert sel.sum() > 0.05 * W * H
    over = sel & (dist > bound)
    assert not over.any(), f"tier (b): {over.sum()} hits beyond the bound, worst {(dist - bound)[over].max():.3g} voxel over"
    out["b_max"] = float(dist[sel].max())
    out["b_bound_max"] = float(bound[sel].max())
    if icp:
        out.update(_check_icp(api, scene, rs, m, M, intr, ref, hit, sel, bound, thr_a))
    out.update(_check_shading(api, pkg, scene, rs, m, M, intr, ref, both & ~tie, sel, dist, xw, scale))
    if colour:
        img = api.get_image(scene, rs, M, intr, pkg.IMAGE_COLOUR_FROM_VOLUME)
        chit = img[..., 3] > 0
        assert not (chit & ~hit).any(), "COLOUR_FROM_VOLUME pixel where the raycast found nothing"
        ca = chit & both & ~tie
        want = np.trunc(ref64.read_colour_trilinear(m, ref["p"][ca]))
        got = img[ca][:, :3].astype(np.float64)
        # tier (a): truncation (1) plus the colour gradient times the hit's distance from the float64 hit (the
        # depth error, stretched to a distance along the ray by at most 1 / cos of the ray's angle to the axis: 2)
        gvox = np.abs(m.colour_grad).sum(0) * m.vs  # colour change per voxel, per channel
        lim = 1.0 + gvox[None, :] * err[ca][:, None] * 2.0 + 1e-9
        assert (np.abs(got - want) <= lim).all(), f"COLOUR_FROM_VOLUME off by {np.abs(got - want).max()}"
        # tier (b) against the closed-form field at the kernel's hit: floor on storage (1) + truncation on output (1)
        # + the gradient times the hit's distance from the surface along the ray
        cb = chit & sel
        got_b = img[cb][:, :3].astype(np.float64)
        truth = m.colour(xw[cb])
        lim_b = 2.0 + gvox[None, :] * (dist[cb] / np.maximum(cos_t[cb], 0.1))[:, None] + 1e-6
        assert (np.abs(got_b - truth) <= lim_b).all(), "COLOUR_FROM_VOLUME against the analytic colour field"
        out["colour_max"] = float(np.abs(got - want).max())
    return out


def check_raycast_untied(api, pkg, m, M, intr, W, H, scale, ref, min_rays=40):
    """The ray march where the float64 march calls most rays ties (the full FAR placements, the table's ends): what holds
    ray by ray, asserted on every ray that is no tie, with no cap on the ties and a floor on the rays left.  The hit masks
    agree; depth, raycast result and ICP point lie within the scaled tier (a) bound of the float64 hit; the hit lies within
    the tier (b) bound of the closed-form surface; get_depth_image_int16 is (int16)(depth * 1000); no image type draws a
    pixel the march did not hit.  What needs whole neighbourhoods or counts of rays (the ICP normals, the shading's drawn
    set, the colours, the 1 % rule) stays with check_raycast at the D its tie cap allows."""
    scene, rs = load_map(api, pkg, m, W, H)
    thr_a = scale(1e-3, C_RAY)
    depth = api.get_image(scene, rs, M, intr, pkg.IMAGE_DEPTH).astype(np.float64)
    hit, tie = depth > 0, ref["tie"]
    assert np.array_equal(hit[~tie], ref["hit"][~tie]), f"hit masks differ on {(hit != ref['hit'])[~tie].sum()} non-tie pixels"
    ok = hit & ref["hit"] & ~tie
    assert ok.sum() >= min_rays, f"only {ok.sum()} hits that are no tie"
    err = np.abs(depth - ref64.camera_depth(M, ref["p"], m.vs)) / m.vs
    assert err[ok].max() <= thr_a, f"tier (a): |ddepth| up to {err[ok].max():.3g} voxel with no threshold tie"
    res = api.download_raycast_result(rs)
    assert np.array_equal(res[..., 3] > 0, hit), "the raycast result and the depth image disagree on the hits"
    rerr = np.abs(res[..., :3].astype(np.float64) - ref["p"]).max(-1)
    assert rerr[ok].max() <= thr_a, f"raycast result {rerr[ok].max():.3g} voxel from the float64 march"
    mm = api.get_depth_image_int16(scene, rs, M, intr, 1000)
    want = (depth.astype(np.float32) * np.float32(1000)).astype(np.int32).astype(np.int16)
    assert np.array_equal(mm, want), "get_depth_image_int16 is not (int16)(depth * 1000)"
    xw = world_points_from_depth(M, intr, depth)
    dist = np.abs(m.geom.sdf(xw)) / m.vs
    cos_t = np.abs(np.sum(m.geom.normal(xw) * ref["dir"], -1))
    d0 = m.geom.sdf(ref["p_stop"] * m.vs) / m.vs
    bound = tier_b_bound(m, cos_t, d0, ref["sdf_stop"] * (m.mu / m.vs)) + scale(0.0, C_RAY)
    sel = ok & ~ref["miss_cell"] & (np.abs(d0) + np.sqrt(3.0) < m.mu / m.vs)  # (as in check_raycast)
    if isinstance(m.geom, am.BoxCorner):
        g = np.sort(m.geom.k - xw, -1)
        sel &= (g[..., 1] - g[..., 0]) > 3.0 * m.vs
    assert sel.sum() >= min_rays // 2, f"only {sel.sum()} rays for tier (b)"
    over = sel & (dist > bound)
    assert not over.any(), f"tier (b): {over.sum()} hits beyond the bound, worst {(dist - bound)[over].max():.3g} voxel over"
    api.find_visible_blocks(scene, rs, M, intr)
    pts, nrms = api.create_icp_maps(scene, rs, M, intr)
    pok = pts[..., 3] > 0
    assert not (pok & ~hit).any(), "ICP point where the raycast found nothing"
    perr = np.linalg.norm(pts[..., :3] - ref["p"] * float(np.float32(m.vs)), axis=-1) / m.vs
    assert (pok & ok).sum() >= min_rays // 4 and perr[pok & ok].max() <= np.sqrt(3.0) * thr_a, "ICP points"
    for t in (pkg.IMAGE_SHADED, pkg.IMAGE_COLOUR_FROM_NORMAL, pkg.IMAGE_COLOUR_FROM_VOLUME):
        assert not ((api.get_image(scene, rs, M, intr, t)[..., 3] > 0) & ~hit).any(), f"image type {t} draws a pixel that is no hit"
    return dict(hits=int(hit.sum()), untied=int(ok.sum()), tier_b_rays=int(sel.sum()), a_max=float(err[ok].max()),
                result_max=float(rerr[ok].max()), b_max=float(dist[sel].max()), b_bound_max=float(bound[sel].max()))


def _check_icp(api, scene, rs, m, M, intr, ref, hit, sel, bound, thr_a=1e-3):
    """CreateICPMaps: points and normals against the float64 restatement built from the float64 march points
    (tier a), and the normals against the analytic surface with a bound derived from the tap points' tier-(b)
    bounds (tier b)."""
    api.find_visible_blocks(scene, rs, M, intr)
    pts, nrms = api.create_icp_maps(scene, rs, M, intr)
    ok = pts[..., 3] > 0
    assert np.array_equal(ok, nrms[..., 3] == 0), "ICP point and normal maps disagree on which pixels hold a point"
    assert not (ok & ~hit).any(), "ICP point where the raycast found nothing"
    n_ref, f_ref, tap, t_icp = ref64.icp_normals(ref["p"], ref["hit"], ref["tie"], m.vs, ref64.light_of(M))
    assert np.array_equal(ok[~t_icp], f_ref[~t_icp]), f"ICP: {(ok != f_ref)[~t_icp].sum()} pixels differ in validity"
    assert ok.sum() > 0.3 * hit.sum(), f"only {ok.sum()} ICP points"
    a = ok & ~t_icp
    # points: the raycast points in metres, so the depth's tier (a) -- 1e-3 voxel -- holds for them too (the float32
    # rounding of a metric coordinate below 1 m is < 6e-8 m = 1.2e-5 voxel, inside that figure)
    perr = np.linalg.norm(pts[..., :3] - ref["p"] * float(np.float32(m.vs)), axis=-1) / m.vs
    # (far from the origin: within thr_a per component, sqrt(3) thr_a as a distance)
    tap_err = np.sqrt(3.0) * thr_a if thr_a > 1e-3 else 1e-3
    assert perr[a].max() <= tap_err, f"ICP points: {perr[a].max():.3g} voxel from the float64 march"
    # normals, tier (a): each tap point is within 1e-3 voxel of its float64 twin, so each difference vector is within
    # 2e-3 voxel and the cross product's direction tilts by at most 2e-3 (1/|dx| + 1/|dy|) / sin(angle(dx, dy))
    dxv, dyv, sphi = _tap_geometry(ref["p"], tap)
    lim_a = 2.0 * tap_err * (1.0 / dxv + 1.0 / dyv) / sphi + 1e-6
    ang_a = _angle(nrms[..., :3], n_ref)
    assert (ang_a[a] <= lim_a[a]).all(), f"ICP normals: {np.degrees(ang_a[a]).max():.3g} deg from the float64 restatement"
    out = dict(icp_points=int(ok.sum()), icp_ties=int((t_icp & (ok | f_ref)).sum()), icp_a_deg=float(np.degrees(ang_a[a]).max()))
    # normals, tier (b): a tap is at most bound[tap] off the surface along the normal, so a difference vector leaves
    # the tangent plane by at most (b+ + b-) / |d|; on a sphere of radius r the chord is tangent at its own midpoint,
    # up to |d| / 2 away from the pixel's point: |d| / (2r) more
    bsel = a & sel
    tb = np.zeros(a.shape)
    for k, dv in ((1, dxv), (0, dyv)):
        for t in (1, 2):
            off = [0, 0]
            off[k] = t
            bp = np.roll(np.where(sel, bound, np.inf), (-off[0], -off[1]), axis=(0, 1))
            bm = np.roll(np.where(sel, bound, np.inf), (off[0], off[1]), axis=(0, 1))
            on = tap == t
            tb = np.where(on, tb + (bp + bm) / dv, tb)
    if isinstance(m.geom, am.Sphere):
        tb = tb + (dxv + dyv) / (2.0 * m.geom.r / m.vs)
    lim_b = tb / sphi + 1e-4
    bsel &= np.isfinite(lim_b)
    n_true = m.geom.normal(pts[..., :3].astype(np.float64))
    ang_b = _angle(nrms[..., :3], n_true)
    assert bsel.sum() > 0.2 * ok.sum()
    assert (ang_b[bsel] <= lim_b[bsel]).all(), f"ICP normals: {np.degrees((ang_b - lim_b)[bsel]).max():.3g} deg beyond the bound"
    out["icp_b_deg"] = float(np.degrees(ang_b[bsel]).max())
    return out


def _angle(a, b):
    """Angle between direction fields, well conditioned near 0 (arccos of the dot of a float32 unit vector is not)."""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, -1))


def _tap_geometry(p, tap):
    """|dx|, |dy| (voxels) of the float64 tap differences each pixel's normal uses, and the sine of their angle."""
    def sh(a, dy, dx):
        return np.roll(a, (-dy, -dx), axis=(0, 1))
    d = {t: (sh(p, 0, t) - sh(p, 0, -t), sh(p, t, 0) - sh(p, -t, 0)) for t in (1, 2)}
    dx = np.where((tap == 1)[..., None], d[1][0], d[2][0])
    dy = np.where((tap == 1)[..., None], d[1][1], d[2][1])
    lx, ly = np.linalg.norm(dx, axis=-1), np.linalg.norm(dy, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        sphi = np.linalg.norm(np.cross(dx, dy), axis=-1) / (lx * ly)
    return lx, ly, sphi


def _check_shading(api, pkg, scene, rs, m, M, intr, ref, a, sel, dist, xw, scale=ref64.ORIGIN):
    """SHADED and COLOUR_FROM_NORMAL: the 6-tap normal at the hit, shaded against the camera's viewing axis.
    Tier (a): against the float64 normal at the float64 hit (+-1 for the output truncation).  Tier (b): against the
    analytic normal.  The taps read the field one voxel either side along each axis; for a plane the difference is
    2 n_k vs/mu up to 2 LSB of quantisation per component, a relative error of at most sqrt(3) * 2/32767 / (2 vs/mu);
    for a sphere of radius r voxels each trilinear read is off by at most 1/(4r) voxel, sqrt(3)/(4r) on the
    direction, and the central difference of |x| adds < 1/r^2."""
    light = ref64.light_of(M)
    sh = api.get_image(scene, rs, M, intr, pkg.IMAGE_SHADED)
    cn = api.get_image(scene, rs, M, intr, pkg.IMAGE_COLOUR_FROM_NORMAL)
    n64, nmiss = ref64.sdf_normal(m, ref["p"].reshape(-1, 3))
    n64, nmiss = n64.reshape(ref["p"].shape), nmiss.reshape(a.shape)
    angle = n64 @ light
    f_ref = ref["hit"] & (angle > 0)
    t_ang = np.abs(angle) < 1e-4
    fk = sh[..., 3] > 0
    assert np.array_equal(fk, cn[..., 3] > 0), "SHADED and COLOUR_FROM_NORMAL disagree on which pixels are drawn"
    assert np.array_equal(fk[a & ~t_ang], f_ref[a & ~t_ang]), "SHADED: drawn pixels differ from the float64 rule"
    ta = a & f_ref & ~t_ang
    assert ta.sum() > 0.1 * a.sum()
    g_ref = ref64.shaded_grey(angle)
    c_ref = ref64.normal_colour(n64)
    dg = np.abs(sh[..., 0].astype(np.float64) - g_ref)
    dc = np.abs(cn[..., :3].astype(np.float64) - c_ref).max(-1)
    # far from the origin the kernel's normal turns by up to C_TAPS u (its taps' positions are rounded) and, on a sphere
    # of radius r voxels, by the hit's distance from the float64 hit (sqrt(3) C_RAY u) / r; the truncated outputs then
    # differ by one more than the whole levels that turn is worth
    turn = scale(0.0, C_TAPS)
    if isinstance(m.geom, am.Sphere):
        turn += np.sqrt(3.0) * scale(0.0, C_RAY) / (m.geom.r / m.vs)
    lim_g, lim_c = 1 + np.floor(0.8 * 255.0 * turn), 1 + np.floor(0.35 * 255.0 * turn)
    assert dg[ta].max() <= lim_g, f"SHADED off by {dg[ta].max()} from the float64 grey"
    assert (sh[ta][:, :4] == sh[ta][:, :1]).all(), "SHADED: grey channels differ"
    assert dc[ta].max() <= lim_c, f"COLOUR_FROM_NORMAL off by {dc[ta].max()} from the float64 encoding"
    eps = np.sqrt(3.0) * 2.0 / 32767.0 / (2.0 * m.vs / m.mu) + scale(0.0, C_TAPS)
    if isinstance(m.geom, am.Sphere):
        r = m.geom.r / m.vs
        eps += np.sqrt(3.0) / (4.0 * r) + 1.0 / r ** 2
    # the taps' cells reach 1 + sqrt(3) voxels from the hit: they must all lie inside the truncation band
    tb = fk & sel & ~nmiss & (dist + 1.0 + np.sqrt(3.0) < m.mu / m.vs)
    n_true = m.geom.normal(xw)
    ang_t = n_true @ light
    gb = np.abs(sh[..., 0].astype(np.float64) - ref64.shaded_grey(ang_t))
    cb = np.abs(cn[..., :3].astype(np.float64) - ref64.normal_colour(n_true)).max(-1)
    assert tb.sum() > 0.05 * a.sum()
    assert gb[tb].max() <= 1.0 + 0.8 * 255.0 * eps, f"SHADED off by {gb[tb].max():.3g} from the analytic normal"
    assert cb[tb].max() <= 1.0 + 0.35 * 255.0 * eps, f"COLOUR_FROM_NORMAL off by {cb[tb].max():.3g} from the analytic normal"
    return dict(shaded_a=float(dg[ta].max()), shaded_b=float(gb[tb].max()), cfn_b=float(cb[tb].max()))


# ---------------------------------------------------------------------------------------------------------------------
# mesh
# ---------------------------------------------------------------------------------------------------------------------
def check_mesh(api, pkg, m, surface_bound=None, max_triangles=0, scale=ref64.ORIGIN, colour=False):
    """The mesh triangle for triangle, in upstream's order (hash entries, voxels, table slots), against the float64
    re-derivation; then its vertices against the analytic surface.  `max_triangles`: the list's size, where the default
    of 32 per pool slot would be sized by the pool and not by the map.  `scale`: the size of the fixture's coordinates.
    `colour`: the vertex colours too, each within [0, 1] and, where the map has a linear colour field, within 1 / 255
    (the floor on storage of the edge's two ends) of the field at the vertex."""
    scene = api.create_scene(m.scene_params(pkg))
    am.upload(api, scene, m)
    pos, col = api.mesh_scene(scene, max_triangles=max_triangles, colour=colour)
    ec, co = mct.load_small_tables()
    ref = ref64.mesh(m, co, ec, mct.load_table())
    assert len(pos) < (max_triangles or m.num_local_blocks * 32) - 1, "mesh saturated: size the map"
    assert len(pos) == len(ref), f"{len(pos)} triangles, float64 re-derivation has {len(ref)}"
    got = pos.astype(np.float64) / np.float64(np.float32(m.vs))
    # 1e-5 voxel, plus the float32 rounding of the metric output (one ulp of the largest coordinate, in voxels)
    ulp = np.spacing(np.abs(pos).max().astype(np.float32)) / m.vs
    d = np.abs(got - ref).max()
    assert d <= 1e-5 + ulp + scale(0.0, C_MESH), f"mesh vertices {d:.3g} voxel from the float64 edge interpolation"
    out = dict(triangles=len(pos), vertex_max=float(d))
    if surface_bound is not None:
        dist = np.abs(m.geom.sdf(pos.reshape(-1, 3).astype(np.float64))) / m.vs
        lim = surface_bound + scale(0.0, C_MESH_SURFACE)
        assert dist.max() <= lim, f"mesh vertex {dist.max():.3g} voxel off the analytic surface"
        out["surface_max"] = float(dist.max())
    if colour:
        assert col is not None and col.shape == pos.shape and col.min() >= 0.0 and col.max() <= 1.0
        if m.colour is not None:
            x = pos.reshape(-1, 3).astype(np.float64)
            gvox = np.abs(m.colour_grad).sum(0) * m.vs
            lim_c = 1.0 + gvox[None, :] * scale(0.0, C_MESH_SURFACE) + 1e-4
            dc = np.abs(col.reshape(-1, 3).astype(np.float64) * 255.0 - m.colour(x))
            assert (dc <= lim_c).all(), f"mesh colours {dc.max():.3g} / 255 from the analytic colour field"
            out["colour_max"] = float(dc.max())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test files run
# ---------------------------------------------------------------------------------------------------------------------
def _rgb_camera(synth):
    T = synth.pose_matrix(synth.look_rotation(0.01, 0.005), [0.02, -0.01, 0.0]).astype(np.float32)
    return (lambda M: (T @ M).astype(np.float32)), None


INTEGRATION_CASES = ["tiny", "room_70x45", "two_cameras", "depth_weighting", "max_w3", "max_w3_stop", "deintegrate"]


def run_integration_case(api, pkg, synth, case):
    wl = synth.s_tiny()
    p = util.small_params(pkg, wl)
    kw = {}
    frames = range(4)
    if case == "room_70x45":
        wl = synth.s_room(70, 45)
        p = util.small_params(pkg, wl)
        frames = range(3)
    elif case == "two_cameras":
        kw["M_rgb_of"], _ = _rgb_camera(synth)
        kw["intr_rgb"] = np.asarray(wl.intr, np.float32) * np.float32(1.02)
    elif case == "depth_weighting":
        kw["wp"] = (True, 5, 3.0)
    elif case == "max_w3":
        p = util.small_params(pkg, wl, max_w=3)
        frames = range(5)
    elif case == "max_w3_stop":
        p = util.small_params(pkg, wl, max_w=3, stop_integrating_at_max_w=1)
        frames = range(5)
    elif case == "deintegrate":
        kw["deintegrate"] = (1, 2)
    return check_integration(api, pkg, wl, frames, p, **kw)


def raycast_cases():
    """name -> (map builder, W, H, camera kwargs, colour)."""
    return {
        "plane_64x48": (lambda: am.tilted_plane(num_buckets=0x40), 64, 48, dict(yaw=0.1, roll=0.3), False),
        "plane_70x45_grazing_holes": (lambda: am.tilted_plane(tilt_deg=72.0, holes=0.08, seed=3, num_buckets=0x40),
                                      70, 45, dict(pitch=0.05), False),
        "plane_very_close": (lambda: am.tilted_plane(tilt_deg=10.0, num_buckets=0x40), 64, 48,
                             dict(t=(0.0, 0.0, 0.42)), False),
        "plane_1226x370": (lambda: am.tilted_plane(num_buckets=0x100), 1226, 370, dict(yaw=-0.05, roll=0.1), False),
        "sphere_outside": (lambda: am.sphere_outside(num_buckets=0x100), 64, 48, dict(yaw=0.05, pitch=-0.1), False),
        "sphere_inside": (lambda: am.sphere_inside(num_buckets=0x400), 70, 45, dict(yaw=0.4, pitch=0.2, roll=0.2), False),
        "box_corner": (lambda: am.box_corner(num_buckets=0x80), 70, 45, dict(yaw=0.2, pitch=0.15), False),
        "colour_plane": (lambda: am.colour_plane(num_buckets=0x40), 64, 48, dict(roll=0.2), True),
    }


def run_raycast_case(api, pkg, case):
    build, W, H, cam, colour = raycast_cases()[case]
    m = build()
    M, intr = camera(W, H, **cam)
    return check_raycast(api, pkg, m, M, intr, W, H, colour=colour), m.max_chain


def mesh_cases():
    """name -> (map builder, bound on the vertices' distance to the analytic surface in voxels, or None).  A vertex
    is the root of the linear interpolant along its edge: exact for a plane up to the int16 quantisation of both
    ends (2 * mu/vs/32767 voxel); for a sphere of radius r voxels the interpolant of |x - c| along an edge of one
    voxel sags by at most 1/(8r)."""
    q = 2.0 * (MU_VOX / 32767.0) + 1e-5
    return {
        "plane": (lambda: am.tilted_plane(num_buckets=0x40), q),
        "plane_holes": (lambda: am.tilted_plane(tilt_deg=35.0, holes=0.1, seed=5, num_buckets=0x40), q),
        "sphere_outside": (lambda: am.sphere_outside(num_buckets=0x100), q + 1.0 / (8.0 * 0.16 / am.VS)),
        "box_corner": (lambda: am.box_corner(num_buckets=0x80), None),
    }


MU_VOX = am.MU / am.VS


def run_mesh_case(api, pkg, case):
    build, bound = mesh_cases()[case]
    m = build()
    return check_mesh(api, pkg, m, surface_bound=bound)
