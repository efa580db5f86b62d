"""Analytic maps whose weights vary from voxel to voxel, as a fused map's do (a map of analytic_maps.build_map otherwise
carries one w_depth and one w_color): the fixtures on which the weight a cross-map read takes decides the result.  Shared
by the CPU checks of the float64 references and the GPU tests of dslam_get_image_multi, dslam_mesh_scene_multi,
dslam_merge_maps and dslam_register_maps; each fixture is built once per process.

The two field shapes:

texture x ramp   w_depth = floor(LEVELS[(3x + 5y + 7z) mod 11] * ramp(x)).  The coefficients are coprime and differ per
    axis, so inside every cell the trilinear weight, the nearest tap's, tap 0's and a trilinear weight with two axes
    swapped all differ.  LEVELS holds 1, 7 and 60: what separates a trilinear weight from the nearest tap's is the share
    w_B / (w_A + w_B) of the blend, and the two spheres' surfaces are 2 voxels apart, so 0.3 voxel of depth needs the share
    to move by 0.15.  An additive texture 1 + (.. mod 11) under a ramp of 0 .. 24 moves it by 0.05 (measured on the
    float64 reference: median 0.10 voxel between the two reads, 0.26 voxel against per-map mean weights); weights a factor
    of 8 apart from one voxel to the next move it by 0.2 and more (0.44 / 0.64 voxel).  ramp rises from 1 to 4 across the
    middle 30 % of the map's box along its x axis in map A and falls from 4 to 1 in map B, so the blended surface lies
    near A's own at one end of the image and near B's at the other, and neither map's mean weight describes either end.
    w_color = (2x + 3y + 5z) mod 4: zeros included, uncorrelated with w_depth.

zero slabs       ranges of one coordinate in which a map's voxels weigh nothing: stored as fusion leaves a voxel it has
    never observed (sdf 32767), or -- keep_sdf -- with the analytic sdf under the weight 0.  The slabs of the two maps
    partly overlap: only A weighted, only B weighted, neither.
"""
import functools

import numpy as np

import analytic_maps as am
import multimesh_fixtures as fx
import ref64
import ref64_checks as rc
import ref64_multimap as rm

LEVELS = np.array([1, 60, 7, 1, 60, 7, 60, 1, 7, 1, 7])
COLOUR_A, COLOUR_B = fx.COLOUR_A, fx.COLOUR_B
C_WORLD, RADIUS = np.array([0.03, -0.02, 0.45]), 0.16
T_A = fx.pose(yaw=0.2, pitch=-0.1, t=(0.05, 0.02, -0.03))
T_B = fx.pose(yaw=-0.15, roll=0.2, t=(-0.04, 0.01, 0.06))


def texture(p):
    return (3 * p[..., 0] + 5 * p[..., 1] + 7 * p[..., 2]) % 11


def colour_texture(p):
    return (2 * p[..., 0] + 3 * p[..., 1] + 5 * p[..., 2]) % 4


def textured_ramp(x0, x1, rising, top=4.0):
    """The texture x ramp field over the voxel range [x0, x1) of the map's x axis."""
    def field(p):
        u = (p[..., 0] - x0) / (x1 - x0)
        u = u if rising else 1.0 - u
        return np.floor(LEVELS[texture(p)] * (1.0 + (top - 1.0) * np.clip((u - 0.35) / 0.3, 0.0, 1.0))).astype(np.int64)
    return field


def _sphere_centre(T):
    return T[:3, :3].astype(np.float64) @ C_WORLD + T[:3, 3]


def _flat(clr):
    return lambda x: np.broadcast_to(np.array(clr), x.shape)


@functools.lru_cache(maxsize=None)
def ramp_spheres():
    """The two spheres of the blending-law tests (one world sphere, radii r and r + 2 voxels, the two non-trivial poses,
    a flat colour each) with the texture x ramp fields."""
    maps = []
    for T, dr, rising, clr in ((T_A, 0.0, True, COLOUR_A), (T_B, 2 * am.VS, False, COLOUR_B)):
        c = _sphere_centre(T)
        wd = textured_ramp((c[0] - 0.2) / am.VS, (c[0] + 0.2) / am.VS, rising)
        m = am.build_map(am.Sphere(c, RADIUS + dr), am.VS, am.MU, c - 0.2, c + 0.2, colour=_flat(clr), w_depth_field=wd,
                         w_color_field=colour_texture)
        maps.append(rm.Posed(m, T))
    return maps


MESH_SLAB = (8.0, 20.0)


def additive_ramp(x0, x1, rising):
    """w_depth = 1 + texture + ramp, ramp 0 .. 24 over the voxel range [x0, x1) of the map's x axis: weights of 1 .. 35 whose
    neighbours differ by 10 at the most.  The composite mesh's field: a vertex is a zero crossing between two blended lattice
    values, and under the steep field above the values of neighbouring lattice points come so close in places that the
    float32 rounding of the transform moves the crossing by more than the comparison's 1e-3 voxel (measured on the MI355X:
    1.3e-3 voxel at the worst vertex; one ulp on the poses moves the float64 reference's vertices by 2.6e-4 there)."""
    def field(p):
        u = (p[..., 0] - x0) / (x1 - x0)
        return 1 + texture(p) + np.clip(np.floor(25.0 * (u if rising else 1.0 - u)), 0, 24).astype(np.int64)
    return field


@functools.lru_cache(maxsize=None)
def mesh_spheres():
    """The composite mesh's fixture: the two spheres with the additive_ramp fields (rising in map A, falling in map B),
    w_color = (2x + 3y + 5z) mod 4, and a slab of map A -- MESH_SLAB[0] to MESH_SLAB[1] voxels above its sphere's centre
    along the map's y axis -- whose voxels weigh nothing and keep their sdf and colour."""
    maps = []
    for T, dr, rising, clr in ((T_A, 0.0, True, COLOUR_A), (T_B, 2 * am.VS, False, COLOUR_B)):
        c = _sphere_centre(T)
        wd = additive_ramp((c[0] - 0.2) / am.VS, (c[0] + 0.2) / am.VS, rising)
        keep = False
        if rising:
            def keep(p, cy=c[1] / am.VS):
                return (p[..., 1] - cy >= MESH_SLAB[0]) & (p[..., 1] - cy < MESH_SLAB[1])

            def wd(p, ramp=wd, keep=keep):
                return np.where(keep(p), 0, ramp(p))
        m = am.build_map(am.Sphere(c, RADIUS + dr), am.VS, am.MU, c - 0.2, c + 0.2, colour=_flat(clr), w_depth_field=wd,
                         w_color_field=colour_texture, keep_sdf=keep)
        maps.append(rm.Posed(m, T))
    return maps


def mean_weight_maps(maps):
    """The same maps read with one weight per map, its voxels' mean: what a law that ignored the field would blend."""
    out = [rm.Posed(pm.m, pm.T) for pm in maps]
    for pm in out:
        pm.w_depth = float(pm.m.voxels["w_depth"].mean())
    return out


def nearest_weight_maps(maps):
    """The same maps with every trilinear read weighted by its nearest tap's weight."""
    out = [rm.Posed(pm.m, pm.T) for pm in maps]
    for pm in out:
        pm.weight_read = "nearest"
    return out


# slabs of the zero-slab fixture: voxel offsets from the sphere's centre along the map's y axis (w_depth) and x axis (w_color)
SLABS = {"A": dict(keep=(-36, 4), unobserved=(22, 36), no_colour=(-24, 0)),
         "B": dict(keep=(-22, -4), unobserved=(8, 36), no_colour=(-12, 12))}


@functools.lru_cache(maxsize=None)
def slab_spheres():
    """The two spheres with w_depth 1 + texture (1 .. 11) and w_color 1 / 3, except in the slabs of SLABS: `keep` weighs 0
    and keeps the sdf, `unobserved` is stored as never observed, `no_colour` has w_color 0 (the colour bytes stay).  Along
    y: only B weighted, neither (both maps hold the surface, neither a weight), only A, both, only B, neither (no surface
    either), only A -- in the order the slabs of SLABS give.  Along x: a range in which neither map has a w_color while
    both have a w_depth."""
    maps = []
    for name, T, dr, wc, clr in (("A", T_A, 0.0, 1, COLOUR_A), ("B", T_B, 2 * am.VS, 3, COLOUR_B)):
        c = _sphere_centre(T)
        s = SLABS[name]

        def inside(p, axis, rng, c=c):
            v = p[..., axis] - c[axis] / am.VS
            return (v >= rng[0]) & (v < rng[1])

        def keep(p, s=s, inside=inside):
            return inside(p, 1, s["keep"])

        def wd(p, s=s, inside=inside):
            return np.where(inside(p, 1, s["keep"]) | inside(p, 1, s["unobserved"]), 0, 1 + texture(p))

        def wcf(p, s=s, inside=inside, wc=wc):
            return np.where(inside(p, 0, s["no_colour"]), 0, wc)

        hi = c + 0.2
        hi[2] = c[2]   # the half of the sphere that faces the cameras: a ray that passes the surface meets nothing behind it
        m = am.build_map(am.Sphere(c, RADIUS + dr), am.VS, am.MU, c - 0.2, hi, colour=_flat(clr), w_depth_field=wd,
                         w_color_field=wcf, keep_sdf=keep)
        maps.append(rm.Posed(m, T))
    return maps


def slab_regions(maps, p_world):
    """Of world points [n, 3] (voxel units): per map whether the point lies 2 voxels inside a slab of the kind (`keep`,
    `unobserved`, `no_colour`), and whether it lies 2 voxels outside every w_depth slab of the map (`weighted`) -- so that
    all 8 taps of a trilinear read at the point, and of one a voxel away, are of the one kind."""
    out = []
    for name, pm in zip("AB", maps):
        c = _sphere_centre(pm.T) / am.VS
        q = pm.to_map(p_world) - c
        r = {}
        for kind, axis in (("keep", 1), ("unobserved", 1), ("no_colour", 0)):
            lo, hi = SLABS[name][kind]
            r[kind] = (q[:, axis] >= lo + 2) & (q[:, axis] < hi - 3)
            r["off_" + kind] = (q[:, axis] < lo - 3) | (q[:, axis] >= hi + 2)
        r["weighted"] = r["off_keep"] & r["off_unobserved"]
        out.append(r)
    return out


W, H = 96, 72


@functools.lru_cache(maxsize=None)
def render_reference(name):
    """(maps, M, intr, float64 reference with the sharp tie flags) of the composite-raycast fixture `name` at 96 x 72,
    computed once per process."""
    maps = ramp_spheres() if name == "ramp" else slab_spheres()
    M, intr = rc.camera(W, H)
    return maps, M, intr, rm.cast_rays(maps, M, intr, W, H, sharp_ties=True)


@functools.lru_cache(maxsize=None)
def single_references(name):
    """Per map of the fixture its own float64 render (ref64.cast_rays from the camera that sees the map) with the hit
    points taken back to the world frame: dicts of depth [H, W] (metres), hit, tie, p_world and p_stop_world [H, W, 3]
    (voxels; p_stop: where the march stopped, before the two refinement steps)."""
    maps, M, intr, _ = render_reference(name)
    out = []
    for pm in maps:
        Mi = rm.camera_of(M, pm.T)
        r = ref64.cast_rays(pm.m, Mi, intr, W, H)
        out.append(dict(depth=ref64.camera_depth(Mi, r["p"], am.VS), hit=r["hit"], tie=r["tie"],
                        p_world=(r["p"] - pm.t_vox) @ pm.R, p_stop_world=(r["p_stop"] - pm.t_vox) @ pm.R))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the merge: the plane pair of test_gpu_merge.py re-weighted
# ---------------------------------------------------------------------------------------------------------------------
def _plane_colour(x):
    return 128.0 + (x - np.array([0.0, 0.0, 0.4])) @ np.array([[300.0, 0.0, 40.0], [0.0, 250.0, -60.0], [60.0, 80.0, 0.0]])


@functools.lru_cache(maxsize=None)
def weighted_planes():
    """(source, destination): one plane seen by two maps that overlap in x.  Source: w_depth 1 .. 7 from the texture with one
    voxel in 37 unobserved (w_depth 0 inside resident blocks), w_color 1 .. 3 with one voxel in 13 at 0, a linear colour
    field.  Destination: w_depth 1 .. 99, so that the clamp at max_w = 100 is reached in places; no colour.
    (Not (2x + 3y + 5z) mod 4 for the source's w_color: the 8 taps of a cell run through all four residues, so one of them
    would always be 0 and the colour half of every resampled voxel would idle.  The zeros chosen here meet 7 of the 13
    residues in a cell, and those of w_depth 6 of 37.)"""
    geom = am.Plane((0.1, 0.05, -1.0), -0.40)

    def src_wd(p):
        return np.where((p[..., 0] + 6 * p[..., 1] + 36 * p[..., 2]) % 37 == 0, 0, 1 + texture(p) % 7)

    def dst_wd(p):
        return 1 + (5 * p[..., 0] + 3 * p[..., 1] + 11 * p[..., 2]) % 99

    def src_wc(p):
        return np.where((p[..., 0] + 3 * p[..., 1] + 9 * p[..., 2]) % 13 == 0, 0, 1 + (2 * p[..., 0] + 3 * p[..., 1] + 5 * p[..., 2]) % 3)

    a = am.build_map(geom, am.VS, am.MU, (-0.15, -0.10, 0.2), (0.10, 0.10, 0.62), colour=_plane_colour, w_depth_field=src_wd,
                     w_color_field=src_wc)
    b = am.build_map(geom, am.VS, am.MU, (-0.05, -0.10, 0.2), (0.20, 0.10, 0.62), w_depth_field=dst_wd)
    return a, b


def merge_outcomes(src_map, before, after, X, with_colour=1):
    """What a merge of `src_map` (the analytic source) under X did to every voxel of the destination's resident blocks,
    from the states (ref_merge.State) before and after it, against the weight law of DESIGN.md section 14 stated on the
    source's lookup grid: w_depth' = min(w_depth + r, max_w) with r the smallest w_depth of the 8 taps (of the one voxel
    under the identity), 0 when a tap weighs nothing; the colour half changes exactly where r > 0 and every tap has a
    w_color.  Asserts both on every voxel and returns the counts: changed, gated (every tap in a resident source block, one
    of them without weight), colour_live, colour_idle (of the voxels with r > 0), clamped."""
    import ref_merge

    _, Yt, identity = ref_merge.transforms(X, src_map.vs)
    empty = np.zeros(512, am.VOXEL_DTYPE)
    empty["sdf"] = 32767
    out = dict(changed=0, gated=0, colour_live=0, colour_idle=0, clamped=0)
    for entry in after.live():
        e = after.hash[entry]
        P = e["pos"].astype(np.int64)[None] * 8 + ref_merge.LOCAL
        if identity:
            taps = P[:, None, :]
        else:
            q = ref_merge.to_map(Yt, False, P.astype(np.float32))
            taps = np.floor(q).astype(np.int64)[:, None, :] + ref_merge.TAPS[None]
        wd, wc = src_map.lookup_weights(taps)
        found = src_map.lookup(taps)[2]
        r = np.where((wd > 0).all(axis=1), wd.min(axis=1), 0).astype(np.int64)
        live = (r > 0) & (wc > 0).all(axis=1) & bool(with_colour)
        old = before.vba[e["ptr"]] if before.hash["ptr"][entry] == e["ptr"] else empty
        new = after.vba[e["ptr"]]
        want = np.minimum(old["w_depth"].astype(np.int64) + r, after.max_w)
        assert np.array_equal(new["w_depth"], want), f"block {e['pos']}: w_depth is not min(w_dst + min of the taps, max_w)"
        same_colour = (new["clr"] == old["clr"]).all(axis=1) & (new["w_color"] == old["w_color"])
        assert not (same_colour & live).any() and same_colour[~live].all(), f"block {e['pos']}: colour halves"
        assert (new["sdf"] == old["sdf"])[r == 0].all()
        out["changed"] += int((new.view(np.uint64) != old.view(np.uint64)).sum())
        out["gated"] += int((found.all(axis=1) & (r == 0)).sum())
        out["colour_live"] += int(live.sum())
        out["colour_idle"] += int(((r > 0) & ~live).sum())
        out["clamped"] += int(((r > 0) & (want == after.max_w)).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the registration: the box-corner pair with scattered voxels that weigh nothing
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def weighted_box_pair():
    """register_fixtures.box_pair("small") with w_depth 1 + texture and one voxel in 37 unobserved in both maps: the source
    loses candidates, the destination's 8-tap gate (every tap with w_depth > 0) turns 6 reads in 37 away."""
    import ref64_register as rr
    import register_fixtures as rf

    def wd(p):
        return np.where((p[..., 0] + 6 * p[..., 1] + 36 * p[..., 2]) % 37 == 0, 0, 1 + texture(p))

    X = rf.true_transform("small")
    dst = am.build_map(rr.Moved(am.BoxCorner((0.16, 0.12, 0.55)), X), am.VS, am.MU, (-0.2, -0.22, 0.2), (0.34, 0.3, 0.72),
                       w_depth_field=wd)
    return rf.Pair(rf._box_source(w_depth_field=wd), dst, X)
