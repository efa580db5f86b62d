"""dslam_query_points and dslam_cast_rays on the MI355X: the laws that hold bit for bit (permutation,
splitting, host against device form, chunking, maps that hold nothing, list order, `what` subsets, a ray's shading against a
point query at its hit point, stored voxels read at their centres), points and rays against the float64 reference of
ref64_query.py on the weight-varying fixtures, the edges, and the argument checks."""
import numpy as np
import pytest

import analytic_maps as am
import placement_fixtures as pf
import query_bounds as qb
import query_fixtures as qf
import ref64_multimap as rm
import ref64_query as rq
import util
import weighted_fixtures as wf

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
SPLITS = (1, 63, 64, 65, -1)


def upload_map(api, pkg, m, **over):
    scene = api.create_scene(m.scene_params(pkg, **over))
    am.upload(api, scene, m)
    return scene


def raw(a):
    """The bytes of a result array, one row of 48 per element."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 48)


class Source:
    """Maps on the device with a point set and a ray set that meet them."""

    def __init__(self, scenes, poses, points, rays, maps=None):
        self.scenes, self.poses, self.points, self.rays, self.maps = scenes, [np.asarray(T, F) for T in poses], points, rays, maps


@pytest.fixture(scope="module")
def ramp(pkg, gpu):
    maps = qf.maps_of("ramp")
    return Source([upload_map(gpu, pkg, pm.m) for pm in maps], [pm.T for pm in maps], qf.points(), qf.ray_sets()["around"], maps)


@pytest.fixture(scope="module")
def slabs(pkg, gpu):
    maps = qf.maps_of("slabs")
    return Source([upload_map(gpu, pkg, pm.m) for pm in maps], [pm.T for pm in maps], qf.points(), qf.ray_sets()["scan"], maps)


@pytest.fixture(scope="module")
def room(pkg, gpu, synth):
    """One fused s_tiny room under the identity (fused_room of the composite tests): points inside its allocated blocks, rays
    from the last camera's centre."""
    wl = synth.s_tiny()
    scene, _, _ = util.run_sequence(gpu, pkg, wl, util.small_params(pkg, wl), 5)
    vs = float(F(wl.scene_kwargs["voxel_size"]))
    table = gpu.download_hash_table(scene)
    pos = table["pos"][table["ptr"] >= 0].astype(np.float64)
    rng = np.random.default_rng(3)
    pick = pos[rng.integers(0, len(pos), 2000)]
    points = ((pick * 8 + rng.uniform(0.0, 8.0, pick.shape)) * vs).astype(F)
    Minv = np.linalg.inv(np.asarray(wl.frame(4)[2], np.float64))
    d = np.concatenate([rng.uniform(-0.5, 0.5, (1500, 2)), np.ones((1500, 1))], axis=1) @ Minv[:3, :3].T
    rays = np.concatenate([np.broadcast_to(Minv[:3, 3], d.shape), d, np.full((1500, 1), 0.05), np.full((1500, 1), 5.0)], axis=1).astype(F)
    return Source([scene], [I4], points, rays)


@pytest.fixture(params=["ramp", "room"])
def source(request):
    return request.getfixturevalue(request.param)


def query(gpu, src, points=None, what=7, scenes=None, poses=None):
    return gpu.query_points(src.scenes if scenes is None else scenes, src.poses if poses is None else poses,
                            src.points if points is None else points, what)


def cast(gpu, src, rays=None, what=7, max_range=0.0, scenes=None, poses=None):
    return gpu.cast_rays(src.scenes if scenes is None else scenes, src.poses if poses is None else poses,
                         src.rays if rays is None else rays, max_range, what)


# ---------------------------------------------------------------------------------------------------------------------
# 1. laws that hold bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_the_sources_are_not_trivial(gpu, ramp, room):
    for src in (ramp, room):
        p, r = query(gpu, src), cast(gpu, src)
        assert (p["found_lo"] != 0).mean() > 0.5 and (p["status"] == 0).all()
        assert (r["status"] > 0).sum() > 0.5 * len(r) and (r["status"] == 0).sum() >= 10
        assert np.abs(p["grad"]).max() > 0.1 and p["colour"].max() > 0.1 and np.abs(r["normal"]).max() > 0.5


def test_permuting_the_inputs_permutes_the_outputs(gpu, source):
    perm = np.random.default_rng(5).permutation(len(source.points))
    assert np.array_equal(raw(query(gpu, source, source.points[perm])), raw(query(gpu, source))[perm])
    perm = np.random.default_rng(6).permutation(len(source.rays))
    assert np.array_equal(raw(cast(gpu, source, source.rays[perm])), raw(cast(gpu, source))[perm])


def test_splitting_a_batch_changes_nothing(gpu, source):
    pts, rays = source.points[:1000], source.rays[:1000]
    whole_p, whole_r = raw(query(gpu, source, pts)), raw(cast(gpu, source, rays))
    for k in SPLITS:
        k = k % len(pts)
        assert np.array_equal(np.concatenate([raw(query(gpu, source, pts[:k])), raw(query(gpu, source, pts[k:]))]), whole_p), k
        assert np.array_equal(np.concatenate([raw(cast(gpu, source, rays[:k])), raw(cast(gpu, source, rays[k:]))]), whole_r), k


def test_host_form_equals_device_form(pkg, gpu, source):
    import torch
    for host, arr, call in ((query(gpu, source), source.points, gpu.query_points_device), (cast(gpu, source), source.rays, gpu.cast_rays_device)):
        n = len(arr)
        d_in = torch.from_numpy(np.array(arr)).to("cuda:0")
        d_out = torch.full((n * 48,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        call(source.scenes, source.poses, d_in.data_ptr(), n, d_out.data_ptr())
        gpu.synchronize()
        assert np.array_equal(d_out.cpu().numpy().reshape(n, 48), raw(host))


def test_a_batch_above_one_chunk_equals_its_halves(gpu, ramp):
    """2^20 + 3 points (the 4096 of the fixture, repeated): the host form stages them in two chunks."""
    n = (1 << 20) + 3
    pts = np.resize(ramp.points, (n, 3))
    whole = raw(query(gpu, ramp, pts))
    half = n // 2
    assert np.array_equal(whole[:half], raw(query(gpu, ramp, pts[:half])))
    assert np.array_equal(whole[half:], raw(query(gpu, ramp, pts[half:])))
    assert np.array_equal(whole, np.resize(raw(query(gpu, ramp)), (n, 48)))


@pytest.mark.parametrize("extra", ["empty", "far"])
def test_a_map_that_holds_nothing_here_changes_nothing(pkg, gpu, source, extra):
    s0 = source.scenes[0]
    if extra == "empty":
        s, T = gpu.create_scene(s0.params), util_pose(yaw=0.3, t=(0.1, 0.0, -0.2))
    else:
        m = am.build_map(am.Sphere((0.0, 0.0, 0.5), 0.3), s0.params.voxel_size, s0.params.mu, (-0.35, -0.35, 0.15), (0.35, 0.35, 0.85))
        s, T = upload_map(gpu, pkg, m), util_pose(t=(100.0, 0.0, 0.0))
    scenes, poses = source.scenes + [s], source.poses + [T]
    assert np.array_equal(raw(query(gpu, source, scenes=scenes, poses=poses)), raw(query(gpu, source)))
    assert np.array_equal(raw(cast(gpu, source, scenes=scenes, poses=poses)), raw(cast(gpu, source)))


def util_pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    import multimesh_fixtures as fx
    return np.asarray(fx.pose(yaw=yaw, pitch=pitch, roll=roll, t=t), F)


def test_list_order_where_exactly_one_map_reports_found(gpu, ramp):
    ab = query(gpu, ramp)
    ba = query(gpu, ramp, scenes=ramp.scenes[::-1], poses=ramp.poses[::-1])
    one = np.isin(ab["found_lo"], (1, 2))
    assert one.sum() >= 100 and (ab["found_lo"] == 1).sum() >= 20 and (ab["found_lo"] == 2).sum() >= 20
    assert np.array_equal(ba["found_lo"][one], 3 - ab["found_lo"][one])
    for field in ("sdf", "weight", "grad", "colour", "status", "found_hi"):
        assert np.array_equal(ab[field][one].view(np.uint32), ba[field][one].view(np.uint32)), field


def test_what_subsets_share_their_fields_bit_for_bit(pkg, gpu, source):
    full_p, full_r = query(gpu, source), cast(gpu, source)
    for what in (pkg.QUERY_SDF, pkg.QUERY_SDF | pkg.QUERY_GRADIENT, pkg.QUERY_SDF | pkg.QUERY_COLOUR):
        p, r = query(gpu, source, what=what), cast(gpu, source, what=what)
        for field in ("sdf", "weight", "found_lo", "found_hi", "status"):
            assert np.array_equal(p[field].view(np.uint32), full_p[field].view(np.uint32)), (what, field)
        for field in ("t", "point", "status", "steps"):
            assert np.array_equal(r[field].view(np.uint32), full_r[field].view(np.uint32)), (what, field)
        for bit, pf_, rf_ in ((pkg.QUERY_GRADIENT, "grad", "normal"), (pkg.QUERY_COLOUR, "colour", "colour")):
            if what & bit:
                assert np.array_equal(p[pf_].view(np.uint32), full_p[pf_].view(np.uint32)), (what, pf_)
                assert np.array_equal(r[rf_].view(np.uint32), full_r[rf_].view(np.uint32)), (what, rf_)
            else:
                assert not p[pf_].view(np.uint32).any() and not r[rf_].view(np.uint32).any(), (what, pf_)
    # rays need no DSLAM_QUERY_SDF
    assert np.array_equal(raw(cast(gpu, source, what=pkg.QUERY_GRADIENT | pkg.QUERY_COLOUR)), raw(full_r))


def test_a_point_query_at_a_hit_point_returns_the_rays_shading(gpu, source):
    """colour bit for bit; grad normalised as the ray kernel normalises it (1 / sqrt of the float32 sum of squares, x, y, z in
    that order, then one product per component) is the ray's normal bit for bit."""
    r = cast(gpu, source)
    hit = r["status"] > 0
    p = query(gpu, source, r["point"][hit])
    assert hit.sum() > 500 and (p["status"] == 0).all()
    assert np.array_equal(p["colour"].view(np.uint32), r["colour"][hit].view(np.uint32))
    g = p["grad"]
    length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2], dtype=F)
    assert length.dtype == F
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where((length == 0)[:, None], F(0), g * (F(1) / length)[:, None]).astype(F)
    assert np.array_equal(n.view(np.uint32), r["normal"][hit].view(np.uint32))
    assert (length > 0).sum() > 500
    assert not raw(r[~hit])[:, :40].any()   # a miss carries nothing but its status (0) and its steps


def test_stored_voxels_read_at_their_centres(pkg, gpu):
    """One identity map with a voxel size of 2^-7 m (so that a voxel's centre in metres and back is exact): at 500 stored
    voxels whose 8 taps are all resident the sdf is float32(raw) / float32(32767) and the weight the stored w_depth."""
    vs = 2.0 ** -7
    m = am.build_map(am.Sphere((0.05, -0.03, 0.6), 0.2), vs, 4 * vs, (-0.2, -0.3, 0.35), (0.3, 0.2, 0.85),
                     w_depth_field=lambda p: 1 + wf.texture(p))
    scene = upload_map(gpu, pkg, m)
    rng = np.random.default_rng(9)
    b = m.block_pos[rng.integers(0, len(m.block_pos), 4000)].astype(np.int64) * 8 + rng.integers(0, 8, (4000, 3))
    corners = b[:, None, :] + np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)])[None]
    p = b[m.lookup(corners)[2].all(axis=1)][:500]
    assert len(p) == 500
    s16 = m.lookup(p)[0]
    assert (np.abs(s16) < 32767).sum() > 100
    out = gpu.query_points([scene], [I4], (p * vs).astype(F), pkg.QUERY_SDF)
    assert np.array_equal(out["sdf"], s16.astype(F) / F(32767))
    assert np.array_equal(out["weight"], m.lookup_weights(p)[0].astype(F))
    assert (out["found_lo"] == 1).all() and (out["status"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. points against float64
# ---------------------------------------------------------------------------------------------------------------------
def _points_against_float64(what, gpu, src, maps, pts, ref=None):
    """Every field of dslam_query_points within query_bounds.point_bounds of ref64_query.sample_points, point by point.
    The bound is derived there: the transform's rounding (DELTA_U = sqrt(3) + 3.5 spacings of float32 at twice the largest
    coordinate) times the slope of each map's read at the point, taken from the cell's stored taps, pushed through the
    exact perturbation formula of the weighted blend, plus the roundings of the 8-term trilinear sums (12 x 2^-24), of the
    gradient's sums (19 x 2^-24) and of the n-map blend ((2 n + 1) x 2^-24).  `found` is compared off the reference's
    boundary ties that decide something (_floor_flip, with the transform's rounding as the tolerance), the values off every
    point that close to a cell boundary (its neighbour cell's slope is not in the bound).

    Measured on an MI355X, largest error / bound over the compared points: 0.14 and below at the origin (the colour), 0.07 and
    below at FAR[0]; the table is in DESIGN.md section 31."""
    b = qb.point_bounds(maps, pts)
    ref = rq.sample_points(maps, pts, tie_tol=b["delta"]) if ref is None else ref
    got = gpu.query_points(src.scenes, src.poses, pts)
    found = np.stack([(got["found_lo"] >> i) & 1 for i in range(len(maps))], axis=1).astype(bool)
    assert (got["status"] == 0).all() and not got["found_hi"].any()
    assert np.array_equal(found[~ref["tie"]], ref["found"][~ref["tie"]])
    ok = ~ref["tie"] & ~b["near_cell"]
    # (a coordinate lies within delta of a cell boundary with probability 2 delta, and there are three per map: far from the
    # origin, where delta is 0.04 voxel, that leaves 6 points in 10)
    assert ok.sum() >= 0.9 * (1.0 - 2.0 * b["delta"]) ** (3 * len(maps)) * len(pts)
    assert ref["found"].all(1)[ok].sum() >= 1000 and (ref["found"].sum(1) == 1)[ok].sum() >= 100
    worst = {}
    for field in ("sdf", "weight", "grad", "colour"):
        err = np.abs(got[field].astype(np.float64) - ref[field])[ok]
        bound = b[field][ok]
        assert np.isfinite(bound).mean() > 0.9, field     # (infinite: weights within reach of the transform's rounding)
        worst[field] = (err.max(), float(np.max(err / np.maximum(bound, 1e-300))))
    print(f"{what}: {ok.sum()} points compared, P = {b['P']:.0f} voxels, delta = {b['delta']:.3g} voxel; largest error (largest error / bound): "
          + ", ".join(f"{k} {v[0]:.3g} ({v[1]:.3g})" for k, v in worst.items()))
    for field, (_, ratio) in worst.items():
        assert ratio <= 1.0, f"{what}: {field} is {ratio:.3g} x its bound"


@pytest.mark.parametrize("name", ["ramp", "slabs"])
def test_points_against_float64(gpu, ramp, slabs, name):
    src = ramp if name == "ramp" else slabs
    _points_against_float64(name, gpu, src, src.maps, qf.points())


def test_points_far_from_the_origin(pkg, gpu):
    """The ramp maps moved by FAR[0] blocks in their own frames, the world moved by the same vector: coordinates of 64 000
    voxels, where float32 is spaced 2^-7 voxel apart (at twice the coordinate).  The bound scales with that spacing, as
    DESIGN.md section 27 scales its bounds; nothing else in the check changes."""
    D = pf.FAR[0]
    maps = []
    shift = pf.shift_metres(D, am.VS)
    for pm in qf.maps_of("ramp"):
        T = pm.T.astype(np.float64).copy()
        T[:3, 3] = T[:3, 3] + shift - T[:3, :3] @ shift      # q' = R (p + shift) + t' = (R p + t) + shift
        maps.append(rm.Posed(pf.shift_map(pm.m, D), T.astype(F)))
    src = Source([upload_map(gpu, pkg, pm.m) for pm in maps], [pm.T for pm in maps], None, None, maps)
    pts = (qf.points().astype(np.float64) + shift).astype(F)
    _points_against_float64("ramp at FAR[0]", gpu, src, maps, pts)


# ---------------------------------------------------------------------------------------------------------------------
# 3. rays against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ramp", "slabs"])
@pytest.mark.parametrize("kind", ["scan", "around"])
def test_rays_against_float64(gpu, ramp, slabs, name, kind):
    """The composite raycast's acceptance: hit or miss equal off ties; the hit point within 1e-3 voxel off ties, at most 1 % of
    the hits beyond it and each of those a flagged tie; t within 1e-3 voxel x vs; the normal, where the reference's gradient
    is longer than 1e-3, within what 2 grey levels of a shaded image stand for per component (2 / (0.8 x 255) of n . l for
    any unit l); the colour within 1 / 255."""
    src = ramp if name == "ramp" else slabs
    rays, ref = qf.ray_sets()[kind], qf.ray_reference(name, kind)
    got = cast(gpu, src, rays)
    vs = float(F(am.VS))
    tie = ref["tie"]
    assert (got["status"] >= 0).all()
    assert np.array_equal((got["status"] > 0)[~tie], ref["hit"][~tie])
    assert np.array_equal(got["status"][~tie], ref["status"][~tie]) and np.array_equal(got["steps"][~tie], ref["steps"][~tie])
    both = (got["status"] > 0) & ref["hit"]
    err = np.linalg.norm(got["point"].astype(np.float64) / vs - ref["p"], axis=1)
    big = both & (err > 1e-3)
    sel = both & ~tie
    d_t = np.abs(got["t"].astype(np.float64) - ref["t"])[sel] / vs
    lit = ref["grad_length"][sel] > 1e-3
    d_n = np.abs(got["normal"].astype(np.float64)[sel] - ref["normal"][sel])[lit]
    d_c = np.abs(got["colour"].astype(np.float64)[sel] - ref["colour"][sel])
    print(f"{name} / {kind}: {both.sum()} hits, {sel.sum()} off a tie, |dpoint| <= {err[sel].max():.3g} voxel, |dt| <= {d_t.max():.3g} voxel, "
          f"normal within {d_n.max():.3g} on {lit.sum()} hits, colour within {d_c.max() * 255:.3g} / 255; {big.sum()} hits beyond 1e-3 voxel")
    assert both.sum() >= 1000
    assert not (big & ~tie).any(), f"|dpoint| up to {err[big & ~tie].max():.3g} voxel off a tie"
    assert big.sum() <= 0.01 * both.sum()
    assert d_t.max() <= 1e-3
    assert lit.sum() > 0.5 * sel.sum() and d_n.max() <= 2.0 / (0.8 * 255.0)
    assert d_c.max() <= 1.0 / 255.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_elements_inside_a_batch_leave_their_neighbours_alone(pkg, gpu, ramp):
    nan, inf = np.nan, np.inf
    rays = ramp.rays[:256].copy()
    clean_r = raw(cast(gpu, ramp, rays))
    bad = {10: (3, 0.0, 4, 0.0, 5, 0.0), 64: (0, nan), 65: (4, inf), 130: (6, -0.25), 200: (7, inf), 201: (1, 6000.0), 255: (6, nan)}
    for i, edits in bad.items():
        for col, val in zip(edits[::2], edits[1::2]):
            rays[i, col] = val
    got = cast(gpu, ramp, rays)
    keep = np.ones(len(rays), bool)
    keep[list(bad)] = False
    assert np.array_equal(raw(got)[keep], clean_r[keep])
    want = np.zeros(1, pkg.RAY_HIT_DTYPE)
    want["status"] = -1
    assert all(np.array_equal(raw(got[i:i + 1]), raw(want)) for i in bad)      # status -1, everything else 0

    pts = ramp.points[:256].copy()
    clean_p = raw(query(gpu, ramp, pts))
    bad = {0: (0, nan), 63: (1, inf), 64: (2, -inf), 129: (0, 5300.0), 255: (2, -5300.0)}    # 2^20 voxels of 5 mm: 5242.88 m
    for i, (col, val) in bad.items():
        pts[i, col] = val
    got = query(gpu, ramp, pts)
    keep = np.ones(len(pts), bool)
    keep[list(bad)] = False
    assert np.array_equal(raw(got)[keep], clean_p[keep])
    want = np.zeros(1, pkg.POINT_SAMPLE_DTYPE)
    want["sdf"], want["status"] = 1.0, pkg.QUERY_OUTSIDE
    assert all(np.array_equal(raw(got[i:i + 1]), raw(want)) for i in bad)      # sdf 1, status OUTSIDE, everything else 0
    inside = query(gpu, ramp, np.array([[5242.0, 0.0, 0.0]], F))               # just inside the range: read, nothing found
    assert inside["status"][0] == 0 and inside["sdf"][0] == 1.0 and inside["found_lo"][0] == 0


def test_ray_range_edges(pkg, gpu, ramp):
    vs = float(F(am.VS))
    away, o = np.array([0.0, 0.0, -1.0]), np.array([0.0, 0.0, -1.0])
    u = np.array([0.0, 0.0, -1.0])
    outside = wf.C_WORLD + (wf.RADIUS + 0.1) * u
    rays = np.array([
        [*o, *away, 0.3, 0.3],                  # t_min == t_max: a miss, never marched
        [*o, *away, 0.4, 0.3],                  # t_min > t_max
        [*o, *away, 0.0, 0.1],                  # 20 voxels of empty space: ceil(20 / 8) block steps
        [*o, *away, 0.0, 1e30],                 # empty space for ever: the default max_range ends it
        [*outside, *(-u), 0.0, 0.1 - vs],       # ends one voxel before map A's surface
        [*outside, *(-u), 0.0, 0.1 + 2 * vs],   # ... and two behind it
    ], F)
    one = Source(ramp.scenes[:1], ramp.poses[:1], None, rays)
    got = cast(gpu, one)
    ref = rq.cast_rays(ramp.maps[:1], rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    # (rays 0 and 3 end exactly where a step lands: t_min == t_max is decided by one comparison of two equal float32 products,
    # steps 0; 16384 voxels are 2048 block steps and the float32 total_max may lie an ulp above 16384, one step more)
    decided = [0, 1, 2, 4, 5]
    assert not ref["tie"][[1, 2, 4, 5]].any()
    assert list(got["status"]) == [0, 0, 0, 0, 0, 1] == list(ref["status"])
    assert list(got["steps"][:3]) == [0, 0, 3] and got["steps"][2] == int(np.ceil(F(0.1) / F(vs) / 8))
    assert pkg.QUERY_MAX_RAY_VOXELS // 8 <= got["steps"][3] <= pkg.QUERY_MAX_RAY_VOXELS // 8 + 1 <= pkg.QUERY_MAX_RAY_VOXELS
    assert np.array_equal(got["steps"][decided], ref["steps"][decided])
    assert not raw(got[:5])[:, :40].any()
    assert abs(got["t"][5] - 0.1) < vs and np.linalg.norm(got["point"][5] / vs - ref["p"][5]) <= 1e-3
    # a max_range of the caller's binds the same way (202 voxels: 26 block steps)
    short = cast(gpu, one, rays[3:4], max_range=1.01)
    assert short["steps"][0] == int(np.ceil(F(1.01) / F(vs) / 8)) == 26 and short["status"][0] == 0
    # a ray that starts behind the surface: a hit at the first read
    inside = wf.C_WORLD + (wf.RADIUS - 1.5 * am.VS) * u
    back = cast(gpu, one, np.array([[*inside, *(-u), 0.0, 0.5]], F))
    assert back["status"][0] == 2 and back["steps"][0] == 1 and back["t"][0] < 0


def test_no_elements(pkg, gpu, ramp):
    assert len(query(gpu, ramp, np.zeros((0, 3), F))) == 0 and len(cast(gpu, ramp, np.zeros((0, 8), F))) == 0
    gpu.query_points_device(ramp.scenes, ramp.poses, 0, 0, 0)       # n == 0: nothing is launched, nothing is read
    gpu.cast_rays_device(ramp.scenes, ramp.poses, 0, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg, gpu, ramp):
    S, T, pts, rays = ramp.scenes, ramp.poses, ramp.points[:8], ramp.rays[:8]
    limit = float(F(pkg.QUERY_MAX_RAY_VOXELS) * F(am.VS))
    sheared = T[0].copy()
    sheared[0, 1] += 0.1
    bad = [
        lambda: gpu.query_points([], np.zeros((0, 4, 4), F), pts),                          # no map
        lambda: gpu.query_points([S[0], S[0]], [T[0], T[1]], pts),                          # a scene twice
        lambda: gpu.query_points(S, [sheared, T[1]], pts),                                  # not rigid
        lambda: gpu.query_points([S[0], None], T, pts),                                     # a NULL scene
        lambda: gpu.query_points_device(S, T, 256, pkg.QUERY_MAX_ELEMENTS + 1, 256),        # n above the limit
        lambda: gpu.query_points_device(S, T, 256, -1, 256),                                # n negative
        lambda: gpu.cast_rays_device(S, T, 256, pkg.QUERY_MAX_ELEMENTS + 1, 256),
        lambda: gpu.query_points(S, T, pts, what=8 | pkg.QUERY_SDF),                        # unknown bits
        lambda: gpu.query_points(S, T, pts, what=pkg.QUERY_GRADIENT),                       # points without SDF
        lambda: gpu.cast_rays(S, T, rays, what=16),
        lambda: gpu.cast_rays(S, T, rays, max_range=-1.0),
        lambda: gpu.cast_rays(S, T, rays, max_range=float("nan")),
        lambda: gpu.cast_rays(S, T, rays, max_range=float("inf")),
        lambda: gpu.cast_rays(S, T, rays, max_range=limit * 1.01),
        lambda: gpu.query_points_device(S, T, 0, 8, 256),                                   # NULL arrays with n > 0
        lambda: gpu.query_points_device(S, T, 256, 8, 0),
        lambda: gpu.cast_rays_device(S, T, 0, 8, 256),
        lambda: gpu.cast_rays_device(S, T, 256, 8, 0),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.DslamError, match="status -1") as e:
            call()
        assert "status -1" in str(e.value), i
    assert np.array_equal(raw(cast(gpu, ramp, rays, max_range=limit)), raw(cast(gpu, ramp, rays)))   # the limit itself is the default
    assert np.array_equal(raw(query(gpu, ramp, pts)), raw(query(gpu, ramp)[:8]))
