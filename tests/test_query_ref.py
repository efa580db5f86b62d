"""The float64 reference of the point and ray queries (ref64_query.py) checked on its own, without an engine: against a scalar
loop over stored voxels, its tie shares on the ray sets of query_fixtures.py, the march's behaviour at a ray that begins
behind a surface, the iteration bound, and that the two laws a kernel must not follow lie far outside the point bounds."""
import numpy as np
import pytest

import analytic_maps as am
import query_bounds as qb
import query_fixtures as qf
import ref64_query as rq
import weighted_fixtures as wf


def test_sample_points_equals_a_scalar_loop_over_stored_voxels():
    maps = qf.maps_of("ramp")
    pts = np.concatenate([qf.points()[:100], qf.points()[-100:]])
    ref = rq.sample_points(maps, pts, what=rq.SDF)
    sdf, weight, found = rq.sample_points_scalar(maps, pts)
    assert np.array_equal(found, ref["found"])
    assert found.all(1).sum() >= 50 and (found.sum(1) == 1).sum() >= 5 and (~found.any(1)).sum() >= 5
    assert np.abs(sdf - ref["sdf"]).max() <= 1e-12
    assert np.abs(weight - ref["weight"]).max() <= 1e-11
    assert not ref["grad"].any() and not ref["colour"].any()   # not asked for


@pytest.mark.parametrize("name", ["ramp", "slabs"])
@pytest.mark.parametrize("kind", ["scan", "around"])
def test_the_ray_sets_hold_their_tie_cap(name, kind):
    r = qf.ray_reference(name, kind)
    hits = int(r["hit"].sum())
    share = (r["tie"] & r["hit"]).sum() / hits
    print(f"{name} / {kind}: {hits} hits of {qf.N_RAYS}, {share:.2%} of them ties, {int(r['tie'].sum())} ties in all")
    assert hits >= 1000 and qf.N_RAYS - hits >= 20
    assert share < 0.01
    assert (r["status"] >= 0).all() and r["steps"].max() < 100


def test_a_ray_that_starts_behind_the_surface_hits_at_its_first_read():
    """The march's law there is castRay's: the first nearest read is already <= 0 (or its trilinear read is), the loop breaks
    in its first iteration, and the two refinement steps walk sdf * mu / vs voxels along the ray -- backwards, the sdf being
    negative.  For a ray that entered the surface from outside (or starts just inside looking inwards) backwards is towards
    the surface; a ray that looks outwards from inside is walked deeper in.  Status 2 tells the caller that the point is
    not a first surface along the ray."""
    maps = qf.maps_of("ramp")
    u = np.array([0.0, 0.0, -1.0])
    inside = wf.C_WORLD + (wf.RADIUS - 1.5 * am.VS) * u     # 1.5 voxels behind A's surface, 3.5 behind B's
    outside = wf.C_WORLD + (wf.RADIUS + 0.1) * u
    r = rq.cast_rays(maps, [inside, outside, inside], [u, -u, -u], 0.0, 0.5)
    assert list(r["status"]) == [2, 1, 2] and list(r["steps"][[0, 2]]) == [1, 1] and r["steps"][1] > 1
    # the refinement moved both points against their ray's direction ...
    assert r["t"][0] < 0 and r["t"][2] < 0
    dist = np.linalg.norm(r["point"] - wf.C_WORLD, axis=1)
    # ... the inward-looking ray's to the blended surface (between A's at RADIUS and B's, 2 voxels further out), where the
    # ray from outside stops too; the outward-looking ray's deeper in than it began
    assert np.all((dist[1:] > wf.RADIUS) & (dist[1:] < wf.RADIUS + 2 * am.VS))
    assert dist[0] < wf.RADIUS - 1.5 * am.VS


def test_the_iteration_bound_and_the_rays_that_are_never_marched():
    maps = qf.maps_of("ramp")
    vs = float(np.float32(am.VS))
    away = np.array([0.0, 0.0, -1.0])
    o = np.array([0.0, 0.0, -1.0])
    nan, inf = np.nan, np.inf
    rays = np.array([
        [*o, *away, 0.0, 1e30],            # empty space for ever: the default max_range ends it
        [*o, *away, 0.0, 0.1],             # 20 voxels of empty space
        [*o, *away, 0.3, 0.3],             # t_min >= t_max
        [*o, *away, 0.4, 0.3],
        [*o, 0.0, 0.0, 0.0, 0.0, 1.0],     # no direction
        [nan, 0.0, 0.0, *away, 0.0, 1.0],
        [*o, inf, 0.0, 0.0, 0.0, 1.0],
        [*o, *away, -0.1, 1.0],            # t_min < 0
        [*o, *away, 0.0, inf],
        [6000.0, 0.0, 0.0, *away, 0.0, 1.0],   # beyond 2^20 voxels of 5 mm
    ], np.float32)
    r = rq.cast_rays(maps, rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7])
    assert list(r["status"]) == [0, 0, 0, 0, -1, -1, -1, -1, -1, -1]
    assert r["steps"][0] == rq.MAX_RAY_VOXELS // 8 and r["steps"][0] <= rq.MAX_RAY_VOXELS
    assert r["steps"][1] == int(np.ceil(float(np.float32(0.1)) / vs / 8.0)) == 3
    assert not r["steps"][2:].any()
    # a shorter max_range binds the same way
    r = rq.cast_rays(maps, rays[:1, :3], rays[:1, 3:6], 0.0, 1e30, max_range=1.01)
    assert r["steps"][0] == int(np.ceil(float(np.float32(1.01)) / vs / 8.0)) == 26


def test_the_laws_a_kernel_must_not_follow_lie_far_outside_the_point_bounds():
    """Where both maps hold the cell, the sdf blended with each map's mean weight, or with the nearest tap's weight in place of
    the trilinear one, differs from the law's by more than ten times the bound test_gpu_query.py holds an engine to (median
    over the ramp points)."""
    maps, pts = qf.maps_of("ramp"), qf.points()
    ref, b = qf.point_reference("ramp"), qb.point_bounds(maps, pts)
    both = ref["found"].all(1) & ~b["near_cell"] & ~ref["tie"]
    assert both.sum() >= 2000
    for name, alt in (("per-map mean weights", wf.mean_weight_maps(maps)), ("nearest tap's weight", wf.nearest_weight_maps(maps))):
        other = rq.sample_points(alt, pts, what=rq.SDF)
        ratio = np.median(np.abs(other["sdf"] - ref["sdf"])[both] / b["sdf"][both])
        print(f"{name}: median |sdf - law's| = {ratio:.0f} x the bound")
        assert ratio > 10.0, name
