"""The point and ray sets of the query tests (test_query_ref.py, test_gpu_query.py) on the weight-varying fixtures of
weighted_fixtures.py, and their float64 references; each built once per process."""
import functools

import numpy as np

import analytic_maps as am
import ref64_query as rq
import weighted_fixtures as wf

F = np.float32
N_POINTS, N_RAYS = 4096, 2048
SCAN_ORIGIN = np.array([0.021, -0.013, 0.052])


def maps_of(name):
    return wf.ramp_spheres() if name == "ramp" else wf.slab_spheres()


@functools.lru_cache(maxsize=None)
def points():
    """4096 world points (metres, float32): half C_WORLD + U(-0.2, 0.2)^3, half within +-1.5 voxel of sphere A's surface
    (the world sphere of radius RADIUS about C_WORLD); seed 11."""
    rng = np.random.default_rng(11)
    box = wf.C_WORLD + rng.uniform(-0.2, 0.2, (N_POINTS // 2, 3))
    u = rng.normal(size=(N_POINTS // 2, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    shell = wf.C_WORLD + u * (wf.RADIUS + rng.uniform(-1.5, 1.5, (N_POINTS // 2, 1)) * am.VS)
    pts = np.concatenate([box, shell]).astype(F)
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def ray_sets():
    """{"scan": rays, "around": rays}, each [2048, 8] float32 (origin, direction, t_min, t_max).  scan: one origin, un-normalised
    directions into the box about the spheres, t 0.1 .. 0.803; around: origins on a shell of 0.33 m about C_WORLD looking
    inwards, t 0 .. 0.601.  (0.803, not 0.8: a t_max a whole number of 8-voxel steps from t_min makes every ray that meets
    no block a tie of `total < total_max`.)"""
    rng = np.random.default_rng(7)
    n = N_RAYS
    out = {}
    o = np.broadcast_to(SCAN_ORIGIN, (n, 3))
    d = wf.C_WORLD + rng.uniform(-0.2, 0.2, (n, 3)) - o
    out["scan"] = np.concatenate([o, d, np.full((n, 1), 0.1), np.full((n, 1), 0.803)], axis=1).astype(F)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = wf.C_WORLD + 0.33 * u + rng.uniform(-0.01, 0.01, (n, 3))
    d = wf.C_WORLD + rng.uniform(-0.12, 0.12, (n, 3)) - o
    out["around"] = np.concatenate([o, d, np.zeros((n, 1)), np.full((n, 1), 0.601)], axis=1).astype(F)
    for r in out.values():
        r.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def point_reference(name):
    """ref64_query.sample_points of points() on fixture `name` ("ramp" / "slabs"), all fields."""
    return rq.sample_points(maps_of(name), points())


@functools.lru_cache(maxsize=None)
def ray_reference(name, kind):
    """ref64_query.cast_rays of ray set `kind` on fixture `name`, sharp tie flags, the default max_range."""
    r = ray_sets()[kind]
    return rq.cast_rays(maps_of(name), r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7], sharp_ties=True)
