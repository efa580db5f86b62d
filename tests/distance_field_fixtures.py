"""The grids of the distance-field tests (test_distance_field_ref.py, test_gpu_distance_field.py) on the two posed maps of
weighted_fixtures.ramp_spheres(), their reference states and distances (each computed once per process), and the seeded
random state arrays of the transform's own cases."""
import functools

import numpy as np

import analytic_maps as am
import ref_distance_field as rd
import weighted_fixtures as wf

LO = np.floor((wf.C_WORLD - 0.2) / am.VS).astype(np.int64)
GRIDS = {
    "A": rd.grid_of(LO + (-1, 3, 10), 2, (41, 37, 29)),
    "B": rd.grid_of(LO + (5, 20, 30), 1, (65, 40, 33)),
    "C": rd.grid_of(LO + (-6, -6, -6), 4, (19, 23, 17)),
}
# occupied, free, unknown cells of each grid under the default parameters
COUNTS = {"A": (17688, 17553, 8752), "B": (49095, 9255, 27450), "C": (2407, 2543, 2479)}
LARGEST_D2_A = 177

# the transform's own cases: (dims, seed density)
TRANSFORM_SHAPES = (((1, 1, 1), 1.0), ((1024, 3, 2), 0.002), ((3, 1024, 2), 0.002), ((2, 3, 1024), 0.002), ((65, 63, 17), 0.001),
                    ((64, 64, 64), 0.5))


def ramp_maps(which=(0, 1)):
    """[(block_pos, voxels, T)] of the ramp spheres, as ref_distance_field.mark takes them."""
    maps = wf.ramp_spheres()
    return [(maps[i].m.block_pos, maps[i].m.voxels, maps[i].T) for i in which]


@functools.lru_cache(maxsize=None)
def ramp_states(name, which=(0, 1), **kw):
    s = rd.mark(ramp_maps(which), GRIDS[name], am.VS, am.MU, **kw)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def ramp_distances(name, seeds=rd.SEED_OCCUPIED, max_cells=0):
    d = rd.edt(ramp_states(name), GRIDS[name], seeds, max_cells)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def random_states(dims, density, seed=0):
    """Random state bytes of grid `dims`: occupied (3) with probability `density`, the rest observed free (1) or unknown (0)
    half and half; bits 2 .. 7 random, for the transform reads bits 0 and 1 only."""
    rng = np.random.default_rng(1000 + seed)
    n = int(np.prod(dims))
    s = np.where(rng.random(n) < density, 3, rng.integers(0, 2, n)).astype(np.uint8)
    s |= (rng.integers(0, 64, n) << 2).astype(np.uint8)
    s.setflags(write=False)
    return s


def unit_grid(dims, cell=1):
    return rd.grid_of((0, 0, 0), cell, dims)
