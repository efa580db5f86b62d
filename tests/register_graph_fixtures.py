"""The analytic map sets the joint-registration tests share (test_register_graph_ref.py on the CPU,
test_gpu_register_graph.py on the GPU): three maps of the same box corner, map i built in a frame displaced by a known
T_i, so the true world -> map transforms are known (map 0 is the world).  Each set and each reference run is computed once
per process."""
import functools

import numpy as np

import analytic_maps as am
import ref64_register as rr
import ref64_register_graph as rg
import register_fixtures as fx

I4 = fx.I4
GEOM = (0.16, 0.12, 0.55)
AXIS2 = (0.2, 0.7, 0.3)
DIR2 = np.array([-0.5, 0.6, 0.62])

TRIANGLE = [(0, 1), (0, 2), (1, 2)]                  # every destination covers its source with a margin; anchor 0
RING = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0)]      # sources larger than destinations, free maps are sources; anchor 1


class MapSet:
    def __init__(self, maps, T_true):
        self.maps = maps
        self.T_true = [np.asarray(T, np.float64) for T in T_true]
        self.data = [rr.MapData.of_map(m) for m in maps]
        self.corners = self.data[0].corners()

    def distance(self, T, i):
        """Largest displacement, in voxels, of map 0's bounding-box corners between T and map i's true transform."""
        return rr.pose_distance(T, self.T_true[i], self.corners, am.VS)

    def pair_distance(self, T, s, d):
        """The same for the pair transform T_d T_s^-1 against the true one."""
        X = np.asarray(T[d], np.float64) @ np.linalg.inv(np.asarray(T[s], np.float64))
        return rr.pose_distance(X, self.T_true[d] @ np.linalg.inv(self.T_true[s]), self.corners, am.VS)


def _moved(T, lo, hi):
    return am.build_map(rr.Moved(am.BoxCorner(GEOM), T), am.VS, am.MU, lo, hi)


@functools.lru_cache(maxsize=None)
def map_set(name):
    """'small': T1 = true_transform('small'), T2 9 mrad / 2 voxels; 'large': T1 = true_transform('large'), T2 25 mrad / 5
    voxels."""
    if name == "small":
        T1, T2 = fx.true_transform("small"), rr.rigid(-9e-3, AXIS2, 2.0 * am.VS * DIR2, fx.BOX_CENTRE)
    else:
        T1, T2 = fx.true_transform("large"), rr.rigid(-25e-3, AXIS2, 5.0 * am.VS * DIR2, fx.BOX_CENTRE)
    maps = [fx._box_source(),
            _moved(T1, (-0.15, -0.17, 0.25), (0.29, 0.25, 0.67)),
            _moved(T2, (-0.2, -0.22, 0.2), (0.34, 0.3, 0.72))]
    return MapSet(maps, [np.eye(4), T1, T2])


# a start 3 m away: disjoint from everything (as test_register_ref.py::test_disjoint_maps)
FAR = rr.rigid(0.0, fx.AXIS, (3.0, 0.0, 0.0)).astype(np.float32)
# (map set, pairs, anchor, parameters) of a connected graph with an inactive pair: (0, 1) has 25395 candidates, fewer than
# min_valid, while (1, 0) and (1, 2) start with 33660 and 42698 valid voxels
INACTIVE_BETWEEN = ("small", [(0, 1), (1, 0), (1, 2)], 1, dict(min_valid=30000, max_evaluations=4))

CASES = {"triangle": ("small", TRIANGLE, 0), "large": ("large", TRIANGLE, 0), "ring": ("large", RING, 1)}


def identity_starts(n=3):
    return np.stack([I4] * n)


@functools.lru_cache(maxsize=None)
def reference_run(case, max_evaluations=0):
    """ref64_register_graph.register_graph on a case of CASES from identity starts, once per process."""
    name, pairs, anchor = CASES[case]
    ms = map_set(name)
    T, res = rg.register_graph(ms.data, identity_starts(), pairs, anchor, max_evaluations=max_evaluations)
    return ms, T, res


def off_lattice_starts():
    """The starts of the compared single joint evaluation: off the voxel lattice (the identity's q is integral)."""
    return np.stack([I4, fx.off_lattice(), fx.off_lattice(1.5, 0.45)])


@functools.lru_cache(maxsize=None)
def few_map():
    """The 5 blocks of the box source the surface passes through (as test_gpu_register.py::test_grid_coverage builds)."""
    m = fx.box_pair("small").src_map
    pick = np.argsort(np.abs(m.voxels["sdf"].astype(np.int64)).min(axis=1))[:5]
    return am.Map(m.vs, m.mu, m.block_pos[pick], m.voxels[pick], 0x400, 0x100, 0x100, m.geom)
