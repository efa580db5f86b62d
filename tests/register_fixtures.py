"""The analytic map pairs the registration tests share (test_register_ref.py on the CPU, test_gpu_register.py on the GPU):
a source map of a geometry and a destination map of the SAME surface built in a displaced frame (ref64_register.Moved), so
the true transform between the two maps is known.  Each pair and each reference run is computed once per process."""
import functools

import numpy as np

import analytic_maps as am
import ref64_register as rr

I4 = np.eye(4, dtype=np.float32)
AXIS, TDIR = (0.42, -0.61, 0.67), (0.53, 0.37, -0.76)   # neither axis-aligned
BOX_CENTRE = (0.07, 0.04, 0.46)
SPHERE_CENTRE = (0.03, -0.02, 0.45)

# name -> (rotation in rad about AXIS through the source's centre, translation in voxels along TDIR) of the true transform
STARTS = {"small": (7.1e-3, 1.5), "large": (32e-3, 6.5), "xl": (64e-3, 12.0), "xxl": (134e-3, 23.0)}


def true_transform(name, centre=BOX_CENTRE):
    ang, vox = STARTS[name]
    t = vox * am.VS * np.asarray(TDIR) / np.linalg.norm(TDIR)
    return rr.rigid(ang, AXIS, t, centre)


class Pair:
    def __init__(self, src, dst, X_true):
        self.src_map, self.dst_map, self.X_true = src, dst, np.asarray(X_true, np.float64)
        self.src, self.dst = rr.MapData.of_map(src), rr.MapData.of_map(dst)

    def distance(self, X):
        """Largest displacement, in voxels, of the source's bounding-box corners between X and the true transform."""
        return rr.pose_distance(X, self.X_true, self.src.corners(), am.VS)

    def difference(self, X):
        """(mrad, voxels at the source's centre) between X and the true transform."""
        a, t = rr.pose_difference(X, self.X_true, self.src.centre(), am.VS)
        return 1e3 * a, t


def _box_source(**kw):
    return am.build_map(am.BoxCorner((0.16, 0.12, 0.55)), am.VS, am.MU, (-0.10, -0.12, 0.30), (0.24, 0.20, 0.62), **kw)


@functools.lru_cache(maxsize=None)
def box_pair(name):
    X = true_transform(name)
    dst = am.build_map(rr.Moved(am.BoxCorner((0.16, 0.12, 0.55)), X), am.VS, am.MU, (-0.2, -0.22, 0.2), (0.34, 0.3, 0.72))
    return Pair(_box_source(), dst, X)


@functools.lru_cache(maxsize=None)
def holes_pair():
    """Source with holes and chains up to 8 (64 buckets), destination with holes: the small displacement."""
    X = true_transform("small")
    src = _box_source(holes=0.15, seed=5, num_buckets=0x40)
    dst = am.build_map(rr.Moved(am.BoxCorner((0.16, 0.12, 0.55)), X), am.VS, am.MU, (-0.2, -0.22, 0.2), (0.34, 0.3, 0.72),
                       holes=0.2, seed=9)
    return Pair(src, dst, X)


@functools.lru_cache(maxsize=None)
def negative_pair():
    """Both maps at negative block coordinates throughout: the corner of three walls in the octant x, y, z < 0."""
    geom = am.BoxCorner((-0.30, -0.25, -0.20))
    c = (-0.39, -0.33, -0.29)
    X = true_transform("small", c)
    src = am.build_map(geom, am.VS, am.MU, (-0.56, -0.49, -0.45), (-0.22, -0.17, -0.13))
    dst = am.build_map(rr.Moved(geom, X), am.VS, am.MU, (-0.66, -0.59, -0.55), (-0.16, -0.11, -0.07))
    assert src.block_pos.max() < 0 and dst.block_pos.max() < 0
    return Pair(src, dst, X)


@functools.lru_cache(maxsize=None)
def sphere_pair():
    """A sphere fixes its centre and nothing else: the front half of sphere_outside's sphere as the source, the whole sphere
    displaced by 2 voxels as the destination."""
    geom = am.Sphere(SPHERE_CENTRE, 0.16)
    X = rr.rigid(0.0, AXIS, 2.0 * am.VS * np.asarray(TDIR) / np.linalg.norm(TDIR))
    src = am.build_map(geom, am.VS, am.MU, (-0.17, -0.22, 0.24), (0.23, 0.18, 0.45))
    dst = am.build_map(rr.Moved(geom, X), am.VS, am.MU, (-0.22, -0.27, 0.19), (0.28, 0.23, 0.71))
    return Pair(src, dst, X)


@functools.lru_cache(maxsize=None)
def plane_pair():
    """A plane fixes one translation and two rotations."""
    src = am.tilted_plane()
    X = rr.rigid(5e-3, AXIS, 1.0 * am.VS * np.asarray(TDIR) / np.linalg.norm(TDIR), (0.0, 0.0, 0.5))
    dst = am.build_map(rr.Moved(src.geom, X), am.VS, am.MU, (-0.5, -0.38, 0.1), (0.5, 0.38, 0.9))
    return Pair(src, dst, X)


def off_lattice(mrad=2.0, voxels=0.3):
    """The identity start moved off the voxel lattice (the identity's q is integral: every voxel would be a tie)."""
    return rr.rigid(mrad * 1e-3, (0.3, 0.8, -0.52), voxels * am.VS * np.array([0.6, -0.64, 0.48]), BOX_CENTRE).astype(np.float32)


def near_truth(pair, mrad=2.0, voxels=0.4):
    """A start 2 mrad / 0.4 voxel from the pair's true transform (float32 entries, as the ABI takes them)."""
    D = rr.rigid(mrad * 1e-3, (0.3, 0.8, -0.52), voxels * am.VS * np.array([0.6, -0.64, 0.48]), pair.src.centre())
    return (D @ pair.X_true).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_run(kind, name=None, start="identity", max_evaluations=0):
    """ref64_register.register on a fixture pair, once per process.  start: 'identity', 'truth' or 'near'."""
    pair = {"box": box_pair, "holes": lambda _: holes_pair(), "negative": lambda _: negative_pair(),
            "sphere": lambda _: sphere_pair(), "plane": lambda _: plane_pair()}[kind](name)
    X0 = {"identity": I4, "truth": pair.X_true.astype(np.float32), "near": near_truth(pair)}[start]
    X, res = rr.register(pair.src, pair.dst, X0, max_evaluations=max_evaluations)
    return pair, X, res


def single_evaluations():
    """(name, pair, X0) of the single evaluations the GPU file compares sum by sum with the reference.  None starts at
    the identity or at a translation of whole voxels: there every q is integral and every voxel a tie."""
    small = box_pair("small")
    return [("box-corner at the small start", small, off_lattice()),
            ("box-corner 2 mrad / 0.4 voxel from the truth", small, near_truth(small)),
            ("holes and chains", holes_pair(), off_lattice()),
            ("negative block coordinates", negative_pair(), near_truth(negative_pair(), 3.0, 0.7))]
