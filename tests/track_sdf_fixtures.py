"""The depth images and posed maps the depth-to-SDF tracker's tests share (test_track_sdf_ref.py on the CPU,
test_gpu_track_sdf.py on the GPU).  The maps are those of register_fixtures.py and weighted_fixtures.py, placed under
non-trivial world -> map transforms; the depth images are cast in float64 from the maps' closed-form geometries
(analytic_maps: plane, sphere, box corner) under a known camera pose and quantised to int16 millimetres.  Each fixture and
each reference run is computed once per process."""
import functools

import numpy as np

import analytic_maps as am
import multimesh_fixtures as mf
import ref64_checks as rc
import ref64_track_sdf as rt
import ref64_tracker_checks as tc
import register_fixtures as rf
import weighted_fixtures as wf

I4 = np.eye(4, dtype=np.float32)
W, H = 96, 72
# world -> the frame the box-corner source map was built in
G_BOX = mf.pose(yaw=0.2, pitch=-0.1, t=(0.05, 0.02, -0.03)).astype(np.float64)
# the camera of the box-corner fixtures in the source map's frame: it sees the corner and a stretch of all three walls
BOX_CAMERA = dict(yaw=0.16, pitch=-0.12, t=(0.03, 0.02, 0.06), f_scale=1.6)


class Fixture:
    """maps: analytic_maps.Map per local map; T: world -> map per map (float32); geom, G: the closed-form surface and the
    world -> its frame transform; M_true: the world -> camera pose the depth image mm [H, W] was cast from."""

    def __init__(self, name, maps, T, geom, G, M_geom, intr, w=W, h=H):
        self.name, self.maps, self.w, self.h = name, maps, w, h
        self.T = [np.asarray(t, np.float32) for t in T]
        self.intr = np.asarray(intr, np.float32)
        self.M_true = (np.asarray(M_geom, np.float64) @ np.asarray(G, np.float64)).astype(np.float32)
        # cast in the geometry's own frame from the float32 pose the tests are given
        self.mm = tc.closed_form_depth_mm(geom, self.M_true.astype(np.float64) @ np.linalg.inv(G), self.intr, w, h)
        self.depth0 = rt.depth_level0(self.mm)
        self.vs = float(np.float32(maps[0].vs))

    @functools.cached_property
    def posed(self):
        return [rt.PosedMap(rt.MapData.of_map(m), t) for m, t in zip(self.maps, self.T)]

    @functools.cached_property
    def corners(self):
        """The 8 corners (metres, world) of the bounding box of the depth image's points under the true pose."""
        _, p, _ = rt.world_points(self.depth0, self.intr, rt.camera_to_world(self.M_true, self.vs), self.vs)
        lo, hi = p.min(0) * self.vs, p.max(0) * self.vs
        return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])

    def distance(self, M):
        """Largest displacement, in voxels, of those corners between the camera frames of M and of the true pose."""
        return rt.pose_distance(M, self.M_true, self.corners, self.vs)

    def start(self, mrad=5.0, voxels=1.0):
        """The true pose moved by a rotation about the scene's centre and a translation (float32, as the ABI takes it)."""
        c = np.append(self.corners.mean(0), 1.0)
        D = rt.rigid(mrad * 1e-3, (0.3, 0.8, -0.52), voxels * self.vs * np.array([0.6, -0.64, 0.48]),
                     (self.M_true.astype(np.float64) @ c)[:3])
        return (D @ self.M_true.astype(np.float64)).astype(np.float32)


def _box_geom():
    return am.BoxCorner((0.16, 0.12, 0.55))


@functools.lru_cache(maxsize=None)
def identity_box(w=W, h=H):
    """One map under the identity: the box-corner source of register_fixtures."""
    M, intr = rc.camera(w, h, **BOX_CAMERA)
    return Fixture("identity box", [rf.box_pair("small").src_map], [I4], _box_geom(), np.eye(4), M, intr, w, h)


@functools.lru_cache(maxsize=None)
def posed_box():
    """One posed map: the box-corner destination (the source's surface in a displaced frame) in a rotated world."""
    pair = rf.box_pair("small")
    M, intr = rc.camera(W, H, **BOX_CAMERA)
    return Fixture("posed box", [pair.dst_map], [pair.X_true @ G_BOX], _box_geom(), G_BOX, M, intr)


@functools.lru_cache(maxsize=None)
def ramp_spheres():
    """Two overlapping maps whose weights vary per voxel (weighted_fixtures.ramp_spheres: one world sphere with radius r in
    map A and r + 2 voxels in map B); the depth image is of the sphere of radius r + 1 voxel, so the two maps' values have
    opposite signs and the blend is decided by the weights."""
    maps = wf.ramp_spheres()
    M, intr = rc.camera(W, H)
    return Fixture("ramp spheres", [pm.m for pm in maps], [pm.T for pm in maps], am.Sphere(wf.C_WORLD, wf.RADIUS + am.VS),
                   np.eye(4), M, intr)


@functools.lru_cache(maxsize=None)
def three_maps():
    """Three maps: the box-corner source, a map that lies behind the camera (the negative-octant corner), and the box-corner
    destination with holes (one block in five left out)."""
    pair = rf.holes_pair()
    M, intr = rc.camera(W, H, **BOX_CAMERA)
    return Fixture("three maps", [rf.box_pair("small").src_map, rf.negative_pair().src_map, pair.dst_map],
                   [G_BOX, mf.rot_x(0.1, (0.0, 0.0, -0.3)), pair.X_true @ G_BOX], _box_geom(), G_BOX, M, intr)


@functools.lru_cache(maxsize=None)
def posed_plane():
    """One posed map of a tilted plane (register_fixtures.plane_pair's destination): a surface that fixes one translation
    and two rotations only, so it is evaluated and never run."""
    pair = rf.plane_pair()
    M, intr = rc.camera(W, H)
    return Fixture("posed plane", [pair.dst_map], [pair.X_true], pair.src_map.geom, np.eye(4), M, intr)


def single_evaluations():
    """(fixture, pose) of the single evaluations the GPU file compares sum by sum with the reference."""
    return [(identity_box(), identity_box().M_true), (posed_box(), posed_box().start(2.0, 0.3)),
            (ramp_spheres(), ramp_spheres().start(2.0, 0.3)), (three_maps(), three_maps().start(2.0, 0.3))]


RUN_PARAMS = dict(min_valid=100)   # level 2 of 96 x 72 has 432 pixels, below the default of 500


@functools.lru_cache(maxsize=None)
def reference_run(which):
    """ref64_track_sdf.track on fixture `which` from its 5 mrad / 1 voxel start, once per process."""
    f = {"identity": identity_box, "posed": posed_box, "ramp": ramp_spheres, "three": three_maps}[which]()
    M, res = rt.track(f.posed, f.depth0, f.intr, f.start(), **RUN_PARAMS)
    return f, M, res
