"""The textured maps, depth and colour images the photometric depth-to-SDF tracker's tests share
(test_track_sdf_rgb_ref.py on the CPU, test_gpu_track_sdf_rgb.py on the GPU).  The surfaces are analytic_maps' tilted
plane and box corner; their colour is a sinusoidal texture of 8 cm period (16 voxels) in two directions, with a phase per
channel.  A view's depth is cast in closed form and quantised to millimetres as track_sdf_fixtures.Fixture does; its
colours are the texture at the closed-form hit points.  Each fixture and each reference run is computed once per process."""
import functools

import numpy as np

import analytic_maps as am
import ref64_checks as rc
import ref64_track_sdf as rt
import ref64_track_sdf_rgb as rr
import track_sdf_fixtures as fx

I4 = fx.I4
W, H = fx.W, fx.H
PERIOD = 0.08
OFFSET_B = 30.0     # fixture (c): the second map's colour is the first's plus this


def texture(x, period=PERIOD, offset=0.0):
    """[..., 3] in [48, 208] + offset at metric points x [..., 3]: two sinusoids, along x + z / 2 and along y + z / 2 (so
    that it varies along both in-plane directions of the tilted plane and on all three walls of the box corner)."""
    x = np.asarray(x, np.float64)
    u, v = (x[..., 0] + 0.5 * x[..., 2]) * (2 * np.pi / period), (x[..., 1] + 0.5 * x[..., 2]) * (2 * np.pi / period)
    ph = np.array([0.0, 1.1, 2.3])
    return 128.0 + offset + 40.0 * np.sin(u[..., None] + ph) + 40.0 * np.sin(v[..., None] + 1.7 * ph)


def view_colours(geom, M, intr, w, h, colour):
    """RGBA [h, w, 4] uint8: `colour` at the points where the pixels' rays meet `geom` from world -> camera pose M (both in
    the geometry's frame); alpha 255, black where no surface is met."""
    ys, xs = np.mgrid[0:h, 0:w]
    fx_, fy_, cx, cy = (float(v) for v in intr)
    inv = np.linalg.inv(np.asarray(M, np.float64))
    dirs = np.stack([(xs - cx) / fx_, (ys - cy) / fy_, np.ones((h, w))], -1) @ inv[:3, :3].T
    z = geom.ray_depth(inv[:3, 3], dirs)
    hit = np.isfinite(z)
    pts = inv[:3, 3] + np.where(hit, z, 0.0)[..., None] * dirs
    out = np.zeros((h, w, 4), np.uint8)
    out[..., :3] = np.where(hit[..., None], np.clip(np.floor(colour(pts)), 0, 255), 0).astype(np.uint8)
    out[..., 3] = 255
    return out


class Fixture(fx.Fixture):
    """track_sdf_fixtures.Fixture with the view's colour image rgba [h, w, 4]; colour: the texture in the geometry's frame."""

    def __init__(self, name, maps, T, geom, G, M_geom, intr, w=W, h=H, colour=texture):
        super().__init__(name, maps, T, geom, G, M_geom, intr, w, h)
        self.geom, self.G = geom, np.asarray(G, np.float64)
        self.rgba = view_colours(geom, self.M_true.astype(np.float64) @ np.linalg.inv(self.G), self.intr, w, h, colour)

    def greys(self, levels=3):
        return rr.grey_pyramid(self.rgba, levels)

    def moved(self, along=(0.0, 0.0), spin_mrad=0.0):
        """The true pose after the scene has slid `along` (voxels, the plane's two in-plane axes) and turned by spin_mrad
        about the plane's normal through the scene's centre: the motions a plane's shape cannot see."""
        n = self.geom.n
        a1 = np.array([0.0, 1.0, 0.0])
        a1 = a1 - (a1 @ n) * n
        a1 /= np.linalg.norm(a1)
        a2 = np.cross(n, a1)
        Rg = self.G[:3, :3].T                                       # the geometry's axes in the world
        t = self.vs * (along[0] * (Rg @ a1) + along[1] * (Rg @ a2))
        D = rt.rigid(spin_mrad * 1e-3, Rg @ n, t, self.corners.mean(0))
        return (self.M_true.astype(np.float64) @ D).astype(np.float32)

    def starts(self):
        """The four starts of the whole runs: a slide along each in-plane axis, a slide with a spin about the normal, and
        track_sdf_fixtures' 5 mrad / 1 voxel."""
        return [self.moved((1.0, 0.0)), self.moved((0.0, 1.5)), self.moved((0.8, -0.8), 4.0), self.start()]


def _plane_camera(w, h):
    """ref64_checks.camera turned a little: from the unturned camera under the identity a point's z is its depth, whose
    millimetres are whole fifths of a voxel, and every pose that only slides has one pixel in six on a cell boundary.
    (The turn is small: the map has to cover the view, or pixels at its rim come and go with the pose at the price of the gate.)"""
    return rc.camera(w, h, yaw=0.012, pitch=-0.009, roll=0.02)


@functools.lru_cache(maxsize=None)
def textured_plane_map():
    return am.tilted_plane(colour=texture)


@functools.lru_cache(maxsize=None)
def plane(w=W, h=H):
    """(a) the textured tilted plane under the identity; (g) at 70 x 45, (h) at 416 x 320."""
    m = textured_plane_map()
    M, intr = _plane_camera(w, h)
    return Fixture(f"textured plane {w} x {h}", [m], [I4], m.geom, np.eye(4), M, intr, w, h)


# world -> map of fixture (b): a rotated world
T_POSED = rt.rigid(0.35, (0.3, -0.5, 0.81), (0.04, -0.03, 0.05)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def posed_plane():
    """(b) the same map under a non-trivial world -> map transform: R_i^T h_i matters."""
    m = textured_plane_map()
    M, intr = _plane_camera(W, H)
    return Fixture("posed textured plane", [m], [T_POSED], m.geom, T_POSED.astype(np.float64), M, intr)


SHIFT_B = np.array([0.04, 0.0, 0.0])   # map B's frame: the world moved by one block along x


@functools.lru_cache(maxsize=None)
def two_maps():
    """(c) two overlapping maps of one plane: B's colour is A's plus OFFSET_B, their w_color fields are opposite ramps along
    x and their w_depth is a ramp along y, so the blended colour is decided by the colour weights alone."""
    a0 = textured_plane_map()
    n, c = a0.geom.n, a0.geom.c

    def ramp(P, x0):
        return np.clip(1 + (P[..., 0] - x0 + 90) // 3, 1, 60)

    def w_depth(P):
        return np.clip(1 + (P[..., 1] + 70) // 4, 1, 40)

    A = am.tilted_plane(colour=texture, w_color_field=lambda P: ramp(P, 0), w_depth_field=w_depth)
    geom_b = am.Plane(n, c + float(n @ SHIFT_B))
    B = am.build_map(geom_b, am.VS, am.MU, np.array((-0.45, -0.33, 0.15)) + SHIFT_B, np.array((0.45, 0.33, 0.85)) + SHIFT_B,
                     colour=lambda x: texture(x - SHIFT_B, offset=OFFSET_B), w_color_field=lambda P: 61 - ramp(P, 8),
                     w_depth_field=w_depth)
    T_b = np.eye(4, dtype=np.float32)
    T_b[:3, 3] = SHIFT_B
    M, intr = _plane_camera(W, H)
    return Fixture("two textured planes", [A, B], [I4, T_b], a0.geom, np.eye(4), M, intr)


def _holes(P, seed=5):
    b = np.asarray(P, np.int64) >> 3
    hsh = (b[..., 0] * 73856093) ^ (b[..., 1] * 19349669) ^ (b[..., 2] * 83492791) ^ seed
    return np.where(hsh % 4 == 0, 0, 1)


@functools.lru_cache(maxsize=None)
def colour_holes():
    """(d) plane (a) with w_color = 0 in a seeded quarter of the blocks."""
    m = am.tilted_plane(colour=texture, w_color_field=_holes)
    M, intr = _plane_camera(W, H)
    return Fixture("textured plane with colour holes", [m], [I4], m.geom, np.eye(4), M, intr)


@functools.lru_cache(maxsize=None)
def no_colour():
    """(e) a map without colour."""
    m = am.tilted_plane()
    M, intr = _plane_camera(W, H)
    return Fixture("plane without colour", [m], [I4], m.geom, np.eye(4), M, intr)


@functools.lru_cache(maxsize=None)
def box():
    """(f) the textured box corner: well conditioned without colour."""
    m = am.box_corner(colour=texture)
    M, intr = rc.camera(W, H, **fx.BOX_CAMERA)
    return Fixture("textured box corner", [m], [I4], m.geom, np.eye(4), M, intr)


def fixtures():
    """name -> fixture, all of them."""
    return {"a": plane(), "b": posed_plane(), "c": two_maps(), "d": colour_holes(), "e": no_colour(), "f": box(),
            "g": plane(70, 45), "h": plane(416, 320)}


def evaluation_pose(f):
    """The pose of the single evaluations: off the truth by a slide (where the fixture is a plane) or by 2 mrad / 0.3 voxel."""
    return f.moved((0.3, -0.2), 2.0) if isinstance(f.geom, am.Plane) else f.start(2.0, 0.3)


def reference_evaluation(f, pose, level=0, colour_levels=1, run_till_level=None, law="law", **kw):
    """ref64_track_sdf_rgb.evaluate of fixture f at `pose` on `level` of a call whose finest level is run_till_level
    (default: `level` itself)."""
    depth, intr = rt.pyramid(f.depth0, f.intr, level + 1)[level]
    till = level if run_till_level is None else run_till_level
    grey = f.greys(level + 1)[level] if level - till < colour_levels else None
    return rr.evaluate(f.posed, depth, grey, intr, rt.camera_to_world(pose, f.vs), law=law, **kw)


RUN_PARAMS = dict(min_valid=100)   # level 2 of 96 x 72 has 432 pixels, below the default of 500


@functools.lru_cache(maxsize=None)
def reference_run(which, start):
    """ref64_track_sdf_rgb.track on fixture `which` ('a', 'b') from start `start` (0 .. 3), once per process:
    (fixture, start pose, pose, result)."""
    f = fixtures()[which]
    s = f.starts()[start]
    M, res = rr.track(f.posed, f.depth0, f.rgba, f.intr, s, **RUN_PARAMS)
    return f, s, M, res


@functools.lru_cache(maxsize=None)
def depth_only_run(which, start):
    """ref64_track_sdf.track (no photometric term) from the same start."""
    f = fixtures()[which]
    s = f.starts()[start]
    M, res = rt.track(f.posed, f.depth0, f.intr, s, **RUN_PARAMS)
    return f, s, M, res
