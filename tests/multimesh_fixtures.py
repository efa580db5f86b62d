"""The posed analytic maps the composite-mesh tests share (test_multimesh_ref.py on the CPU, test_gpu_multimesh.py on the
GPU), each built once, with its float64 reference (ref64_multimesh.mesh_maps) computed once."""
import functools

import numpy as np

import analytic_maps as am
import ref64_checks as rc
import ref64_multimap as rm
import ref64_multimesh as r64

I4 = np.eye(4, dtype=np.float32)


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """A rigid world -> map transform (metres)."""
    R = np.linalg.inv(rc.camera(8, 8, yaw=yaw, pitch=pitch, roll=roll)[0].astype(np.float64))[:3, :3]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def rot_x(angle, t):
    """World -> map: a rotation about the x axis, then a translation (metres)."""
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]
    T[:3, 3] = t
    return T.astype(np.float32)


COLOUR_A, COLOUR_B = (220.0, 40.0, 30.0), (30.0, 90.0, 230.0)


@functools.lru_cache(maxsize=None)
def two_spheres():
    """One world sphere seen by two local maps (the fixture of the composite-raycast test): radii r and r + 2 voxels,
    w_depth 5 / 20, w_color 1 / 3, one flat colour per map, each map built in its own frame under a non-trivial pose.
    Returns (maps, centre in the world, r)."""
    c_world, r = np.array([0.03, -0.02, 0.45]), 0.16
    T_a = pose(yaw=0.2, pitch=-0.1, t=(0.05, 0.02, -0.03))
    T_b = pose(yaw=-0.15, roll=0.2, t=(-0.04, 0.01, 0.06))
    maps = []
    for T, dr, wd, wc, clr in ((T_a, 0.0, 5, 1, COLOUR_A), (T_b, 2 * am.VS, 20, 3, COLOUR_B)):
        c = T[:3, :3].astype(np.float64) @ c_world + T[:3, 3]
        m = am.build_map(am.Sphere(c, r + dr), am.VS, am.MU, c - 0.2, c + 0.2,
                         colour=lambda x, clr=clr: np.broadcast_to(np.array(clr), x.shape))
        maps.append(rm.Posed(rm.set_weights(m, wd, wc), T))
    return maps, c_world, r


SEAM_Z = 0.5013          # the wall: the world plane z = SEAM_Z, seen from z < SEAM_Z
SEAM_X = 0.08            # A's last block column ends here (2 blocks of 8 voxels of 5 mm), in the world (A is at the identity)


@functools.lru_cache(maxsize=None)
def seam_planes():
    """One wall seen by two maps side by side, equal weights: A at the identity over x in [-0.32, 0.08), B under a rotation
    about x and a translation that is no multiple of the voxel size over x in about [-0.09, 0.31): a shared strip four
    blocks wide."""
    world = am.Plane((0.0, 0.0, -1.0), -SEAM_Z)
    A = am.build_map(world, am.VS, am.MU, (-0.30, -0.16, 0.42), (0.06, 0.16, 0.58),
                     colour=lambda x: np.broadcast_to(np.array((200.0, 60.0, 20.0)), x.shape))
    T = rot_x(0.12, (0.013, -0.021, 0.017))
    R = T[:3, :3].astype(np.float64)
    n = R @ world.n
    c = world.c + n @ T[:3, 3]
    corners = np.array([[x, y, z] for x in (-0.06, 0.30) for y in (-0.16, 0.16) for z in (0.42, 0.58)])
    local = corners @ R.T + T[:3, 3]
    B = am.build_map(am.Plane(n, c), am.VS, am.MU, local.min(0), local.max(0),
                     colour=lambda x: np.broadcast_to(np.array((20.0, 60.0, 200.0)), x.shape))
    return [rm.Posed(rm.set_weights(A, 10, 2), I4), rm.Posed(rm.set_weights(B, 10, 2), T)]


def seam_wall_offsets(pos):
    """Of a mesh [n, 3, 3] of seam_planes(): every vertex's distance from the wall in voxels, and whether it lies within 2
    voxels of a map's block edge inside the other map (A's at x = SEAM_X and y = -+0.16, B's first block column).

    The bounds the tests hold them to.  Where both maps are read in full, the blend of two equal fields is the field:
    0.25 voxel, as for the two spheres.  Within a voxel of such an edge the other map's read is partial: a share f of its
    trilinear weight is found and the missing taps enter its value as sdf 1 (the read of DESIGN section 10), so a
    lattice point at truncated distance v combines to (v + f (f v + 1 - f)) / (1 + f).  That is zero at
    v = -f (1 - f) / (1 + f^2), at most (sqrt(2) - 1) / 2 = 0.207 of mu = 4 voxels (at f = sqrt(2) - 1): 0.83 voxel off
    the wall.  A crossing between lattice points of different f, whose values are scaled by (1 + f^2) / (1 + f) in
    [0.83, 1], moves by at most |u1 u2| (a1 - a2) / (a1 u1 - a2 u2) <= 0.21 * (0.25 + 0.207) / 4 of mu = 0.10 voxel more.
    1 voxel in all: the crack the law accepts along a map's edge."""
    A, B = seam_planes()
    v = np.asarray(pos, np.float64).reshape(-1, 3)
    off = np.abs(v[:, 2] - SEAM_Z) / am.VS
    b_x0 = r64.live_blocks(B.m)[:, 0].min() * 8 * am.VS - float(B.T[0, 3])
    edge = ((np.abs(v[:, 0] - SEAM_X) <= 2 * am.VS) | (np.abs(v[:, 0] - b_x0) <= 2 * am.VS)
            | (np.abs(np.abs(v[:, 1]) - 0.16) <= 2 * am.VS))
    return off, edge


@functools.lru_cache(maxsize=None)
def reference(name):
    """mesh_maps (with colours) of a fixture, computed once per process."""
    return r64.mesh_maps(fixture(name), colour=True)


def fixture(name):
    """The list of posed maps of a fixture by its name."""
    if name == "weighted_spheres":   # weights that vary per voxel, and a slab of map 0 that weighs nothing
        import weighted_fixtures as wf   # (it imports this module)
        return wf.mesh_spheres()
    return two_spheres()[0] if name == "two_spheres" else seam_planes()
