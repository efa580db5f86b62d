"""Maps, poses and workloads moved by whole blocks, far from the world origin.

Every fixture that pins a kernel to an independent reference sits at the world origin; the engine's map does not.  Here a
map of analytic_maps.py and its camera, or a synth workload, are moved by an integer block vector D: the same voxels in
blocks `pos + D`, the geometry translated by t = 8 vs D, the pose M' = float32(M T(-t)).  The metric shift is formed with
the voxel size the engine holds (float32), so that block b of the moved map lies where the engine puts it and the moved
map is, voxel for voxel, the map at the origin.

Placements (D in blocks): NEAR, the eight sign combinations of (1000, 700, 1300); FAR, +-(8000, 8000, -8000); the edges,
chosen per map so that its largest block coordinate is LAST_BLOCK = 32766 on every axis (the engines add a block's corner
offset in 16 bits, so 32767 is not usable) or its smallest is FIRST_BLOCK = -32768.  P(m) is the largest |voxel
coordinate| of a map, the far corner's + 8 included, and u(P) the spacing of float32 there: the unit every bound of the
placement tests is stated in.
"""
import copy
import itertools

import numpy as np

import analytic_maps as am

F = np.float32
FIRST_BLOCK, LAST_BLOCK = -32768, 32766
NEAR = tuple(tuple(int(s * v) for s, v in zip(sg, (1000, 700, 1300))) for sg in itertools.product((1, -1), repeat=3))
FAR = ((8000, 8000, -8000), (-8000, -8000, 8000))
TIE_CAP = {"near": 0.05, "far": 0.10, "edge": 0.25}


def vs32(vs):
    """The voxel size as the engine holds it."""
    return float(F(vs))


def shift_metres(D, vs):
    return 8.0 * vs32(vs) * np.asarray(D, np.float64)


def edge_pos(block_pos):
    """D that puts the largest block coordinate of every axis at LAST_BLOCK."""
    return tuple(int(v) for v in LAST_BLOCK - np.asarray(block_pos, np.int64).max(axis=0))


def edge_neg(block_pos):
    """D that puts the smallest block coordinate of every axis at FIRST_BLOCK."""
    return tuple(int(v) for v in FIRST_BLOCK - np.asarray(block_pos, np.int64).min(axis=0))


def placements(block_pos, near=NEAR):
    """name -> (class, D) for a map or a block set at the origin."""
    out = {"near" + "".join("+" if v > 0 else "-" for v in D): ("near", D) for D in near}
    out["far+"], out["far-"] = ("far", FAR[0]), ("far", FAR[1])
    out["edge_pos"], out["edge_neg"] = ("edge", edge_pos(block_pos)), ("edge", edge_neg(block_pos))
    return out


def halved(D, k):
    """D halved k times (towards the origin, whole blocks)."""
    return tuple(int(v / 2 ** k) for v in D)


def P_of_blocks(block_pos):
    b = np.asarray(block_pos, np.int64)
    return int(max(np.abs(b * 8).max(), np.abs(b * 8 + 8).max()))


def P(m):
    return P_of_blocks(m.block_pos)


def u(p):
    return float(np.spacing(F(p)))


class _ShiftedColour:
    def __init__(self, colour, t):
        self.colour, self.t = colour, t

    def __call__(self, x):
        return self.colour(x - self.t)


def shift_map(m, D):
    """`m` moved by D blocks: a new analytic_maps.Map with the same voxels at block_pos + D, the geometry and the colour
    field translated by 8 vs D.  The table is rebuilt (the hash of a position changes), so the chains are new ones:
    `max_chain` of the result says how long."""
    D = np.asarray(D, np.int64)
    t = shift_metres(D, m.vs)
    pos = m.block_pos + D
    assert pos.min() >= FIRST_BLOCK and pos.max() <= LAST_BLOCK, "a fixture may not hold a block beyond -32768 .. 32766"
    g = copy.copy(m.geom)
    if isinstance(g, am.Plane):
        g.c = m.geom.c + float(g.n @ t)
    elif isinstance(g, am.Sphere):
        g.c = m.geom.c + t
    elif isinstance(g, am.BoxCorner):
        g.k = m.geom.k + t
    else:
        raise TypeError(type(g))
    colour = None if m.colour is None else _ShiftedColour(m.colour, t)
    out = am.Map(m.vs, m.mu, pos, m.voxels, m.num_buckets, m.num_excess, m.num_local_blocks, g, colour)
    if hasattr(m, "colour_grad"):
        out.colour_grad = m.colour_grad
    out.D = tuple(int(v) for v in D)
    return out


def shift_pose(M, D, vs):
    """World -> camera of the moved world: M T(-t) in float64, rounded to float32 once."""
    T = np.eye(4)
    T[:3, 3] = -shift_metres(D, vs)
    return (np.asarray(M, np.float64) @ T).astype(F)


class Shifted:
    """A synth workload in the world moved by D blocks: the same images, the moved poses."""

    def __init__(self, wl, D):
        self._wl, self.D = wl, tuple(int(v) for v in D)
        self._t = shift_metres(D, wl.scene_kwargs["voxel_size"])

    def __getattr__(self, name):
        return getattr(self._wl, name)

    def pose(self, i):
        T = np.eye(4)
        T[:3, 3] = self._t
        return T @ self._wl.pose(i)

    def frame(self, i):
        rgba, mm, _ = self._wl.frame(i)
        return rgba, mm, shift_pose(np.linalg.inv(self._wl.pose(i)), self.D, self._wl.scene_kwargs["voxel_size"])


# ---------------------------------------------------------------------------------------------------------------------
# which blocks a depth image can ask for, from the images alone, in float64: the check that no fusion
# fixture reaches past the last usable block
# ---------------------------------------------------------------------------------------------------------------------
EDGE_MARGIN = 0.05  # blocks (0.4 voxel) between the outermost point a fixture asks for and the end of the range


def requested_extent(depth_m, M, intr, vs, mu, frustum_max):
    """(lo, hi) [3], in blocks and not yet floored: the extent of the segments depth -+ mu along every valid pixel's ray,
    which hold every point the allocation pass asks a block for."""
    d = np.asarray(depth_m, np.float64)
    H, W = d.shape
    ok = (d > 0) & (d - mu > 0) & (d - mu < frustum_max)
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy, cx, cy = (float(v) for v in intr)
    ray = (np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(d)], -1) * d[..., None])[ok]
    n = np.linalg.norm(ray, axis=1)
    invM = np.linalg.inv(np.asarray(M, np.float64))
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for s in (-1.0, 1.0):
        pc = ray * (1.0 + s * mu / n)[:, None]
        b = (pc @ invM[:3, :3].T + invM[:3, 3]) / (8.0 * vs32(vs))
        lo, hi = np.minimum(lo, b.min(0)), np.maximum(hi, b.max(0))
    return lo, hi


def workload_extent(wl, frames, poses=None):
    """requested_extent over frames of a synth workload; `poses`: world -> camera matrices per frame, where a frame is
    fused under other poses than its own."""
    kw = wl.scene_kwargs
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i in frames:
        _, mm, M = wl.frame(i)
        for Mi in [M] + list((poses or {}).get(i, [])):
            a, b = requested_extent(mm.astype(np.float64) / 1000.0, Mi, wl.intr, kw["voxel_size"], kw["mu"], kw["frustum_max"])
            lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    return lo, hi


def edge_safe(lo, hi, pname, near=NEAR):
    """(class, D) of placement `pname` for a fusion fixture whose requests span lo .. hi (blocks, not floored): at an edge
    the outermost point lies EDGE_MARGIN inside the last or first block, so that block is asked for and none beyond."""
    if pname == "edge_pos":
        return "edge", tuple(int(v) for v in np.floor(LAST_BLOCK + 1 - EDGE_MARGIN - hi))
    if pname == "edge_neg":
        return "edge", tuple(int(v) for v in np.ceil(FIRST_BLOCK + EDGE_MARGIN - lo))
    return placements(np.zeros((1, 3), np.int64), near)[pname]


def assert_inside(lo, hi, D):
    """No point of lo .. hi moved by D lies in a block beyond FIRST_BLOCK .. LAST_BLOCK."""
    a, b = np.floor(lo + np.asarray(D)), np.floor(hi + np.asarray(D))
    assert a.min() >= FIRST_BLOCK and b.max() <= LAST_BLOCK, f"requests reach blocks {a} .. {b}"


# ---------------------------------------------------------------------------------------------------------------------
# the teeth
# ---------------------------------------------------------------------------------------------------------------------
def straddling_cells(block_pos):
    """Trilinear cells whose eight corners lie in more than one block of the set, both blocks present: counted as the
    face-adjacent block pairs times the 64 cells of a face."""
    where = {tuple(p) for p in np.asarray(block_pos, np.int64).tolist()}
    pairs = 0
    for p in where:
        for axis in range(3):
            q = list(p)
            q[axis] += 1
            pairs += tuple(q) in where
    return 64 * pairs


def teeth(table, D, edge=None):
    """Asserted on what an engine holds (`table`: its hash table), moved by D: every block lies on D's side of the origin
    on every axis (over a placement set the signs are spread, see `sign_coverage`); at an edge ("edge_pos", "edge_neg") a
    block sits exactly at the last or first coordinate on every axis; at least 20 trilinear cells straddle two blocks;
    at least one excess-chain link."""
    live = table[table["ptr"] >= 0]
    pos = live["pos"].astype(np.int64)
    assert len(pos) > 0
    sg = np.sign(np.asarray(D, np.int64))
    assert (np.sign(pos) == sg).all(), f"blocks {pos.min(axis=0)} .. {pos.max(axis=0)} are not all on the side of D = {D}"
    if edge == "edge_pos":
        assert (pos.max(axis=0) == LAST_BLOCK).all(), f"largest block {pos.max(axis=0)}"
    elif edge == "edge_neg":
        assert (pos.min(axis=0) == FIRST_BLOCK).all(), f"smallest block {pos.min(axis=0)}"
    cells = straddling_cells(pos)
    assert cells >= 20, f"{cells} straddling cells"
    links = int((table["offset"] >= 1).sum())
    assert links >= 1, "no excess-chain link"
    return dict(blocks=len(pos), straddling_cells=cells, chain_links=links, lo=pos.min(axis=0).tolist(), hi=pos.max(axis=0).tolist())


def sign_coverage(Ds):
    """Over a placement set, both signs occur on every axis."""
    s = np.sign(np.asarray(Ds, np.int64))
    return bool(((s > 0).any(axis=0) & (s < 0).any(axis=0)).all())
