"""The depth-to-SDF tracker's fixtures (track_sdf_fixtures.py) far from the world origin, in the two
ways a tracker meets large coordinates:

  far map    `identity_box` stays under the identity and its blocks move by D (placement_fixtures.shift_map), the camera with
             them (shift_pose): block coordinates up to 32766 / -32768 in the table probe and the 8-tap gather, and
             points next to the range guard |q| < 262144 at edge_neg;
  far world  `posed_box` and `ramp_spheres` keep their blocks near their own origins and the world moves: T' = float32(T
             T(-t)), the camera by shift_pose.  The map transform then subtracts two position-sized numbers.

The same image is tracked: the truth and the 5 mrad / 1 voxel start are the origin's, moved.  D is placement_fixtures'
placements of identity_box's blocks for every fixture, so a placement's name means one D.

Ties.  With the reference's derived window (max(TIE_Q, dq) per pixel and axis) the share of pixels the reference cannot
decide grows with u(P).  placement_fixtures.TIE_CAP is the share a placement class may have; where the reference alone
exceeds it at D, D is halved (placement_fixtures.halved) until it does not.  HALVINGS records how often, per fixture and
placement, from the reference's own evaluation of level 0 at the fixture's single-evaluation pose;
test_track_placement_ref.py asserts that the cap is met there and missed with one halving fewer.  The unhalved edges of the
far-map fixture are kept as cases of their own ("edge_pos!", "edge_neg!"): only there does a block sit at the last or first
coordinate.
"""
import functools

import numpy as np

import placement_fixtures as pf
import ref64_track_sdf as rt
import track_sdf_fixtures as fx

PLACEMENTS = ("near+-+", "near-+-", "far+", "far-", "edge_pos", "edge_neg")
UNHALVED = ("edge_pos!", "edge_neg!")
FIXTURES = {"identity": fx.identity_box, "posed": fx.posed_box, "ramp": fx.ramp_spheres}
FAR_MAP = ("identity",)

# times D is halved until the reference's tie share is within TIE_CAP of the placement's class (measured values: DESIGN
# section 28)
HALVINGS = {
    ("identity", "near+-+"): 0, ("identity", "near-+-"): 0, ("identity", "far+"): 2, ("identity", "far-"): 1,
    ("identity", "edge_pos"): 3, ("identity", "edge_neg"): 3,
    ("posed", "near+-+"): 0, ("posed", "near-+-"): 0, ("posed", "far+"): 1, ("posed", "far-"): 1,
    ("posed", "edge_pos"): 2, ("posed", "edge_neg"): 2,
    ("ramp", "near+-+"): 1, ("ramp", "near-+-"): 1, ("ramp", "far+"): 3, ("ramp", "far-"): 3,
    ("ramp", "edge_pos"): 3, ("ramp", "edge_neg"): 3,
}


def _all_placements():
    return pf.placements(fx.identity_box().maps[0].block_pos)


def placement(which, pname, halvings=None):
    """(class, D) of fixture `which` at `pname`; halvings: instead of the recorded number."""
    if pname in UNHALVED:
        assert which in FAR_MAP
        return _all_placements()[pname[:-1]]
    cls, D = _all_placements()[pname]
    return cls, pf.halved(D, HALVINGS[which, pname] if halvings is None else halvings)


class Placed:
    """A track_sdf_fixtures.Fixture moved by D blocks; the same attributes and methods."""

    def __init__(self, which, pname, cls, D):
        f = FIXTURES[which]()
        self.origin, self.which, self.pname, self.cls, self.D = f, which, pname, cls, tuple(int(v) for v in D)
        self.name = f"{f.name} at {pname} {self.D}"
        self.w, self.h, self.intr, self.mm, self.depth0, self.vs = f.w, f.h, f.intr, f.mm, f.depth0, f.vs
        self.far_map = which in FAR_MAP
        if self.far_map:
            self.maps, self.T = [pf.shift_map(m, D) for m in f.maps], list(f.T)
        else:
            self.maps, self.T = list(f.maps), [pf.shift_pose(t, D, f.vs) for t in f.T]
        self.M_true = pf.shift_pose(f.M_true, D, f.vs)
        self.corners = f.corners + pf.shift_metres(D, f.vs)
        # the largest |coordinate| in voxels a point of the image has in the world, and the spacing of float32 there
        self.P = float(np.abs(self.corners).max() / self.vs)
        self.u = pf.u(self.P)

    @functools.cached_property
    def posed(self):
        if self.far_map:
            return [rt.PosedMap(rt.MapData.of_map(m), t) for m, t in zip(self.maps, self.T)]
        return [rt.PosedMap(pm.data, t) for pm, t in zip(self.origin.posed, self.T)]

    def distance(self, M):
        return rt.pose_distance(M, self.M_true, self.corners, self.vs)

    def start(self, mrad=5.0, voxels=1.0):
        return pf.shift_pose(self.origin.start(mrad, voxels), self.D, self.vs)

    def single_pose(self):
        """The pose of the single evaluations: the origin's (track_sdf_fixtures.single_evaluations), moved."""
        return self.M_true if self.which == "identity" else self.start(2.0, 0.3)


@functools.lru_cache(maxsize=None)
def placed(which, pname, halvings=None):
    cls, D = placement(which, pname, halvings)
    return Placed(which, pname, cls, D)


@functools.lru_cache(maxsize=None)
def reference_evaluation(which, pname, halvings=None):
    """The reference's evaluation of level 0 at the single-evaluation pose, once per process."""
    f = placed(which, pname, halvings)
    return rt.evaluate(f.posed, f.depth0, f.intr, rt.camera_to_world(f.single_pose(), f.vs))


@functools.lru_cache(maxsize=None)
def reference_run(which, pname):
    """ref64_track_sdf.track on the placed fixture from its 5 mrad / 1 voxel start, once per process."""
    f = placed(which, pname)
    M, res = rt.track(f.posed, f.depth0, f.intr, f.start(), **fx.RUN_PARAMS)
    return f, M, res


def cases(whiches=tuple(FIXTURES), unhalved=True):
    out = [(w, p) for w in whiches for p in PLACEMENTS]
    if unhalved:
        out += [(w, p) for w in whiches if w in FAR_MAP for p in UNHALVED]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# measured constants: the float32 restatement (ref32_track_sdf.py, camera pivot) against the float64 reference, on the CPU,
# no engine involved; test_track_placement_ref.py asserts each one, the GPU file allows the engine twice as much (FMA
# contraction and the reduction order, as for the ray march's C_RAY)
# ---------------------------------------------------------------------------------------------------------------------
# single evaluations, the pixels the reference calls no tie: worst distance of the pivoted system per fixture and placement
# class; H_c relative to its largest entry, g_c relative to |g_c| (identity_box is evaluated at the true pose, where g_c
# nearly vanishes: its figures are its own and nobody else's)
H_DEV = {"identity": {"near": 8.0e-7, "far": 3.5e-6, "edge": 6.4e-5},
         "posed": {"near": 3.2e-6, "far": 8.0e-6, "edge": 1.7e-5},
         "ramp": {"near": 1.7e-7, "far": 5.5e-7, "edge": 2.6e-6}}
G_DEV = {"identity": {"near": 6.0e-3, "far": 7.0e-2, "edge": 1.3e-1},
         "posed": {"near": 7.6e-5, "far": 3.3e-4, "edge": 1.35e-3},
         "ramp": {"near": 7.2e-5, "far": 8.2e-5, "edge": 2.2e-4}}
# whole runs: worst excess of the restatement's distance to the truth over the reference's, in u(P) ...
RUN_EXCESS_U = 1.0
# ... and worst relative deviation of its conditioning, per placement class
COND_DEV = {"near": 2.2e-4, "far": 2.3e-4, "edge": 1.9e-3}
FACTOR = 2.0


def pivot_at(sums, c_rel):
    """(H_c [6, 6], g_c [6]) of camera-pivoted sums re-pivoted to the point c_rel (relative to the camera centre): linear in
    the sums, so that two evaluations' sums can be compared at one and the same pivot."""
    H = np.zeros((6, 6))
    for col, (k, j) in enumerate(rt._TRI):
        H[k, j] = H[j, k] = sums[col]
    S = np.eye(6)
    S[:3, 3:] = np.array([[0, c_rel[2], -c_rel[1]], [-c_rel[2], 0, c_rel[0]], [c_rel[1], -c_rel[0], 0]])
    return S @ H @ S.T, S @ np.asarray(sums[21:27]), S


def system_distance(sums, ev, tie_pixels=True, rows_at_world=False, allow=True):
    """How far the pivoted system of `sums` lies from the reference evaluation ev's, at the reference's centroid: (H distance /
    largest |H_c| entry, g distance / |g_c|), each less what the tie pixels may account for.
    tie_pixels: `sums` are over all pixels (an engine's), so the tie pixels' share is compared as the interval of their
    alternatives: its midpoint joins the reference and its half width, pivoted with |S|, is the allowance.  Otherwise `sums`
    are over the reference's non-tie pixels alone.  rows_at_world: the rows of `sums` were formed at the world origin (the
    law as it stood), so the centroid is t further away from their pivot.  allow=False: the plain distances, to be printed."""
    c_rel = ev.sums_no_tie[29:32] / ev.sums_no_tie[28]
    mid = 0.5 * (ev.tie_lo + ev.tie_hi) if tie_pixels else np.zeros(rt.NSUMS)
    half = 0.5 * (ev.tie_hi - ev.tie_lo) if tie_pixels else np.zeros(rt.NSUMS)
    H_ref, g_ref, S = pivot_at(ev.sums_no_tie + mid, c_rel)
    H, g, _ = pivot_at(np.asarray(sums, np.float64), c_rel + ev.t if rows_at_world else c_rel)
    aS = np.abs(S)
    H_allow = aS @ pivot_at(half, np.zeros(3))[0] @ aS.T
    g_allow = aS @ half[21:27]
    if not allow:
        H_allow, g_allow = 0.0, 0.0
    dH = np.maximum(np.abs(H - H_ref) - H_allow, 0.0).max() / np.abs(H_ref).max()
    dg = np.linalg.norm(np.maximum(np.abs(g - g_ref) - g_allow, 0.0)) / np.linalg.norm(g_ref)
    return float(dH), float(dg)
