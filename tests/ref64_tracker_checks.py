"""Check bodies shared by test_oracle_tracker64.py (CPU oracle) and test_gpu_tracker64.py (HIP engine): the depth
tracker against the float64 reference of ref64_tracker.py on the exact maps of analytic_maps.py.

The scene side is what create_icp_maps leaves (read back with download_icp_maps and handed to the reference as data:
the raycast has its own check in ref64_checks.py); the view side is the closed-form depth image of the map's geometry
from a known camera pose, quantised to int16 millimetres and passed through view_update.

Tier (a), one evaluation: dslam_debug_icp_sums against ref64_tracker.evaluate with the derived rounding bound.
Tier (a), whole runs: track_camera against ref64_tracker.track.  Tier (b): the tracked pose against the true one."""
import math

import numpy as np

import analytic_maps as am
import placement_fixtures as pf
import ref64_checks as rc
import ref64_tracker as rt

TIE_SHARE = 0.01  # tie pixels per valid pixel, the cap check_raycast uses
ONE_EVALUATION = 1e30  # a termination threshold no step stays below: the loop ends after its first evaluation


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def perturbed(M, rot_deg, trans_m, axis=(0.42, -0.61, 0.67), tdir=(0.53, 0.37, -0.76)):
    """world -> camera pose `M` followed by a rotation of rot_deg about `axis` and a shift of trans_m along `tdir`
    (neither axis-aligned)."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(rot_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    D = np.eye(4)
    D[:3, :3] = np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)
    D[:3, 3] = trans_m * np.asarray(tdir) / np.linalg.norm(tdir)
    return (D @ np.asarray(M, np.float64)).astype(np.float32)


def closed_form_depth_mm(geom, M, intr, W, H):
    """The geometry's depth image from world -> camera pose M, int16 millimetres (0 where no surface is met or the
    depth leaves the 32 m range)."""
    ys, xs = np.mgrid[0:H, 0:W]
    fx, fy, cx, cy = (float(v) for v in intr)
    inv = np.linalg.inv(np.asarray(M, np.float64))
    dirs = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], -1) @ inv[:3, :3].T
    z = geom.ray_depth(inv[:3, 3], dirs)  # the camera-frame direction has z = 1: the ray parameter is the depth
    mm = np.rint(np.where(np.isfinite(z), z, 0.0) * 1000.0)
    return np.where((mm > 0) & (mm <= 32000), mm, 0).astype(np.int16)


def graded_holes(mm):
    """Holes (0 and > 32 m alternately) so that the 2x2 groups of the image hold 0, 1, 2, 3, 4 valid pixels in turn."""
    mm = mm.copy()
    H, W = mm.shape
    order = [(0, 0), (1, 1), (0, 1), (1, 0)]
    for gy in range(H // 2):
        for gx in range(W // 2):
            drop = (gx + 2 * gy) % 5  # pixels of this group to blank
            for k in range(min(drop, 4)):
                dy, dx = order[(k + gx) % 4]
                mm[2 * gy + dy, 2 * gx + dx] = 0 if (gx + gy + k) % 2 else 32500
    return mm


def keep_sparse(mm, every=6):
    """All holes except every sixth pixel of every sixth row: fewer than 100 valid pixels at 64x48, more than none,
    spread over all three walls so that the six parameters stay constrained."""
    out = np.zeros_like(mm)
    out[2::every, 3::every] = mm[2::every, 3::every]
    return out


class Setup:
    """A loaded analytic map with its ICP maps rendered from `M_map`, and a view of the geometry from `M_true`."""

    def __init__(self, api, pkg, m, W, H, map_cam, true_off=(1.0, 0.01), view_edit=None, M_true=None, fy_scale=1.0, D=None):
        """D: a placement (placement_fixtures.py, whole blocks): the map's blocks and geometry moved by shift_map, `M_map`
        and `M_true` by shift_pose; `self.D`, and `self.place(M)` moves any other pose of the origin's (a start) likewise."""
        self.D = None if D is None else tuple(int(v) for v in D)
        if D is not None:
            m = pf.shift_map(m, D)
        self.api, self.pkg, self.m, self.W, self.H = api, pkg, m, W, H
        self.M_map, self.intr = rc.camera(W, H, **map_cam)
        self.intr[1] *= np.float32(fy_scale)  # rc.camera gives fy = fx
        self.M_true = perturbed(self.M_map, *true_off) if M_true is None else np.asarray(M_true, np.float32)
        self.M_map, self.M_true = self.place(self.M_map), self.place(self.M_true)
        self.scene, self.rs = rc.load_map(api, pkg, m, W, H)
        api.get_image(self.scene, self.rs, self.M_map, self.intr, pkg.IMAGE_DEPTH)
        api.find_visible_blocks(self.scene, self.rs, self.M_map, self.intr)
        self.points, self.normals = api.create_icp_maps(self.scene, self.rs, self.M_map, self.intr)
        if api.has("download_icp_maps"):  # what the tracker will read (the oracle keeps its maps on the host: no such call)
            self.points, self.normals = api.download_icp_maps(self.rs)
        mm = closed_form_depth_mm(m.geom, self.M_true, self.intr, W, H)
        if view_edit is not None:
            mm = view_edit(mm)
        self.view = api.create_view(W, H)
        api.view_update(self.view, np.zeros((H, W, 4), np.uint8), mm)
        self.depth = api.download_view_depth(self.view)

    def place(self, M):
        return np.asarray(M, np.float32) if self.D is None else pf.shift_pose(M, self.D, self.m.vs)

    def track(self, start, **kw):
        return self.api.track_camera(self.view, self.rs, self.M_map, start, self.intr, self.pkg.TrackerParams(**kw))


# ---------------------------------------------------------------------------------------------------------------------
# tier (a): one evaluation
# ---------------------------------------------------------------------------------------------------------------------
def evaluation_cases():
    """name -> dict(map, W, H, levels, map_cam, and optionally true_off (deg, m), start_off (deg, m) of the start pose
    from the map pose, dist_thresh, view_edit, M_true builder, gate_share (required share of gated pixels at level 0),
    max_valid).  dist_thresh: the squared distance (m^2) from which on the gate rejects -- chosen per case against
    the offset between the view and the start pose so that it rejects part of the image."""
    box = lambda: am.box_corner(num_buckets=0x80)
    cam = dict(yaw=0.2, pitch=0.15)
    return {
        "box_64x48_small_perturbation": dict(map=box, W=64, H=48, levels=4, map_cam=cam, true_off=(0.13, 0.0017),
                                             dist_thresh=0.0031 ** 2),
        "box_70x45": dict(map=box, W=70, H=45, levels=4, map_cam=cam, true_off=(0.9, 0.011), dist_thresh=0.0123 ** 2),
        # fy = 1.17 fx: every other case has square pixels, where fx and fy (or cx and cy at 1:1) could be swapped unseen
        "box_70x45_fy_not_fx": dict(map=box, W=70, H=45, levels=3, map_cam=cam, true_off=(0.7, 0.009), dist_thresh=0.0117 ** 2,
                                    fy_scale=1.17),
        "box_640x480": dict(map=box, W=640, H=480, levels=5, map_cam=cam, true_off=(0.9, 0.011), dist_thresh=0.0123 ** 2),
        "plane_1226x370": dict(map=lambda: am.tilted_plane(num_buckets=0x100), W=1226, H=370, levels=3,
                               map_cam=dict(yaw=-0.05, roll=0.1), true_off=(0.7, 0.008), dist_thresh=0.0071 ** 2),
        "plane_holes_70x45": dict(map=lambda: am.tilted_plane(tilt_deg=35.0, holes=0.08, seed=3, num_buckets=0x40), W=70, H=45,
                                  levels=3, map_cam=dict(yaw=0.07, pitch=0.05, roll=0.2), true_off=(0.6, 0.006),
                                  # gate wide open: a cell with one corner on a hole would otherwise fail it anyway (its
                                  # interpolant is pulled towards (0, 0, 0)) and the hole rule could not be told from the gate
                                  dist_thresh=0.83 ** 2, view_edit=graded_holes),
        # the same rule where it decides: a finer image against the 4 cm blocks, more of them missing and the camera
        # rolled, so that the holes' slanted outlines are staircases of cells with exactly one hole corner -- at least
        # 20 view pixels on such cells for each of the four corners (asserted from the reference)
        "plane_holes_fine_203x131": dict(map=lambda: am.tilted_plane(tilt_deg=35.0, holes=0.27, seed=11, num_buckets=0x40), W=203,
                                         H=131, levels=2, map_cam=dict(yaw=0.07, pitch=0.05, roll=0.47), true_off=(0.6, 0.006),
                                         dist_thresh=0.83 ** 2, view_edit=graded_holes, one_hole_min=20),
        "sphere_inside_gate": dict(map=lambda: am.sphere_inside(num_buckets=0x400), W=64, H=48, levels=3,
                                   map_cam=dict(yaw=0.4, pitch=0.2, roll=0.2), true_off=(1.0, 0.01),
                                   dist_thresh=0.0087 ** 2, gate_share=(0.2, 0.8)),
        "box_scene_yawed_100deg": dict(map=box, W=64, H=48, levels=3, map_cam=cam, true_yaw=1.741,
                                       # gate wide open: a point behind the scene camera that projects back into the
                                       # image is far from what it lands on, and only q.z <= 0 may reject it
                                       dist_thresh=1.9 ** 2, expect="behind"),
        # 155 degrees: the view looks back along the x wall, whose points lie behind the scene camera inside the cone
        # that projects (mirrored) into its image, onto valid cells -- with the gate open nothing but q.z <= 0 rejects them
        "box_scene_yawed_155deg": dict(map=box, W=64, H=48, levels=2, map_cam=cam, true_yaw=2.705, dist_thresh=1.9 ** 2,
                                       expect="behind", behind_inside_min=200),
        "box_scene_yawed_25deg": dict(map=box, W=64, H=48, levels=3, map_cam=cam, true_yaw=0.437, dist_thresh=0.0123 ** 2, expect="outside"),
        "box_few_valid": dict(map=box, W=64, H=48, levels=1, map_cam=cam, true_off=(0.4, 0.004), dist_thresh=0.0123 ** 2,
                              view_edit=keep_sparse, max_valid=100),
    }


def _setup_case(api, pkg, c, D=None):
    M_true = None
    if "true_yaw" in c:  # the view camera yawed away from the scene camera, about the scene camera's own position
        cam = dict(c["map_cam"])
        cam["yaw"] = cam.get("yaw", 0.0) + c["true_yaw"]
        M_true = perturbed(rc.camera(c["W"], c["H"], **cam)[0], 0.3, 0.003)
    return Setup(api, pkg, c["map"](), c["W"], c["H"], c["map_cam"], c.get("true_off", (1.0, 0.01)), c.get("view_edit"), M_true,
                 c.get("fy_scale", 1.0), D=D)


def check_evaluations(api, pkg, case, D=None, tie_cap=TIE_SHARE):
    """Every level and iteration type of one case.  Returns the figures (tie share, worst |got - ref| / bound).
    D: the case moved by D blocks (Setup); the reference then derives its tie windows from its own bound, and tie_cap is the
    share of tie pixels the placement may have (placement_fixtures.TIE_CAP)."""
    c = evaluation_cases()[case]
    s = _setup_case(api, pkg, c, D)
    # the pose to evaluate at: the true view pose for the yawed cases (the scene pose is what differs); else a pose off
    # both the map pose (where every pixel would project onto an integer scene pixel: all ties) and the true one
    start = s.M_true if "true_yaw" in c else perturbed(s.M_map, 0.23, 0.0019, axis=(-0.31, 0.52, 0.8), tdir=(-0.4, 0.7, 0.59))
    pyr = rt.pyramid(s.depth, s.intr, c["levels"])
    inv = np.linalg.inv(np.asarray(start, np.float64))
    worst, worst_f, tie_share, n_valid = 0.0, 0.0, 0.0, []
    for level in range(c["levels"]):
        lv_depth, lv_intr = pyr[level]
        for type in (rt.ROTATION, rt.TRANSLATION, rt.BOTH):
            pose, res = s.track(start, levels=level + 1, run_till_level=level, regime=[rt.NONE] * level + [type],
                                dist_thresh=c["dist_thresh"], termination_threshold=ONE_EVALUATION)
            assert res.iterations == 1, f"{case} level {level} type {type}: {res.iterations} evaluations"
            got = api.debug_icp_sums()
            ev = rt.evaluate(lv_depth, lv_intr, s.points, s.normals, s.intr, inv, s.M_map, c["dist_thresh"], type,
                             derived_ties=D is not None)
            ref, ties = ev["sums"], int(ev["tie"].sum())
            valid = int(ref[28])
            what = f"{case} level {level} ({lv_depth.shape[1]}x{lv_depth.shape[0]}) type {type}"
            assert ties <= tie_cap * valid, f"{what}: {ties} tie pixels for {valid} valid ones"
            assert abs(got[28] - valid) <= ties, f"{what}: {int(got[28])} valid points, float64 reference {valid}"
            assert res.valid_points_last == int(got[28])
            npara = 6 if type == rt.BOTH else 3
            used = list(range(npara * (npara + 1) // 2)) + list(range(21, 21 + npara)) + [27]
            unused = [i for i in range(28) if i not in used]
            assert not np.any(got[unused]), f"{what}: unused slots are not zero"
            lim = ev["bound"] + ev["max_term"] * ties
            for i in used:
                d = abs(got[i] - ref[i])
                ratio = d / lim[i] if lim[i] > 0 else (0.0 if d == 0 else math.inf)
                print(f"{what} sum {i}: got {got[i]:.9g} ref {ref[i]:.9g} |d| {d:.3g} bound {lim[i]:.3g} ratio {ratio:.3g}")
                worst = max(worst, ratio)
                assert d <= lim[i], f"{what}: sum {i} off by {d:.3g}, rounding bound {lim[i]:.3g}"
            # f = sqrt(sum b^2) / valid, the same bound propagated (+ float conversion, sqrtf, division)
            f_ref = rt.error_value(ref[27], valid)
            if valid - ties > 100:
                f_lo, f_hi = rt.error_interval(ref[27], ev["bound"][27], ev["max_term"][27], valid, ties)
                print(f"{what} f: got {res.f_last:.9g} ref {f_ref:.9g} in [{f_lo:.9g}, {f_hi:.9g}]")
                assert f_lo <= res.f_last <= f_hi, f"{what}: f {res.f_last:.9g}, reference {f_ref:.9g}"
                if f_hi > f_lo:
                    worst_f = max(worst_f, abs(res.f_last - f_ref) / max(f_hi - f_ref, f_ref - f_lo))
            elif valid + ties <= 100:
                assert res.f_last == np.float32(1e5), f"{what}: f {res.f_last} with {valid} valid points"
            if valid:
                tie_share = max(tie_share, ties / valid)
            n_valid.append(valid)
            if level == 0 and type == rt.BOTH:
                print(f"{what}: {ev['behind']} behind the scene camera, {ev['outside']} outside the bounds, {ev['holes']} on holes")
                if "expect" in c:  # the case reaches the branch it is there for, on a large share of the image
                    assert ev[c["expect"]] > 0.2 * (lv_depth > 0).sum(), f"{what}: {ev[c['expect']]} pixels {c['expect']}"
                if c.get("view_edit") is graded_holes:
                    assert ev["holes"] > 0.05 * (lv_depth > 0).sum(), f"{what}: {ev['holes']} pixels next to a hole of the ICP map"
                if "behind_inside_min" in c:
                    print(f"{what}: {ev['behind_inside']} pixels behind the scene camera would pass every later test")
                    assert ev["behind_inside"] >= c["behind_inside_min"], f"{what}: {ev['behind_inside']} such pixels"
                if "one_hole_min" in c:
                    print(f"{what}: pixels on cells whose only hole is corner a / b / c / d: {ev['one_hole']}")
                    assert min(ev["one_hole"]) >= c["one_hole_min"], f"{what}: one-hole cells reached {ev['one_hole']}"
                if "gate_share" in c:
                    share = ev["gated"].sum() / max(1, ev["projected"].sum())
                    print(f"{what}: the distance gate rejects {share:.3f} of {ev['projected'].sum()} projected pixels")
                    assert c["gate_share"][0] <= share <= c["gate_share"][1], f"{what}: gate share {share:.3f}"
                if "max_valid" in c:
                    assert 0 < valid <= c["max_valid"], f"{what}: {valid} valid points"
                    # f = 1e5 < 1e20 is accepted: the pose moves by the step of this evaluation's own sums (a rejection
                    # would leave it at the start) ...
                    M_ref, _ = rt.apply_step(inv, _lm_step(ref, valid, npara), type)
                    moved = np.abs(M_ref - start).max()
                    assert np.abs(pose - M_ref).max() < 0.1 * moved, f"{what}: the f = 1e5 evaluation was not accepted"
                    # ... and so is the second one, whose f = 1e5 equals f_old (f_new > f_old is false): a rejection
                    # would go back to the start and take a step damped a hundred times as much
                    pose2, res2 = s.track(start, levels=1, regime=[type], dist_thresh=c["dist_thresh"], termination_threshold=0.0)
                    M_ref2, log = rt.track(s.depth, s.intr, s.points, s.normals, s.M_map, start, levels=1, regime=[type],
                                           dist_thresh=c["dist_thresh"], termination_threshold=0.0)
                    assert res2.iterations == 2 and [r["accepted"] for r in log] == [True, True] and log[1]["valid"] <= 100
                    assert np.abs(pose2 - M_ref2).max() < 0.1 * np.abs(M_ref2 - start).max(), f"{what}: equal f was not accepted"
    return dict(tie_share=tie_share, worst_ratio=worst, worst_f_ratio=worst_f, valid=n_valid)


def _lm_step(sums, valid, npara, lam=0.1):
    Hm, g = rt._full(sums, npara)
    A = Hm / valid
    A[np.diag_indices(npara)] *= 1.0 + lam
    return np.linalg.solve(A, g / valid)


# ---------------------------------------------------------------------------------------------------------------------
# tier (a): whole runs
# ---------------------------------------------------------------------------------------------------------------------
RUN_W, RUN_H = 160, 120


def run_cases():
    """name -> (tracker parameters, start offset (deg, m) from the map pose, needs a rejected iteration)."""
    return {
        "default_5_levels": (dict(), (0.0, 0.0), False),
        "regime_3_2_1": (dict(levels=3, regime=[3, 2, 1]), (0.0, 0.0), False),
        "regime_2_2": (dict(levels=2, regime=[2, 2]), (0.0, 0.0), False),
        "regime_1": (dict(levels=1, regime=[1]), (0.0, 0.0), False),
        "run_till_level_1": (dict(levels=4, run_till_level=1, regime=[3, 3, 3, 1]), (0.0, 0.0), False),
        "early_stop": (dict(levels=3, regime=[3, 3, 3], termination_threshold=2.3e-4), (0.0, 0.0), False),
        "far_start_rejects": (dict(levels=3, regime=[3, 3, 3], termination_threshold=1e-7), (4.1, 0.131), True),
    }


# max |entry| distance of the CPU oracle's tracked pose from the float64 reference's, measured per case (DESIGN.md
# section 7); the limit of either engine is four times that (the HIP engine differs from the oracle only in the
# summation order of the 29 sums, bounded at 1e-6 by tests/test_gpu_tracker.py)
ORACLE_RUN_DISTANCE = {
    "default_5_levels": 5.32e-08,
    "early_stop": 7.97e-08,
    "far_start_rejects": 3.98e-08,
    "regime_1": 2.46e-06,
    "regime_2_2": 1.11e-07,
    "regime_3_2_1": 9.50e-08,
    "run_till_level_1": 2.35e-08,
}
RUN_LIMIT_FACTOR = 4.0


def pose_error(M, M_true):
    """(rotation angle in rad, translation in m) of M relative to M_true."""
    D = np.asarray(M, np.float64) @ np.linalg.inv(np.asarray(M_true, np.float64))
    ang = math.atan2(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0, (np.trace(D[:3, :3]) - 1.0) / 2.0)
    return ang, float(np.linalg.norm(D[:3, 3]))


def assert_rigid(M, what):
    M = np.asarray(M)
    assert np.isfinite(M).all(), f"{what}: pose not finite"
    R = M[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6, f"{what}: rotation not orthonormal"
    assert np.array_equal(M[3], np.array([0, 0, 0, 1], M.dtype)), f"{what}: bottom row {M[3]}"


def _box_setup(api, pkg, W=RUN_W, H=RUN_H):
    return Setup(api, pkg, am.box_corner(num_buckets=0x80), W, H, dict(yaw=0.27, pitch=-0.19, roll=0.1), (1.0, 0.01))


def check_run(api, pkg, case, setup=None):
    """track_camera against ref64_tracker.track.  Returns (distance, figures), or None when the reference flags an
    accept / reject decision as a tie (the case is then reported, not judged)."""
    kw, start_off, needs_reject = run_cases()[case]
    s = setup or _box_setup(api, pkg)
    start = perturbed(s.M_map, *start_off) if start_off != (0.0, 0.0) else s.M_map
    tp = pkg.TrackerParams(**kw)
    M_ref, log = rt.track(s.depth, s.intr, s.points, s.normals, s.M_map, start, levels=tp.no_hierarchy_levels,
                          run_till_level=tp.no_icp_run_till_level, dist_thresh=tp.dist_thresh,
                          termination_threshold=tp.termination_threshold, regime=list(tp.regime))
    seq = "".join("a" if r["accepted"] else "r" for r in log)
    print(f"{case}: reference runs {len(log)} evaluations, {seq}, levels {[r['level'] for r in log]}, "
          f"lambda up to {max(r['lam'] for r in log):g}, last valid {log[-1]['valid']}, last f {log[-1]['f']:.6g}")
    if needs_reject:
        assert "r" in seq and max(r["lam"] for r in log) > 1.0, f"{case}: the reference trajectory has no rejection"
    if case == "early_stop":
        iters, _ = rt.level_schedule(tp.no_hierarchy_levels, tp.dist_thresh)
        per_level = {lv: sum(1 for r in log if r["level"] == lv) for lv in range(tp.no_hierarchy_levels)}
        assert any(per_level[lv] < iters[lv] for lv in per_level), f"{case}: no level stopped early ({per_level})"
    if any(r["accept_tie"] for r in log):
        print(f"{case}: the reference's accept / reject decision is a tie; not judged")
        return None
    pose, res = s.track(start, **kw)
    assert_rigid(pose, case)
    # the ABI reports the number of evaluations and the last one's valid count and error value, not the accept /
    # reject sequence: a different sequence changes them (a rejected step restores the pose, the next evaluation
    # repeats) and the pose
    last = log[-1]
    assert res.iterations == len(log), f"{case}: {res.iterations} evaluations, reference {len(log)} ({seq})"
    assert abs(res.valid_points_last - last["valid"]) <= last["ties"], f"{case}: last valid {res.valid_points_last}, reference {last['valid']}"
    dist = float(np.abs(np.asarray(pose, np.float64) - M_ref).max())
    print(f"{case}: max |pose - reference| {dist:.3g}")
    # f of the last evaluation: the tier-(a) interval, plus what the pose's own distance from the reference's may add.
    # Poses at most L = the run's limit apart per entry move a point p by at most L (|p|_1 + 1) <= L (3 p_max + 1), each
    # residual b = n . (cp - p) by as much (|n| = 1; to first order the correspondence moves along the surface), so
    # |d sqrt(sum b^2)| <= sqrt(valid) L (3 p_max + 1) and |df| <= L (3 p_max + 1) / sqrt(valid)
    f_lo, f_hi = rt.error_interval(last["sum_bb"], last["bound_bb"], last["max_bb"], last["valid"], last["ties"])
    df = RUN_LIMIT_FACTOR * ORACLE_RUN_DISTANCE[case] * (3.0 * last["p_max"] + 1.0) / math.sqrt(last["valid"])
    print(f"{case}: last f {res.f_last:.9g}, reference {last['f']:.9g} in [{f_lo - df:.9g}, {f_hi + df:.9g}]")
    assert f_lo - df <= res.f_last <= f_hi + df, f"{case}: last f {res.f_last:.9g}, reference {last['f']:.9g}"
    return dist, dict(evaluations=len(log), sequence=seq, f_last=res.f_last, f_ref=log[-1]["f"])


def assert_recorded_distance_is_the_oracles(case, dist):
    """CPU only: the recorded figure the limits hang on is still what the oracle gives, within a factor of two either way."""
    rec = ORACLE_RUN_DISTANCE[case]
    assert 0.5 * rec <= dist <= 2.0 * rec, f"{case}: the oracle is {dist:.3g} from the reference, recorded {rec:.3g}"


def assert_run_within_limit(case, dist):
    lim = RUN_LIMIT_FACTOR * ORACLE_RUN_DISTANCE[case]
    assert dist <= lim, f"{case}: pose {dist:.3g} from the float64 reference, limit {lim:.3g}"


# ---------------------------------------------------------------------------------------------------------------------
# tier (b): against the true pose
# ---------------------------------------------------------------------------------------------------------------------
# what the float64 reference reaches on the same input: (rotation rad, translation m) from the true pose (DESIGN.md
# section 7); either engine must stay within twice that
REFERENCE_TRUTH_ERROR = {
    "box_single_level_three_calls": (3.772e-04, 4.216e-04),
    "box_default_5_levels": (1.1244e-03, 2.316e-04),
    "plane_default_5_levels": (3.561e-04, 3.788e-05),  # (tilt rad, distance along the normal m)
}
TRUTH_LIMIT_FACTOR = 2.0


def _ref_track(s, start, tp):
    return rt.track(s.depth, s.intr, s.points, s.normals, s.M_map, start, levels=tp.no_hierarchy_levels,
                    run_till_level=tp.no_icp_run_till_level, dist_thresh=tp.dist_thresh,
                    termination_threshold=tp.termination_threshold, regime=list(tp.regime))[0]


def truth_cases():
    return ["box_single_level_three_calls", "box_default_5_levels", "plane_default_5_levels"]


def check_truth(api, pkg, case, reference_only=False):
    """Returns (engine error, reference error, start error); for the plane the errors are (tilt rad, distance m)."""
    plane = case.startswith("plane")
    if plane:
        s = Setup(api, pkg, am.tilted_plane(num_buckets=0x100), RUN_W, RUN_H, dict(yaw=-0.05, roll=0.1), (1.0, 0.01))
    else:
        s = _box_setup(api, pkg)
    calls = [dict(levels=1, regime=[3])] * 3 if case == "box_single_level_three_calls" else [dict()]

    def err(M):
        if not plane:
            return pose_error(M, s.M_true)
        n, c = s.m.geom.n, s.m.geom.c
        out = []
        for P in (M, s.M_true):
            P = np.asarray(P, np.float64)
            centre = np.linalg.inv(P)[:3, 3]
            out.append((P[:3, :3] @ n, n @ centre - c))
        (n_e, d_e), (n_t, d_t) = out
        return math.atan2(np.linalg.norm(np.cross(n_e, n_t)), n_e @ n_t), abs(d_e - d_t)

    pose, ref = s.M_map, np.asarray(s.M_map, np.float64)
    for kw in calls:
        tp = pkg.TrackerParams(**kw)
        ref = _ref_track(s, ref, tp)
        if not reference_only:
            pose, _ = s.track(pose, **kw)
    e_start, e_ref = err(s.M_map), err(ref)
    print(f"{case}: start {e_start}, float64 reference {e_ref}")
    if reference_only:
        return None, e_ref, e_start
    assert_rigid(pose, case)
    e = err(pose)
    print(f"{case}: engine {e}")
    return e, e_ref, e_start


def assert_truth_within_limit(case, e, e_start):
    lim = [TRUTH_LIMIT_FACTOR * v for v in REFERENCE_TRUTH_ERROR[case]]
    assert e[0] <= lim[0] and e[1] <= lim[1], f"{case}: {e} from the truth, limits {lim}"
    if not case.startswith("plane"):
        assert e[0] < 0.25 * e_start[0] and e[1] < 0.25 * e_start[1], f"{case}: error {e}, start error {e_start}"


# ---------------------------------------------------------------------------------------------------------------------
# away from the world origin.  The law is the reference's and is not changed.
# ---------------------------------------------------------------------------------------------------------------------
PLACED_CASES = ("box_64x48_small_perturbation", "box_70x45_fy_not_fx")
PLACEMENTS = ("near+-+", "near-+-", "far+", "far-", "edge_pos", "edge_neg")
# One evaluation.  The reference's bound propagates with the magnitudes of the coordinates (26 eps |t|_1 for the pose's
# float32 inverse alone), and with the tie windows derived from it (ref64_tracker.evaluate, derived_ties) a projection is a
# tie over ever more of the image: 37 % of the valid pixels at block 1000, all of them from block 4000 on.  The caps are
# placement_fixtures.TIE_CAP's; D is halved until the reference meets the cap on every level and iteration type.  Times
# halved, per case and placement (test_oracle_tracker_placement.py asserts the cap there and that one halving fewer misses
# it, which is also the statement that the unhalved placements cannot be judged):
EVALUATION_HALVINGS = {
    ("box_64x48_small_perturbation", "near+-+"): 6, ("box_64x48_small_perturbation", "near-+-"): 6,
    ("box_64x48_small_perturbation", "far+"): 8, ("box_64x48_small_perturbation", "far-"): 8,
    ("box_64x48_small_perturbation", "edge_pos"): 8, ("box_64x48_small_perturbation", "edge_neg"): 8,
    ("box_70x45_fy_not_fx", "near+-+"): 4, ("box_70x45_fy_not_fx", "near-+-"): 4,
    ("box_70x45_fy_not_fx", "far+"): 6, ("box_70x45_fy_not_fx", "far-"): 6,
    ("box_70x45_fy_not_fx", "edge_pos"): 6, ("box_70x45_fy_not_fx", "edge_neg"): 6,
}


def placed_evaluation(case, pname, fewer=0):
    """(tie cap, D) of a placed single-evaluation case; fewer: that many halvings fewer than recorded."""
    cls, D = pf.placements(evaluation_cases()[case]["map"]().block_pos)[pname]
    return pf.TIE_CAP[cls], pf.halved(D, EVALUATION_HALVINGS[case, pname] - fewer)


def check_placed_evaluations(api, pkg, case, pname):
    """check_evaluations, every level and iteration type, with the case moved to its placement."""
    cap, D = placed_evaluation(case, pname)
    return check_evaluations(api, pkg, case, D=D, tie_cap=cap)


# Whole runs: the default five-level run on the box corner, from the map pose (1 degree and 1 cm from the true one).
PLACED_RUNS = {"origin": None, "block_100": (100, -70, 130), "near+-+": (1000, -700, 1300), "near-+-": (-1000, 700, -1300)}
# what a pose far out may differ by, whatever computed it: the float32 inverse of a pose carries 26 eps per rotation entry
# and 26 eps |t|_1 in its translation (ref64_tracker.inverse_error), and |t|_1 <= 3 P vs, eps P <= u(P): 78 u(P) vs
POSE_U = 78.0


def check_placed_run(api, pkg, name, D=None):
    """The run on the map moved by D (default PLACED_RUNS[name]) blocks against ref64_tracker.track, with derived tie
    windows, on the ICP maps the engine rendered there.  Returns (engine's error, reference's error, start error, u), the
    errors (rotation rad, translation m) from the true pose and u = u(P) vs in metres, or None where the reference flags
    an accept / reject decision as a tie."""
    D = PLACED_RUNS[name] if D is None and name in PLACED_RUNS else D
    s = Setup(api, pkg, am.box_corner(num_buckets=0x80), RUN_W, RUN_H, dict(yaw=0.27, pitch=-0.19, roll=0.1), (1.0, 0.01), D=D)
    tp = pkg.TrackerParams()
    M_ref, log = rt.track(s.depth, s.intr, s.points, s.normals, s.M_map, s.M_map, levels=tp.no_hierarchy_levels,
                          run_till_level=tp.no_icp_run_till_level, dist_thresh=tp.dist_thresh,
                          termination_threshold=tp.termination_threshold, regime=list(tp.regime), derived_ties=D is not None)
    e_start, e_ref = pose_error(s.M_map, s.M_true), pose_error(M_ref, s.M_true)
    u = pf.u(pf.P(s.m)) * s.m.vs
    print(f"{name}: reference runs {len(log)} evaluations on levels {[r['level'] for r in log]}; start {e_start}, reference {e_ref}")
    if any(r["accept_tie"] for r in log):
        print(f"{name}: the reference's accept / reject decision is a tie; not judged")
        return None
    pose, res = s.track(s.M_map)
    assert_rigid(pose, name)
    e = pose_error(pose, s.M_true)
    last = log[-1]
    print(f"{name}: engine {res.iterations} evaluations, {e}; last valid {res.valid_points_last}, reference {last['valid']} "
          f"with {last['ties']} ties")
    assert res.iterations == len(log), f"{name}: {res.iterations} evaluations, reference {len(log)}"
    assert abs(res.valid_points_last - last["valid"]) <= last["ties"], f"{name}: last valid {res.valid_points_last}, reference {last['valid']}"
    return e, e_ref, e_start, u


def assert_placed_run(name, e, e_ref, e_start, u):
    """Tier (b)'s rule with what the coordinates' size adds: an engine's error to the truth is within the larger of the
    origin's limit (TRUTH_LIMIT_FACTOR x the reference's error at the origin) and the reference's error on the same input
    plus POSE_U u(P) (translation, metres) or 3 x 26 eps (rotation, the three entries of a row of the inverse)."""
    lim = [TRUTH_LIMIT_FACTOR * v for v in REFERENCE_TRUTH_ERROR["box_default_5_levels"]]
    assert e[0] <= max(lim[0], e_ref[0] + 78.0 * rt.EPS), f"{name}: rotation {e[0]} from the truth, reference {e_ref[0]}"
    assert e[1] <= max(lim[1], e_ref[1] + POSE_U * u), f"{name}: translation {e[1]} from the truth, reference {e_ref[1]}"
    if PLACED_RUNS[name] is None:
        assert e_ref[0] < 0.25 * e_start[0] and e_ref[1] < 0.25 * e_start[1]
