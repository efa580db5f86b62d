"""The float64 tracker reference of ref64_tracker.py against the CPU oracle (check bodies in
ref64_tracker_checks.py, shared with test_gpu_tracker64.py), and the reference's own self-checks, which do not depend
on upstream recall: the Jacobian row against finite differences of ApplyDelta, and accepted steps never raising f."""
import numpy as np
import pytest

import analytic_maps as am
import ref64_tracker as rt
import ref64_tracker_checks as tc


@pytest.mark.parametrize("case", sorted(tc.evaluation_cases()))
def test_one_evaluation_against_float64(pkg, oracle, case):
    print(f"{case}: {tc.check_evaluations(oracle, pkg, case)}")


@pytest.fixture(scope="module")
def box(pkg, oracle):
    return tc._box_setup(oracle, pkg)


def test_whole_runs_against_float64(pkg, oracle, box):
    """Every run case; at most one may end on an accept / reject tie of the reference."""
    skipped = []
    for case in sorted(tc.run_cases()):
        out = tc.check_run(oracle, pkg, case, box)
        if out is None:
            skipped.append(case)
            continue
        # the oracle's own distance is what the recorded figure was measured as: it must not have drifted past its limit
        tc.assert_run_within_limit(case, out[0])
        tc.assert_recorded_distance_is_the_oracles(case, out[0])
    assert len(skipped) <= 1, f"accept ties in {skipped}"


@pytest.mark.parametrize("case", tc.truth_cases())
def test_tracked_pose_against_the_truth(pkg, oracle, case):
    e, e_ref, e_start = tc.check_truth(oracle, pkg, case)
    tc.assert_truth_within_limit(case, e, e_start)


def test_recorded_reference_errors_are_the_references(pkg, oracle):
    """The limits of tier (b) are twice what the float64 reference reaches: the recorded figures must be its own."""
    for case in tc.truth_cases():
        _, e_ref, _ = tc.check_truth(oracle, pkg, case, reference_only=True)
        assert np.allclose(e_ref, tc.REFERENCE_TRUTH_ERROR[case], rtol=0.02, atol=1e-9), (case, e_ref)


def test_icp_sums_need_an_evaluation(pkg):
    import __graft_entry__ as ge
    fresh = ge.load_oracle().open_oracle(pkg.CApi)
    with pytest.raises(pkg.DslamError):
        fresh.debug_icp_sums()


# ---- self-checks of the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("type", [rt.ROTATION, rt.TRANSLATION, rt.BOTH])
def test_jacobian_row_matches_apply_delta(type):
    """With the correspondences (cp, n) held fixed, moving the pose by ApplyDelta(delta) changes every residual to
    b - A . delta up to second order: pins the signs and the order of A against Tinc."""
    rng = np.random.default_rng(7)
    n_pts = 200
    p = rng.normal(size=(n_pts, 3)) * 0.4 + np.array([0.1, -0.2, 0.9])
    nrm = rng.normal(size=(n_pts, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cp = p + rng.normal(size=(n_pts, 3)) * 0.01
    b = np.sum(nrm * (cp - p), -1)
    r = np.stack([p[:, 2] * nrm[:, 1] - p[:, 1] * nrm[:, 2], -p[:, 2] * nrm[:, 0] + p[:, 0] * nrm[:, 2],
                  p[:, 1] * nrm[:, 0] - p[:, 0] * nrm[:, 1]], -1)
    A = r if type == rt.ROTATION else nrm if type == rt.TRANSLATION else np.concatenate([r, nrm], -1)
    npara = A.shape[1]
    for k in range(npara):
        for h in (1e-3, 1e-4):
            delta = np.zeros(npara)
            delta[k] = h
            T = rt.tinc(delta, type)  # the new approxInvPose maps the same camera point to T p
            p2 = p @ T[:3, :3].T + T[:3, 3]
            b2 = np.sum(nrm * (cp - p2), -1)
            assert np.abs((b2 - b) / h + A[:, k]).max() <= 1e-9 + 2.0 * h, (type, k)


def test_reference_evaluate_uses_the_same_row(pkg, oracle):
    """evaluate's A and b are the ones the finite-difference check pins (same formulas on its own p, n, cp)."""
    s = tc.Setup(oracle, pkg, am.box_corner(num_buckets=0x80), 64, 48, dict(yaw=0.2, pitch=0.15), (0.5, 0.005))
    inv = np.linalg.inv(np.asarray(s.M_map, np.float64))
    ev = rt.evaluate(s.depth, s.intr, s.points, s.normals, s.intr, inv, s.M_map, 0.01, rt.BOTH)
    p, n, cp = ev["p"], ev["n"], ev["cp"]
    assert len(p) > 500
    assert np.allclose(ev["b"], np.sum(n * (cp - p), -1), atol=1e-15)
    assert np.allclose(ev["A"][:, :3], -np.cross(p, n), atol=1e-15) and np.array_equal(ev["A"][:, 3:], n)
    # a small step along the solved direction lowers sum b^2 as the linear model says
    Hm, g = rt._full(ev["sums"], 6)
    step = np.linalg.solve(Hm, g) * 1e-2
    _, inv2 = rt.apply_step(inv, step, rt.BOTH)
    ev2 = rt.evaluate(s.depth, s.intr, s.points, s.normals, s.intr, inv2, s.M_map, 0.01, rt.BOTH)
    assert ev2["sums"][27] / ev2["sums"][28] < ev["sums"][27] / ev["sums"][28]


def test_accepted_steps_never_increase_f(pkg, oracle, box):
    for case in sorted(tc.run_cases()):
        kw, start_off, _ = tc.run_cases()[case]
        tp = pkg.TrackerParams(**kw)
        start = tc.perturbed(box.M_map, *start_off) if start_off != (0.0, 0.0) else box.M_map
        _, log = rt.track(box.depth, box.intr, box.points, box.normals, box.M_map, start, levels=tp.no_hierarchy_levels,
                          run_till_level=tp.no_icp_run_till_level, dist_thresh=tp.dist_thresh,
                          termination_threshold=tp.termination_threshold, regime=list(tp.regime))
        for level in {r["level"] for r in log}:
            f = [r["f"] for r in log if r["level"] == level and r["accepted"]]
            assert all(b <= a for a, b in zip(f, f[1:])), (case, level, f)


def test_subsample_with_holes_odd_sizes():
    d = np.arange(1, 5 * 7 + 1, dtype=np.float32).reshape(5, 7)
    d[0, 0] = 0.0
    d[1, 1] = -1.0
    d[2:4, 2:4] = 0.0
    o64, o32 = rt.subsample_with_holes(d)
    assert o64.shape == (2, 3) and o32.dtype == np.float32
    assert o64[0, 0] == (2.0 + 8.0) / 2 and o64[1, 1] == 0.0 and o64[0, 2] == (5 + 6 + 12 + 13) / 4.0
    assert np.array_equal(o64, o32)
