"""The HIP depth tracker (csrc/track.hip) against the float64 reference of ref64_tracker.py (check bodies in
ref64_tracker_checks.py, shared with test_oracle_tracker64.py): the 29 sums of single evaluations within a derived
float32 rounding bound, whole runs, and the tracked pose against the true one -- none of it compared with the CPU
oracle."""
import pytest

pytestmark = pytest.mark.gpu

import ref64_tracker_checks as tc


@pytest.mark.parametrize("case", sorted(tc.evaluation_cases()))
def test_one_evaluation_against_float64(pkg, gpu, case):
    print(f"{case}: {tc.check_evaluations(gpu, pkg, case)}")


def test_whole_runs_against_float64(pkg, gpu):
    """Every run case; at most one may end on an accept / reject tie of the reference."""
    box = tc._box_setup(gpu, pkg)
    skipped = []
    for case in sorted(tc.run_cases()):
        out = tc.check_run(gpu, pkg, case, box)
        if out is None:
            skipped.append(case)
            continue
        tc.assert_run_within_limit(case, out[0])
    assert len(skipped) <= 1, f"accept ties in {skipped}"


@pytest.mark.parametrize("case", tc.truth_cases())
def test_tracked_pose_against_the_truth(pkg, gpu, case):
    e, e_ref, e_start = tc.check_truth(gpu, pkg, case)
    tc.assert_truth_within_limit(case, e, e_start)


@pytest.mark.parametrize("pname", tc.PLACEMENTS)
@pytest.mark.parametrize("case", tc.PLACED_CASES)
def test_one_evaluation_away_from_the_origin(pkg, gpu, case, pname):
    """the 29 sums on maps moved by whole blocks, as far out as the reference can judge them."""
    print(f"{case} at {pname}: {tc.check_placed_evaluations(gpu, pkg, case, pname)}")


@pytest.mark.parametrize("name", sorted(tc.PLACED_RUNS))
def test_whole_run_away_from_the_origin(pkg, gpu, name):
    """the engine runs the float64 reference's iteration on maps moved by whole blocks and ends as
    close to the truth as the reference does."""
    out = tc.check_placed_run(gpu, pkg, name)
    assert out is not None, f"{name}: the reference calls a decision a tie, so the case judges nothing"
    tc.assert_placed_run(name, *out)


def test_icp_sums_need_an_evaluation(pkg, gpu):
    fresh = pkg.open_engine(0)  # `gpu` has tracked by now or will; a new engine has not
    with pytest.raises(pkg.DslamError):
        fresh.debug_icp_sums()
