"""The depth tracker (dslam_track_camera) of the CPU oracle away from the world origin, against the float64 reference on
the ICP maps rendered there (ref64_tracker_checks.py): one evaluation at the six placements, halved
until the reference can judge them, and whole runs near the origin."""
import pytest

import ref64_tracker_checks as tc

PLACED = [(c, p) for c in tc.PLACED_CASES for p in tc.PLACEMENTS]


@pytest.mark.parametrize("case,pname", PLACED)
def test_one_evaluation_away_from_the_origin(pkg, oracle, case, pname):
    out = tc.check_placed_evaluations(oracle, pkg, case, pname)
    cap, D = tc.placed_evaluation(case, pname)
    # one halving fewer, and the reference alone calls too many pixels ties to judge an engine there
    _, D_before = tc.placed_evaluation(case, pname, fewer=1)
    before = tc.check_evaluations(oracle, pkg, case, D=D_before, tie_cap=1.0)["tie_share"]
    print(f"{case} at {pname} {D}: tie share {out['tie_share']:.4f} (cap {cap}), at {D_before}: {before:.4f}; worst share of "
          f"the bound {out['worst_ratio']:.3g}")
    assert out["tie_share"] <= cap < before


@pytest.mark.parametrize("name", sorted(tc.PLACED_RUNS))
def test_whole_run_away_from_the_origin(pkg, oracle, name):
    out = tc.check_placed_run(oracle, pkg, name)
    assert out is not None, f"{name}: the reference calls a decision a tie, so the case judges nothing"
    tc.assert_placed_run(name, *out)
