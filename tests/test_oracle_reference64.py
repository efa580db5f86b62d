"""The float64 references of ref64.py against the CPU oracle (check bodies in ref64_checks.py, shared with
test_gpu_reference64.py).  This validates the references on any machine and is the oracle's first check that does
not go through its own float32 arithmetic."""
import pytest

import analytic_maps as am
import ref64_checks as rc


@pytest.mark.parametrize("case", rc.INTEGRATION_CASES)
def test_integration_step_against_float64(pkg, synth, oracle, case):
    n_upd, n_tie, n_tie_aligned = rc.run_integration_case(oracle, pkg, synth, case)
    print(f"{case}: {n_upd} updated voxels, {n_tie} ties (+{n_tie_aligned} on axis-aligned poses)")


@pytest.mark.parametrize("W,H", [(70, 45), (1226, 370)])
def test_bilateral_filter_against_float64(oracle, W, H):
    print(f"worst relative error {rc.check_view_filter(oracle, W, H, rel_tol=1e-5):.3g}")


@pytest.mark.parametrize("case", sorted(rc.raycast_cases()))
def test_raycast_against_float64_and_geometry(pkg, oracle, case):
    figures, max_chain = rc.run_raycast_case(oracle, pkg, case)
    print(f"{case} (longest chain {max_chain}): {figures}")


@pytest.mark.parametrize("case", sorted(rc.mesh_cases()))
def test_mesh_against_float64_and_geometry(pkg, oracle, case):
    print(f"{case}: {rc.run_mesh_case(oracle, pkg, case)}")


def test_analytic_maps_exercise_the_hash():
    """The maps reach excess chains of length >= 3, negative block coordinates and, with holes, missing blocks."""
    m = am.tilted_plane(num_buckets=0x40)
    assert m.max_chain >= 3 and (m.block_pos < 0).any()
    assert (m.hash["ptr"][m.num_buckets:] >= 0).sum() > len(m.block_pos) // 2
    full, holed = am.tilted_plane(tilt_deg=35.0), am.tilted_plane(tilt_deg=35.0, holes=0.1, seed=5)
    assert len(holed.block_pos) < 0.95 * len(full.block_pos)
