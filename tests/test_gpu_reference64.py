"""The HIP kernels against the float64 references of ref64.py (check bodies in ref64_checks.py, shared with
test_oracle_reference64.py): integration step by step, the bilateral filter, raycast / ICP maps / colour on exact
analytic maps, and the mesh -- none of it compared with the CPU oracle."""
import pytest

pytestmark = pytest.mark.gpu

import ref64_checks as rc


@pytest.mark.parametrize("case", rc.INTEGRATION_CASES)
def test_integration_step_against_float64(pkg, synth, gpu, case):
    n_upd, n_tie, n_tie_aligned = rc.run_integration_case(gpu, pkg, synth, case)
    print(f"{case}: {n_upd} updated voxels, {n_tie} ties (+{n_tie_aligned} on axis-aligned poses)")


@pytest.mark.parametrize("W,H", [(70, 45), (1226, 370)])
def test_bilateral_filter_against_float64(gpu, W, H):
    print(f"worst relative error {rc.check_view_filter(gpu, W, H, rel_tol=1e-5):.3g}")


@pytest.mark.parametrize("case", sorted(rc.raycast_cases()))
def test_raycast_against_float64_and_geometry(pkg, gpu, case):
    figures, max_chain = rc.run_raycast_case(gpu, pkg, case)
    print(f"{case} (longest chain {max_chain}): {figures}")


@pytest.mark.parametrize("case", sorted(rc.mesh_cases()))
def test_mesh_against_float64_and_geometry(pkg, gpu, case):
    print(f"{case}: {rc.run_mesh_case(gpu, pkg, case)}")

