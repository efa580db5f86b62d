"""The float64 references and the map model against the CPU oracle on fixtures moved far from the world origin (check
bodies in placement_checks.py, shared with test_gpu_placement.py).  This validates the scaled bounds
on any machine, before the HIP engine meets them."""
import pytest

import placement_checks as pc
import refvoxel_checks as rv


@pytest.mark.parametrize("pname", pc.PLACEMENTS)
@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_raycast_far_from_the_origin(pkg, oracle, case, pname):
    print(f"{case} at {pname}: {pc.run_raycast(oracle, pkg, case, pname)}")


@pytest.mark.parametrize("pname", pc.UNTIED_PLACEMENTS)
@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_raycast_at_the_full_distance(pkg, oracle, case, pname):
    print(f"{case} at {pname}: {pc.run_raycast_full(oracle, pkg, case, pname)}")


@pytest.mark.parametrize("pname", pc.PLACEMENTS)
@pytest.mark.parametrize("case", pc.MESH_CASES)
def test_mesh_far_from_the_origin(pkg, oracle, case, pname):
    print(f"{case} at {pname}: {pc.run_mesh(oracle, pkg, case, pname)}")


@pytest.mark.parametrize("pname", ["near+-+", "far-", "edge_pos", "edge_neg"])
def test_visible_list_and_range_image_far_from_the_origin(pkg, oracle, pname):
    print(f"{pname}: {pc.run_range(oracle, pkg, pname)}")


@pytest.mark.parametrize("pname", pc.HEAVY)
@pytest.mark.parametrize("case", pc.update_cases(), ids=rv.case_id)
def test_voxel_update_far_from_the_origin(pkg, oracle, case, pname):
    out = pc.run_update(oracle, pkg, *case, pname)
    print(f"{rv.case_id(case)} at {pname}: D {out['D']}, blocks {out['lo']} .. {out['hi']}, {out['values']}")


@pytest.mark.parametrize("pname", pc.HEAVY)
def test_reintegration_batch_far_from_the_origin(pkg, oracle, pname):
    print(f"{pname}: {pc.run_update_batch(oracle, pkg, 'depth_shard', 100, rv.MU_STEPS[1], 3, pname)}")


@pytest.mark.parametrize("pname", pc.HEAVY)
def test_allocation_far_from_the_origin(pkg, synth, oracle, pname):
    print(f"{pname}: {pc.run_allocation(oracle, pkg, synth, pname)}")
