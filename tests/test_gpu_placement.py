"""The HIP kernels far from the world origin (check bodies in placement_checks.py, shared with test_oracle_placement.py;
DESIGN section 27): the reads of one map against the float64 references and the range law, the voxel update against
ref64.update_exact in every kernel form, the allocation pass against the map model -- none of it compared with the CPU
oracle -- and then parity with the oracle, bit for bit, on sequences fused out there."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import placement_checks as pc
import placement_fixtures as pf
import refvoxel_checks as rv
import scenarios
from util import assert_same_mesh as _same_mesh


@pytest.mark.parametrize("pname", pc.PLACEMENTS)
@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_raycast_far_from_the_origin(pkg, gpu, case, pname):
    print(f"{case} at {pname}: {pc.run_raycast(gpu, pkg, case, pname)}")


@pytest.mark.parametrize("pname", pc.FULL_D_PLACEMENTS)
@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_raycast_equals_the_oracle_at_the_full_distance(pkg, gpu, oracle, case, pname):
    """Ray for ray, ties and all: the hit masks are equal and every product of the march is the oracle's, bit for bit."""
    g, o = (pc.run_raycast_images(api, pkg, case, pname) for api in (gpu, oracle))
    assert (o["depth"] > 0).sum() > 1000
    diff = {k: (bool(np.array_equal(g[k], o[k])), float(np.abs(g[k].astype(np.float64) - o[k]).max())) for k in o if k != "teeth"}
    print(f"{case} at {pname}: (equal, largest difference) {diff}")
    assert np.array_equal(g["depth"] > 0, o["depth"] > 0), "hit masks differ"
    for k, (same, d) in diff.items():
        assert same, f"{k} differs from the oracle's by up to {d:.3g}"


@pytest.mark.parametrize("pname", pc.UNTIED_PLACEMENTS)
@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_raycast_at_the_full_distance(pkg, gpu, case, pname):
    print(f"{case} at {pname}: {pc.run_raycast_full(gpu, pkg, case, pname)}")


@pytest.mark.parametrize("pname", pc.PLACEMENTS)
@pytest.mark.parametrize("case", pc.MESH_CASES)
def test_mesh_far_from_the_origin(pkg, gpu, case, pname):
    print(f"{case} at {pname}: {pc.run_mesh(gpu, pkg, case, pname)}")


@pytest.mark.parametrize("pname", ["near+-+", "far-", "edge_pos", "edge_neg"])
def test_visible_list_and_range_image_far_from_the_origin(pkg, gpu, pname):
    print(f"{pname}: {pc.run_range(gpu, pkg, pname)}")


@pytest.mark.parametrize("pname", pc.HEAVY)
@pytest.mark.parametrize("case", pc.update_cases(), ids=rv.case_id)
def test_voxel_update_far_from_the_origin(pkg, gpu, case, pname):
    out = pc.run_update(gpu, pkg, *case, pname)
    print(f"{rv.case_id(case)} at {pname}: D {out['D']}, blocks {out['lo']} .. {out['hi']}, {out['values']}")


@pytest.mark.parametrize("pname", pc.HEAVY)
def test_reintegration_batch_far_from_the_origin(pkg, gpu, pname):
    print(f"{pname}: {pc.run_update_batch(gpu, pkg, 'depth_shard', 100, rv.MU_STEPS[1], 3, pname)}")


@pytest.mark.parametrize("pname", pc.HEAVY)
def test_allocation_far_from_the_origin(pkg, synth, gpu, pname):
    print(f"{pname}: {pc.run_allocation(gpu, pkg, synth, pname)}")


@pytest.mark.parametrize("pname", pc.PARITY_PLACEMENTS)
def test_sequence_and_mesh_equal_the_oracle_far_from_the_origin(pkg, synth, gpu, oracle, pname):
    (sg, mg, ext), (so, mo, _) = (pc.run_parity_sequence(api, pkg, synth, pname) for api in (gpu, oracle))
    scenarios.assert_same_full_state(sg, so, f"decay + slide at {pname}")
    assert len(mo[0]) > 1000
    _same_mesh(mg, mo, f"mesh at {pname}")
    print(f"{pname}: D {pc.parity_D('sequence', pname)[1]}, blocks held {ext[0]} .. {ext[1]}, {len(mo[0])} triangles")
    if pname == "edge_neg":
        assert (ext[0] == pf.FIRST_BLOCK).all(), f"the smallest block held was {ext[0]}"
    else:
        assert (np.minimum(np.abs(ext[0]), np.abs(ext[1])) >= 256).all()


@pytest.mark.parametrize("call", ["batch", "loop"])
@pytest.mark.parametrize("pname", pc.PARITY_PLACEMENTS)
def test_reintegration_equals_the_oracle_far_from_the_origin(pkg, synth, gpu, oracle, pname, call):
    g, o = (pc.run_parity_batch(api, pkg, synth, pname, call) for api in (gpu, oracle))
    for k in ("first", "second"):
        scenarios.assert_same_full_state(g[k], o[k], f"{call} at {pname}: {k}")
    (gt, gc), (ot, oc) = g["alloc_scratch"], o["alloc_scratch"]
    assert np.array_equal(gt, ot), "allocType of the last pass"
    assert np.array_equal(gc[ot > 0], oc[ot > 0]), "blockCoords of the last pass"
    pos = o["second"]["hash"]["pos"][o["second"]["hash"]["ptr"] >= 0]
    assert len(pos) > 300 and pos.min() >= pf.FIRST_BLOCK and pos.max() <= pf.LAST_BLOCK
