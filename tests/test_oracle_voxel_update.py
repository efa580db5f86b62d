"""The CPU oracle's voxel update and de-integration (A.11) on crafted voxels and measurements, every stored
value against ref64.update_exact (refvoxel_checks.py; DESIGN 4c has the bands, the reach and the mutant table)."""
import numpy as np
import pytest

import analytic_maps as am
import ref64
import refvoxel_checks as rv


@pytest.mark.parametrize("case", rv.cases(), ids=rv.case_id)
def test_crafted_update(pkg, oracle, case):
    fig = rv.run_case(oracle, pkg, *case)
    print(rv.case_id(case), fig)


@pytest.mark.parametrize("case", rv.batch_cases(), ids=lambda c: "-".join(map(str, c)))
def test_batch_loop_step_by_step(pkg, oracle, case):
    """The per-keyframe loop over stored lists, every step against update_exact (the oracle's batch call is that loop)."""
    b, h, fig = rv.run_batch(oracle, pkg, *case)
    assert b.conditions(h) == dict(stop=0, swapping=0, depth_weights="depth" in case[0], sharded="shard" in case[0])
    print(case, fig)


def test_reference_on_values_known_without_it():
    """update_exact against answers that need no derivation: one voxel per row, one pixel-sized measurement each."""
    depth = np.full((rv.H_IMG, rv.W_IMG), 52 * rv.VS, np.float32)       # a plane at 52 voxels; the voxel (0, 0, z) is on the axis
    rgba = np.full((rv.H_IMG, rv.W_IMG, 4), 200, np.uint8)
    M = np.eye(4, dtype=np.float32)
    intr = np.array([16.0, 16.0, 30.0, 23.0], np.float32)
    pos = np.array([[0, 0, 6]])                                          # voxels z = 48 .. 55: eta = 4 .. -3 voxels
    v = np.zeros((1, 512), am.VOXEL_DTYPE)
    v["sdf"], v["w_depth"], v["clr"], v["w_color"] = 32767, 1, 100, 1
    at = lambda z: z * 64                                                # voxel (0, 0, z) of the block
    lo, hi, info = ref64.update_exact(v, pos, depth, rgba, M, intr, rv.VS, 4 * rv.VS, 100)
    assert info["f"][0, at(0)] == 1 and (lo[0, at(0)]["sdf"], hi[0, at(0)]["sdf"]) == (32766, 32767)  # (1 + 1) / 2: an integer, a tie
    assert info["f"][0, at(4)] == 0 and lo[0, at(4)]["sdf"] == hi[0, at(4)]["sdf"] == 16383         # 32767 / 2 truncated
    assert lo[0, at(4)]["w_depth"] == 2 and lo[0, at(4)]["w_color"] == 2
    assert info["upd_colour"][0, at(4)] and info["upd_colour"][0, at(3)] and not info["upd_colour"][0, at(2)]  # |eta| <= mu / 4
    assert (hi[0, at(4)]["clr"] == 150).all() and (lo[0, at(4)]["clr"] >= 149).all()                # (100 + 200) / 2
    lo, hi, info = ref64.update_exact(v, pos, depth, rgba, M, intr, rv.VS, 4 * rv.VS, 100, deintegrate=True)
    assert lo[0, at(4)]["w_depth"] == 0 and lo[0, at(4)]["sdf"] == hi[0, at(4)]["sdf"] == 32767      # W == w: the empty voxel
    assert lo[0, at(4)]["w_color"] == 0 and (hi[0, at(4)]["clr"] == 0).all()
    v["w_depth"], v["sdf"] = 2, 30000
    lo, hi, info = ref64.update_exact(v, pos, depth, rgba, M, intr, rv.VS, 4 * rv.VS, 100, deintegrate=True, stop_at_max=True)
    assert lo[0, at(4)]["sdf"] == hi[0, at(4)]["sdf"] == 32767 and lo[0, at(4)]["w_depth"] == 1      # 2 * 30000 - 0 clamps
    assert (lo[0, at(0)]["sdf"], hi[0, at(0)]["sdf"]) == (27232, 27233)                              # 60000 - 32767: an integer, a tie
    v["w_depth"] = 0
    lo, hi, info = ref64.update_exact(v, pos, depth, rgba, M, intr, rv.VS, 4 * rv.VS, 100, deintegrate=True)
    assert lo[0, at(4)]["w_depth"] == 0 and lo[0, at(4)]["sdf"] == 30000 and lo[0, at(4)]["w_color"] == 0  # W < w: colour alone
