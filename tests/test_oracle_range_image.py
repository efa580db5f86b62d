"""The visible list and the range image on the CPU oracle against the law of ref_range.py (check bodies in
refrange_checks.py, shared with test_gpu_range_image.py).  The reference-only tests come first: every fixture reaches
what it is there for and stays inside the tie cap before any engine is in the loop, the law reduces to
ref64.expected_depths where that one is defined, and the tie counter is alive."""
import numpy as np
import pytest

import analytic_maps as am
import range_fixtures as rf
import ref64
import ref64_checks as rc
import ref_range as rr
import refrange_checks as chk

CASES = sorted(rf.ALL_CASES)
BUDGETS = [(w, k) for w in ("close", "shell") for k in rf.BUDGET_KINDS]


@pytest.mark.parametrize("name", CASES)
def test_fixtures_reach_their_paths_from_the_reference_alone(name):
    c = rf.ALL_CASES[name]()          # (the fixture asserts its reach and the tie cap as it is built)
    for pose, r in (("first", c.ref), ("second", c.ref_other)):
        blocks, cells = r.tie_shares()
        print(f"{name}, {pose} pose: {len(r.ids)} listed, {int((r.req != 0).sum())} with tiles, total {r.total}, "
              f"{int((r.tile_cells() > rf.BIG_BOX).sum())} boxes above {rf.BIG_BOX} cells of a tile, "
              f"tie blocks {r.n_tie_blocks} ({blocks:.2%}), tie cells {cells:.2%}")
        assert blocks <= rf.TIE_BLOCKS and cells <= rf.TIE_CELLS


@pytest.mark.parametrize("which,kind", BUDGETS)
def test_budget_fixtures_bite_from_the_reference_alone(which, kind):
    c, b, r = rf.budget(which, kind)
    live = r.req != 0
    print(f"{which}, budget {kind} = {b}: total {r.total}, {int((~r.accepted & live).sum())} of {int(live.sum())} dropped")


def test_budget_rule_by_hand():
    # 3 + 4 = 7 < 9; 7 + 5 >= 9 dropped and not counted; 7 + 1 = 8 < 9; 8 + 1 >= 9 dropped; a req of 0 is never kept
    keep, total = rr.apply_budget([3, 4, 0, 5, 1, 1], 9)
    assert total == 14 and keep.tolist() == [True, True, False, False, True, False]
    keep, total = rr.apply_budget([3, 4, 0, 5, 1, 1], 15)   # total < budget: the rule is off
    assert keep.tolist() == [True, True, False, True, True, True]
    keep, total = rr.apply_budget([3, 4, 0, 5, 1, 1], 14)   # total == budget: on, and only the last entry reaches it
    assert keep.tolist() == [True, True, False, True, True, False]


def test_projection_of_one_block_by_hand():
    """A block straight ahead of an identity camera, numbers a reader can follow: vs = 1/256, so a block edge is 1/32 m."""
    W, H, intr = 64, 48, (64.0, 64.0, 32.0, 24.0)
    M = np.eye(4, dtype=np.float32)
    p = rr.project_blocks([[2, -1, 32]], M, intr, 1.0 / 256.0, W, H)
    # corners x in {2, 3}/32, y in {-1, 0}/32, z in {32, 33}/32: u = 64 x / z + 32 in {35.88, 36, 37.82, 38}, v in {22, 22.06, 24}
    assert p["box"].tolist() == [[4, 2, 5, 3]] and p["req"].tolist() == [1]
    assert p["z"].tolist() == [[1.0, 33.0 / 32.0]]
    # the same block behind the camera: every corner skipped, the start values make an empty box
    q = rr.project_blocks([[2, -1, -40]], M, intr, 1.0 / 256.0, W, H)
    assert q["skipped"].all() and q["req"].tolist() == [0] and q["box"].tolist() == [[8, 6, -1, -1]]


@pytest.mark.parametrize("make,pose", [(am.sphere_outside, dict(yaw=0.1, pitch=-0.05)), (am.tilted_plane, dict(roll=0.2)),
                                       (am.box_corner, dict(yaw=-0.15, pitch=0.1, roll=0.4))])
def test_law_reduces_to_ref64_expected_depths(make, pose):
    """With an unlimited budget and off the ties the cells agree with ref64.expected_depths, which cast_rays marches by:
    the same cells covered, and z within the float32 rounding of the mat-vec row that made it,
    4 * 2^-24 * (|m20 x| + |m21 y| + |m22 z| + |m23|), the largest over the corners of the blocks that cover the cell."""
    W, H = 77, 52
    m = make()
    M, _ = rc.camera(W, H, **pose)
    intr = (57.3, 58.1, 37.6, 25.3)
    r = rr.RangeLaw(m.hash, M, intr, m.vs, W, H, budget=2 ** 62)
    old = ref64.expected_depths(m, M, intr, W, H)
    assert old.shape == r.image.shape
    ok = ~r.tie_cells
    assert ok.mean() >= 0.95 and len(r.ids) > 50
    covered = r.image[..., 0] != rr.FAR_AWAY
    assert np.array_equal(covered[ok], (old[..., 0] != float(rr.FAR_AWAY))[ok])
    M64 = np.asarray(M, np.float64)
    bound = np.zeros(len(r.ids))
    for corner in range(8):
        p = (r.pos + np.array([corner & 1, (corner >> 1) & 1, (corner >> 2) & 1])) * (8 * float(np.float32(m.vs)))
        bound = np.maximum(bound, 4 * 2.0 ** -24 * (np.abs(M64[2, :3] * p).sum(1) + abs(M64[2, 3])))
    a = r.accepted
    cell_bound = rr.splat(r.box[a], bound[a], bound[a], r.cw, r.ch, 0.0, 0.0)[..., 1]
    sel = ok & covered
    err = np.abs(r.image.astype(np.float64) - old)
    raised = r.image[..., 0] == rr.VERY_CLOSE      # (zmin raised to VERY_CLOSE: float32(0.05) on one side, 0.05 as double on the other)
    print(f"{make.__name__}: {int(sel.sum())} cells, worst |dz| / bound {np.max(err[sel].max(-1) / cell_bound[sel]):.3f}")
    assert sel.sum() > 20 and not raised[sel].any()
    assert (err[sel] <= cell_bound[sel][:, None]).all()


def test_tie_counter_is_alive():
    """A principal point nudged so that one corner lands 1e-8 of a cell off a cell border: float32 cannot place it, and
    over forty such nudges some land on the other side of the border -- flagged, with the block's cells in tie_cells."""
    c = rf.shell(200, 136)
    fx, fy, cx, cy = (float(v) for v in c.intr)
    M64 = np.asarray(c.M, np.float64)
    flagged = 0
    for k in range(40):
        b = c.ref.pos[k]
        q = M64[:3, :3] @ (b * (8 * float(np.float32(c.m.vs)))) + M64[:3, 3]
        px = (fx * q[0] / q[2] + cx) / 8
        nudged = np.float32(cx + 8 * (np.round(px) - px) + 8e-8)
        r = rr.RangeLaw(c.table, c.M, (fx, fy, nudged, cy), c.m.vs, c.W, c.H)
        i = np.nonzero((r.pos == b).all(1))[0]
        if len(i) and r.proj_tie[i[0]]:
            flagged += 1
            assert r.tie_cells[np.clip(r.box[i[0], 1], 0, r.ch - 1), np.clip(r.box[i[0], 0], 0, r.cw - 1)]
    print(f"{flagged} of 40 nudged corners flagged")
    assert flagged >= 3


@pytest.mark.parametrize("name", CASES)
def test_separate_calls(pkg, oracle, name):
    chk.check_separate_calls(oracle, pkg, rf.ALL_CASES[name]())


@pytest.mark.parametrize("name", CASES)
def test_get_image(pkg, oracle, name):
    chk.check_get_image(oracle, pkg, rf.ALL_CASES[name]())


@pytest.mark.parametrize("which,kind", BUDGETS)
def test_budget(pkg, oracle, which, kind):
    chk.check_budget(oracle, pkg, which, kind)


def test_fused(pkg, synth, oracle):
    chk.check_fused(oracle, pkg, synth)
