"""The placement fixtures and the scaled references on their own, without an engine: a moved map is
the map at the origin; no fusion fixture asks for a block beyond -32768 .. 32766 (from the depth images); the rays the
float64 march calls ties stay under the caps at the D each case records, and one halving fewer misses them; the float32
restatement of the march stays within half of C_RAY; a bound at the origin is the origin's bound."""
import numpy as np
import pytest

import analytic_maps as am
import placement_checks as pc
import placement_fixtures as pf
import ref32_march
import ref64
import ref64_checks as rc
import refvoxel_checks as rv


def test_scale_is_the_origin_up_to_256_voxels():
    for P in (0, 100, 208, 256):
        s = ref64.Scale(P)
        assert s.u == 0.0 and s(1e-3, rc.C_RAY) == 1e-3 and s(1e-4, rc.C_TIE) == 1e-4 and s(0.0, rc.C_MESH) == 0.0
    for case in rc.raycast_cases():
        if case != "plane_1226x370":
            assert pf.P(rc.raycast_cases()[case][0]()) <= 256, case
    s = ref64.Scale(10544)
    assert s.u == 2.0 ** -10 and s(1e-3, rc.C_RAY) == rc.C_RAY * 2.0 ** -10
    assert ref64.ORIGIN.u == 0.0


def test_placements():
    assert len(set(pf.NEAR)) == 8 and pf.sign_coverage(pf.NEAR) and pf.sign_coverage(pf.FAR)
    assert (1000, -700, 1300) in pf.NEAR and (-1000, 700, -1300) in pf.NEAR
    m = am.sphere_outside(num_buckets=0x100)
    pl = pf.placements(m.block_pos)
    assert (m.block_pos.max(axis=0) + pl["edge_pos"][1] == pf.LAST_BLOCK).all()
    assert (m.block_pos.min(axis=0) + pl["edge_neg"][1] == pf.FIRST_BLOCK).all()
    assert pf.sign_coverage([pc.update_D(0, rv.MU_STEPS[0], p)[1] for p in pc.HEAVY])
    assert pf.u(pf.P(pf.shift_map(m, pl["edge_neg"][1]))) == 2.0 ** -5 and pf.u(10544) == 2.0 ** -10


@pytest.mark.parametrize("pname", ["near+-+", "far-", "edge_pos", "edge_neg"])
def test_a_moved_map_is_the_map_at_the_origin(pname):
    m0 = am.colour_plane(num_buckets=0x40)
    kind, D = pf.placements(m0.block_pos)[pname]
    m = pf.shift_map(m0, D)
    assert np.array_equal(m.block_pos - np.array(D), m0.block_pos) and m.voxels is m0.voxels
    assert m.max_chain >= 2 and (m.hash["ptr"][m.num_buckets:] >= 0).sum() >= 1
    # the same voxels answer at the moved coordinates, and the moved geometry and colour at the moved points
    p = m0.block_pos[::7] * 8 + np.array([3, 5, 1])
    for a, b in zip(m.lookup(p + 8 * np.array(D)), m0.lookup(p)):
        assert np.array_equal(a, b)
    x0 = p * m0.vs
    x = x0 + pf.shift_metres(D, m0.vs)
    assert np.abs(m.geom.sdf(x) - m0.geom.sdf(x0)).max() < 1e-9
    assert np.abs(m.colour(x) - m0.colour(x0)).max() < 1e-6
    # the pose: one float32 rounding of M T(-t); a moved point has the camera coordinates of the point at the origin
    M0, _ = rc.camera(64, 48, roll=0.2)
    M = pf.shift_pose(M0, D, m0.vs)
    got = ref64.mat_vec_f64(M, x)
    want = ref64.mat_vec_f64(M0, x0)
    assert np.abs(got - want).max() <= 2.0 * np.spacing(np.float32(np.abs(x).max()))
    for geom in (am.Sphere((0.03, -0.02, 0.45), 0.16), am.BoxCorner((0.16, 0.12, 0.55))):
        g = pf.shift_map(am.Map(m0.vs, m0.mu, m0.block_pos, m0.voxels, m0.num_buckets, m0.num_excess, m0.num_local_blocks, geom), D).geom
        assert np.abs(g.sdf(x) - geom.sdf(x0)).max() < 1e-9


def test_no_fusion_fixture_asks_for_a_block_beyond_the_range(synth):
    """From the depth images alone, in float64: every point an allocation pass can ask a block for, at every placement the
    fusion fixtures use, lies inside blocks -32768 .. 32766 with half of EDGE_MARGIN to spare; at the edges the outermost
    block is the last (first) one or the one before it (the tests assert the exact one on what the engine holds)."""
    wl = synth.s_tiny()
    seq = pf.workload_extent(wl, range(pc.SEQUENCE_FRAMES))
    batch = pf.workload_extent(wl, range(pc.BATCH_FRAMES + 1), pc.batch_new_poses(synth, wl))
    assert np.array_equal(seq[0], pc.parity_extent("sequence")[0]) and np.array_equal(batch[1], pc.parity_extent("batch")[1])
    spans = [(seq, [pc.parity_D("sequence", p) for p in pc.PARITY_PLACEMENTS]),
             (batch, [pc.parity_D("batch", p) for p in pc.PARITY_PLACEMENTS])]
    wl61 = synth.s_tiny(61, 47)
    import refmap_checks as rmc
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for i, (yaw, pitch) in pc.ALLOC_FRAMES:
        a, b = pf.requested_extent(wl61.frame(i)[1] / 1000.0, rmc.turned(synth, wl61, i, yaw, pitch), wl61.intr, 0.02, rmc.MU_OFF * 0.02, 3.0)
        lo, hi = np.minimum(lo, a), np.maximum(hi, b)
    spans.append(((lo, hi), [pc.alloc_D(p) for p in pc.HEAVY]))
    for k in range(4):
        for mu in rv.MU_STEPS:
            lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
            for seed in range(3):
                a, b = pf.requested_extent(rv.images(mu, seed)[1] * rv.STEP, rv.pose(k), rv.INTR, rv.VS, mu * rv.STEP, 3.0)
                lo, hi = np.minimum(lo, a), np.maximum(hi, b)
            spans.append(((lo, hi), [pc.update_D(k, mu, p) for p in pc.HEAVY]))
    for (lo, hi), Ds in spans:
        for kind, D in Ds:
            pf.assert_inside(lo - pf.EDGE_MARGIN / 2, hi + pf.EDGE_MARGIN / 2, D)
            if kind == "edge":  # (an axis whose outermost point falls within the margin of a block boundary stops one block short)
                a, b = np.floor(lo + np.array(D)), np.floor(hi + np.array(D))
                assert (b >= pf.LAST_BLOCK - 1).all() or (a <= pf.FIRST_BLOCK + 1).all(), (a, b)


@pytest.mark.parametrize("case", pc.RAYCAST_CASES)
def test_tie_caps_and_the_float32_march(case):
    """The reference alone.  At the D each case records (placement_checks.HALVINGS) the float64 march calls at most
    TIE_CAP of its hits ties at every placement; with one halving fewer some placement of the class misses the cap, or
    the check body's own floors (the rays left for the ICP normals), which is what put the edges one halving further in.
    The float32 restatement of the march agrees on the hits of every ray that is no tie and stays within C_RAY / 2 of
    the float64 hit in position and in depth: C_RAY is twice the worst seen."""
    worst = 0.0
    for pname in pc.PLACEMENTS:
        m, M, intr, W, H, _, scale, kind, D = pc.raycast_fixture(case, pname)
        ref = pc.raycast_reference(case, pname)
        share = pc.tie_share(ref)
        assert share <= pf.TIE_CAP[kind], f"{case} at {pname}, D = {D}: tie share {share:.3f}"
        f32 = ref32_march.cast_rays(m, M, intr, W, H)
        nt = ~ref["tie"]
        assert np.array_equal(f32["hit"][nt], ref["hit"][nt]), f"{case} at {pname}: float32 and float64 hits differ off the ties"
        both = f32["hit"] & ref["hit"] & nt
        derr = np.abs(f32["depth"].astype(np.float64) - ref64.camera_depth(M, ref["p"], m.vs))[both].max() / m.vs
        perr = np.abs(f32["p"].astype(np.float64) - ref["p"]).max(-1)[both].max()
        worst = max(worst, derr / scale.u, perr / scale.u)
        print(f"{case} at {pname}: D {D}, P {scale.P}, u {scale.u:.3g}, tie share {share:.3f}, float32 march {derr / scale.u:.2f} u in "
              f"depth, {perr / scale.u:.2f} u in position")
    assert worst <= rc.C_RAY / 2.0, f"the float32 march is {worst:.2f} u from the float64 one"
    for kind, pname in (("near", "near+-+"), ("far", "far+")):
        k = pc.HALVINGS[(case, kind)]
        assert k >= 1 and pc.tie_share(pc.raycast_reference(case, pname, k - 1)) > pf.TIE_CAP[kind], (case, kind)


@pytest.mark.parametrize("pname", ["near+-+", "far-", "edge_pos", "edge_neg"])
def test_range_law_tie_cap(pname):
    """The reference alone: the listed blocks the range law calls ties stay under the cap of the placement class (a range
    image has neither hits nor voxels; a tie block takes the cells of its box out of the comparison), and enough covered
    cells stay in it."""
    ref, kind = pc.range_law(pname)
    blocks, cells = ref.tie_shares()
    print(f"{pname}: {len(ref.ids)} listed, tie blocks {blocks:.3f}, tie cells {cells:.3f}")
    assert len(ref.ids) >= 100 and blocks <= pf.TIE_CAP[kind]
    assert ((ref.image[..., 0] != pc.rr.FAR_AWAY) & ~ref.tie_cells).sum() >= 20


@pytest.mark.parametrize("pname", pc.HEAVY)
def test_allocation_model_tie_cap(pkg, synth, pname):
    """The map model alone: the samples whose block the float32 and the float64 walk disagree on stay under the cap of the
    placement class, and no pixel's step count is a tie."""
    passes, kind = pc.allocation_model_passes(pkg, synth, pname)
    for info in passes:
        ties = info["block_ties"] + info["visibility_ties"] + info["gate_ties"]
        print(f"{pname}: {ties} ties in {info['samples']} samples, {info['commit_ties']} commits decided by one")
        assert ties <= pf.TIE_CAP[kind] * info["samples"] and info["step_tie_samples"] == 0, info
