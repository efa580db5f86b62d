"""What can be shown about the depth-to-SDF tracker far from the world origin without a device: the
halvings of track_placement_fixtures.py, and the float32 restatement of the law (ref32_track_sdf.py) against the float64
reference -- with the rows pivoted at the camera centre it stays in the reference's neighbourhood at every placement, with
the rows formed at the world origin, as the law stood, it leaves it from block 8000 on.  Every constant the GPU file
(test_gpu_track_placement.py) allows the engine a multiple of is asserted here on the restatement."""
import numpy as np
import pytest

import placement_fixtures as pf
import ref32_track_sdf as r32
import ref64_track_sdf as rt
import track_placement_fixtures as tp
import track_sdf_fixtures as fx

RUNS = tp.cases(("identity", "posed"))


@pytest.mark.parametrize("which,pname", tp.cases(unhalved=False))
def test_halved_until_the_tie_cap_is_met_and_no_further(which, pname):
    k = tp.HALVINGS[which, pname]
    f, ev = tp.placed(which, pname), tp.reference_evaluation(which, pname)
    cap = pf.TIE_CAP[f.cls]
    before = tp.reference_evaluation(which, pname, k - 1).tie_share if k else None
    print(f"{f.name}: u(P) = {f.u:.3g}, {k} halvings, tie share {ev.tie_share:.4f} (cap {cap}), one halving fewer: {before}")
    assert ev.tie_share <= cap and (before is None or before > cap)
    assert ev.candidates > 2000 and ev.valid > 0.5 * ev.candidates
    assert np.all(ev.lo <= ev.sums) and np.all(ev.sums <= ev.hi)
    assert all(np.sign(d) == np.sign(d0) for d, d0 in zip(f.D, tp.placement(which, pname, 0)[1]))


def test_the_window_at_the_origin_is_the_fixed_one():
    """At the origin the derived bound of q is below TIE_Q on every fixture, so every case there sees the ties it saw."""
    for f in (fx.identity_box(), fx.posed_box(), fx.ramp_spheres(), fx.three_maps(), fx.posed_plane()):
        _, p, dp = rt.world_points(f.depth0, f.intr, rt.camera_to_world(f.start(), f.vs), f.vs)
        for pm in f.posed:
            T = pm.Tt
            dq = dp if pm.identity else dp @ np.abs(T[:, :3]).T + 3 * rt.U * (np.abs(p) @ np.abs(T[:, :3]).T + np.abs(T[:, 3]))
            assert dq.max() < rt.TIE_Q, (f.name, dq.max())


@pytest.mark.parametrize("which,pname", tp.cases())
def test_one_evaluation_of_the_restatement(which, pname):
    f, ev = tp.placed(which, pname), tp.reference_evaluation(which, pname)
    Pt = rt.camera_to_world(f.single_pose(), f.vs)
    # every pixel: inside the interval the engine's sums are asked to lie in
    used = ev.check_sums(r32.evaluate(f.posed, f.depth0, f.intr, Pt), f.name)
    # the pixels the reference calls no tie: the pivoted system
    nt = ~ev.tie
    dH, dg = tp.system_distance(r32.evaluate(f.posed, f.depth0, f.intr, Pt, pixels=nt), ev, tie_pixels=False)
    wH, wg = tp.system_distance(r32.evaluate(f.posed, f.depth0, f.intr, Pt, pivot="world", pixels=nt), ev, tie_pixels=False,
                                rows_at_world=True)
    print(f"{f.name}: {ev.tie_share:.3f} ties, the sums use {used:.3g} of the bound; H_c {dH:.3g} of its largest entry (rows at the "
          f"world origin: {wH:.3g}), g_c {dg:.3g} of its length ({wg:.3g})")
    assert dH <= tp.H_DEV[which][f.cls] and dg <= tp.G_DEV[which][f.cls]
    # the law as it stood: what twice these constants would have turned away
    if f.cls != "near":
        assert wH > 10 * tp.FACTOR * tp.H_DEV[which][f.cls]
    if pname in tp.UNHALVED:
        assert wH > 1.0      # the largest entry of H_c is wrong by several times itself


@pytest.mark.parametrize("which,pname", RUNS)
def test_whole_runs_of_the_restatement(which, pname):
    f, M_ref, ref = tp.reference_run(which, pname)
    d0, d_ref = f.distance(f.start()), f.distance(M_ref)
    M, res = r32.track(f.posed, f.depth0, f.intr, f.start(), **fx.RUN_PARAMS)
    d, dev = f.distance(M), abs(res["conditioning"] - ref["conditioning"]) / ref["conditioning"]
    print(f"{f.name}: u(P) = {f.u:.3g}; {d0:.4g} -> reference {d_ref:.4g} voxel, conditioning {ref['conditioning']:.4g}; "
          f"restatement {d:.4g} ({(d - d_ref) / f.u:+.2f} u), conditioning {res['conditioning']:.4g} ({dev:.2g} relative)")
    assert d_ref < 0.25 * d0 and ref["conditioning"] > 0.25 and d_ref < 0.05
    assert d <= d_ref + tp.RUN_EXCESS_U * f.u and dev <= tp.COND_DEV[f.cls]
    assert res["conditioning"] > 0.25 and d < 0.05
    if which == "identity" and f.cls != "near":
        # the rows formed at the world origin: the conditioning is off by over five times what the engine is allowed, and at
        # the table's ends the track is lost
        Mw, rw = r32.track(f.posed, f.depth0, f.intr, f.start(), pivot="world", **fx.RUN_PARAMS)
        dw, devw = f.distance(Mw), abs(rw["conditioning"] - ref["conditioning"]) / ref["conditioning"]
        print(f"    rows at the world origin: {dw:.4g} voxel, conditioning {rw['conditioning']:.4g} ({devw:.2g} relative)")
        assert devw > 5 * max(1e-3, tp.FACTOR * tp.COND_DEV[f.cls])
        if pname in tp.UNHALVED:
            assert rw["conditioning"] < 0.25 and dw > 0.05 and dw > d_ref + tp.FACTOR * tp.RUN_EXCESS_U * f.u
