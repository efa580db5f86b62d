"""The depth-to-SDF trackers on the MI355X far from the world origin, on the fixtures of
track_placement_fixtures.py: the far map (blocks up to the table's ends under the identity) and the far world (maps near
their own origins under world -> map transforms with position-sized translations).  One evaluation per fixture and
placement against the float64 reference's derived interval and, because that interval is wide far out, against the
measured distance of the float32 restatement (test_track_placement_ref.py asserts the constants; the engine gets FACTOR
times each); whole runs; the many-starts calls against the single call at one far placement."""
import numpy as np
import pytest

import placement_fixtures as pf
import ref64_track_sdf as rt
import test_gpu_track_sdf as single
import test_gpu_track_starts as many
import track_placement_fixtures as tp
import track_sdf_fixtures as fx

pytestmark = pytest.mark.gpu

RUNS = tp.cases(("identity", "posed"))


@pytest.fixture(scope="module")
def loaded(pkg, gpu):
    """test_gpu_track_sdf.py's: one scene per map, one view per depth image, shared by this file's tests (none writes a map).
    The far-world fixtures share the origin's maps and every fixture of one origin shares its depth image."""
    scenes, views = {}, {}

    def get(f):
        out = []
        for m in f.maps:
            if id(m) not in scenes:
                scenes[id(m)] = (m, single.upload_map(gpu, pkg, m))
            out.append(scenes[id(m)][1])
        key = id(f.mm)
        if key not in views:
            v = gpu.create_view(f.w, f.h)
            gpu.view_update(v, np.zeros((f.h, f.w, 4), np.uint8), f.mm)
            assert np.array_equal(gpu.download_view_depth(v), f.depth0)
            views[key] = (f.mm, v)
        return out, views[key][1]

    return get


# ---------------------------------------------------------------------------------------------------------------------
# 1. one evaluation per fixture and placement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,pname", tp.cases())
def test_single_evaluation_far_from_the_origin(pkg, gpu, loaded, which, pname):
    f = tp.placed(which, pname)
    scenes, _ = loaded(f)
    if f.far_map:
        # what the engine holds lies where the placement says: on D's side on every axis, at an unhalved edge at the last
        # or first block coordinate
        t = pf.teeth(gpu.download_hash_table(scenes[0]), f.D, pname[:-1] if pname in tp.UNHALVED else None)
        print(f"{f.name}: blocks {t['lo']} .. {t['hi']}, {t['chain_links']} chain links")
    else:
        # (a map transform's translation is of the world's size)
        assert all(np.linalg.norm(T[:3, 3]) > 0.5 * np.linalg.norm(pf.shift_metres(f.D, f.vs)) for T in f.T)
    # candidates, valid within the ties, the 33 sums and the cost inside the reference's interval, the pose's bytes
    ev, res, sums = single.check_evaluation(pkg, gpu, loaded, f, f.single_pose())
    ref = tp.reference_evaluation(which, pname)
    assert np.array_equal(ev.sums, ref.sums)
    if pname not in tp.UNHALVED:
        assert ev.tie_share <= pf.TIE_CAP[f.cls]
    assert ev.valid > 0.5 * ev.candidates
    # the measured check: the pivoted system against the reference's, the tie pixels' alternatives allowed for
    dH, dg = tp.system_distance(sums, ev)
    rH, rg = tp.system_distance(sums, ev, allow=False)
    print(f"{f.name}: H_c {dH:.3g} of its largest entry beyond the tie pixels' share ({rH:.3g} with it; allowed "
          f"{tp.FACTOR * tp.H_DEV[which][f.cls]:.3g}), g_c {dg:.3g} of its length ({rg:.3g}; allowed {tp.FACTOR * tp.G_DEV[which][f.cls]:.3g})")
    assert dH <= tp.FACTOR * tp.H_DEV[which][f.cls] and dg <= tp.FACTOR * tp.G_DEV[which][f.cls]


# ---------------------------------------------------------------------------------------------------------------------
# 2. whole runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,pname", RUNS)
def test_whole_run_far_from_the_origin(pkg, gpu, loaded, which, pname):
    """test_whole_run_against_the_reference's assertions with its tie-decision capping; a distance is bounded by the larger
    of the origin's rule and d_ref + C u(P), C = FACTOR x the restatement's worst excess."""
    f, M_ref, ref = tp.reference_run(which, pname)
    scenes, view = loaded(f)
    start = f.start()
    C = tp.FACTOR * tp.RUN_EXCESS_U * f.u
    M, res = gpu.track_camera_sdf(view, scenes, f.T, start, f.intr, pkg.TrackSdfParams(**fx.RUN_PARAMS))
    d_ref, d_gpu, apart = f.distance(M_ref), f.distance(M), rt.pose_distance(M, M_ref, f.corners, f.vs)
    order = sorted(ref["per_level"], reverse=True)
    tie_at = next(((lv, k) for lv in order for k, t in enumerate(ref["per_level"][lv]["trace"])
                   if k > 0 and t["margin"] < t["cost_slack"]), None)
    dev = abs(res.conditioning - ref["conditioning"]) / ref["conditioning"]
    print(f"{f.name}: u(P) = {f.u:.3g}; reference {ref['evaluations']} evaluations (stop {ref['stop_reason']}), engine "
          f"{res.evaluations} (stop {res.stop_reason}); distance to the truth {f.distance(start):.4g} -> {d_ref:.4g} / {d_gpu:.4g} "
          f"voxel ({(d_gpu - d_ref) / f.u:+.2f} u), apart {apart:.4g}; conditioning {ref['conditioning']:.5g} / {res.conditioning:.5g} "
          f"({dev:.2g} relative); first decision within the bound: (level, evaluation) {tie_at}")
    assert d_ref < 0.25 * f.distance(start)
    assert apart <= max(4 * d_ref, d_ref + C) and d_gpu <= max(2 * d_ref, d_ref + C)
    assert res.candidates == ref["candidates"]
    # what a caller judges the track by, at every placement
    assert res.conditioning > 0.25 and d_gpu < 0.05
    assert dev <= max(1e-3, tp.FACTOR * tp.COND_DEV[f.cls])
    # the capped comparison below keeps at least two accepted-or-rejected decisions of the coarsest level
    assert tie_at is None or tie_at[0] < order[0] or tie_at[1] >= 3
    if tie_at is None:
        M_cap, cap, M_g, r_g = M_ref, ref, M, res
    else:
        # compare up to the evaluation before that decision: both runs capped there (far out the cost's interval is wide:
        # the first such decision is evaluation 3 to 6 of the coarsest level)
        top = order[0]
        kw = dict(fx.RUN_PARAMS)
        kw.update(dict(run_till_level=top, max_evaluations=tie_at[1]) if tie_at[0] == top else dict(run_till_level=tie_at[0] + 1))
        M_cap, cap = rt.track(f.posed, f.depth0, f.intr, start, **kw)
        M_g, r_g = gpu.track_camera_sdf(view, scenes, f.T, start, f.intr, pkg.TrackSdfParams(**kw))
    assert r_g.evaluations == cap["evaluations"] and r_g.stop_reason == cap["stop_reason"]
    assert r_g.levels_stepped == cap["levels_stepped"]
    assert abs(r_g.valid_last - cap["valid_last"]) <= max(cap["last"].ties, 1)
    assert abs(r_g.conditioning - cap["conditioning"]) <= max(1e-3, tp.FACTOR * tp.COND_DEV[f.cls]) * cap["conditioning"] + 1e-6
    assert rt.pose_distance(M_g, M_cap, f.corners, f.vs) <= max(4 * d_ref, 1e-3, C)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the many-starts calls at one far placement
# ---------------------------------------------------------------------------------------------------------------------
def test_starts_and_scores_equal_the_single_call_far_out(pkg, gpu, loaded):
    """test_gpu_track_starts.py's comparison, at the far world's edge: every start's result, pose and sums are the single
    call's bytes, every score the single call's one evaluation."""
    f = tp.placed("posed", "edge_neg")
    scenes, view = loaded(f)
    params = pkg.TrackSdfParams(**fx.RUN_PARAMS)
    starts = [f.start(5.0, 1.0), f.start(2.0, 0.3), f.M_true, f.start(-5.0, -1.0)]
    M, res, singles = many.check_starts_against_single(pkg, gpu, view, scenes, f, starts, params)
    print(f"{f.name}: evaluations {[r.evaluations for r in res]}, stop reasons {[r.stop_reason for r in res]}, distances "
          f"{[round(f.distance(m), 4) for m in M]}, conditioning {[round(r.conditioning, 4) for r in res]}")
    assert f.distance(M[0]) < 0.05 and res[0].levels_stepped == 7 and all(r.conditioning > 0.25 for r in res)
    for level in range(3):
        scores = many.check_scores_against_single(pkg, gpu, view, scenes, f, starts, level)
        assert scores[0].valid > 0.5 * scores[0].candidates
    # and under the identity at the table's end
    g = tp.placed("identity", "edge_neg!")
    g_scenes, g_view = loaded(g)
    Mg, rg, _ = many.check_starts_against_single(pkg, gpu, g_view, g_scenes, g, [g.start(), g.M_true], params)
    assert g.distance(Mg[0]) < 0.05 and rg[0].conditioning > 0.25
