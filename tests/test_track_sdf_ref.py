"""CPU checks of the depth-to-SDF tracker's float64 reference (ref64_track_sdf.py) and its fixtures
(track_sdf_fixtures.py): what the GPU tests of test_gpu_track_sdf.py assume holds on the reference alone, the reference's
interpolants are checked against independent statements, and the binding exists."""
import numpy as np
import pytest

import ref64_track_sdf as rt
import track_sdf_fixtures as fx

FIXTURES = {"identity": fx.identity_box, "posed": fx.posed_box, "ramp": fx.ramp_spheres, "three": fx.three_maps,
            "plane": fx.posed_plane}


@pytest.mark.parametrize("which", sorted(FIXTURES))
def test_start_pose_has_few_ties_and_mostly_valid_pixels(which):
    f = FIXTURES[which]()
    for M0 in (f.M_true, f.start(2.0, 0.3), f.start()):
        ev = rt.evaluate(f.posed, f.depth0, f.intr, rt.camera_to_world(M0, f.vs))
        print(f"{f.name} at {f.distance(M0):.3g} voxel: {ev.candidates} candidates, {ev.valid} valid, {ev.ties} ties, "
              f"{ev.maps_per_pixel:.2f} maps per pixel, cost {ev.cost:.5g}")
        assert ev.candidates > 2000 and ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates
        assert np.all(ev.lo <= ev.sums) and np.all(ev.sums <= ev.hi)
    assert any(not pm.identity for pm in f.posed) or which == "identity"


@pytest.mark.parametrize("which", ["identity", "posed", "three"])
def test_whole_run_recovers_the_offset(which):
    f, M, res = fx.reference_run(which)
    start, end = f.distance(f.start()), f.distance(M)
    per = {lv: (v["evaluations"], v["stop_reason"]) for lv, v in res["per_level"].items()}
    print(f"{f.name}: {start:.4g} voxel at the start, {end:.4g} after {res['evaluations']} evaluations (level: evaluations, stop "
          f"{per}); cost {res['cost_first']:.5g} -> {res['cost_last']:.5g}, conditioning {res['conditioning']:.3g}")
    assert start > 1.0 and end < 0.25 * start
    assert res["levels_stepped"] == 7 and res["conditioning"] > 0.1


def test_a_level_without_enough_pixels_changes_nothing():
    """Default min_valid = 500 and 432 pixels on level 2: that level stops with reason 3 and the next starts where it did."""
    f = fx.identity_box()
    M, res = rt.track(f.posed, f.depth0, f.intr, f.start())
    assert res["per_level"][2]["stop_reason"] == 3 and res["per_level"][2]["evaluations"] == 1
    assert res["levels_stepped"] == 3 and f.distance(M) < 0.25 * f.distance(f.start())
    first = res["per_level"][1]["trace"][0]["ev"]
    alone = rt.evaluate(f.posed, rt.pyramid(f.depth0, f.intr, 2)[1][0], rt.pyramid(f.depth0, f.intr, 2)[1][1],
                        rt.camera_to_world(f.start(), f.vs))
    assert np.array_equal(first.sums, alone.sums)


def test_analytic_gradient_against_central_differences():
    """The gradient the reference states is the derivative of its own interpolant (trilinear: exact up to rounding for a
    step that stays inside the cell)."""
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (200, 8))
    c = rng.uniform(0.05, 0.95, (200, 3))
    _, g = rt._lerp3(v, c)
    h = 1e-3
    for axis in range(3):
        e = np.zeros(3)
        e[axis] = h
        num = (rt._lerp3(v, c + e)[0] - rt._lerp3(v, c - e)[0]) / (2 * h)
        assert np.abs(num - g[:, axis]).max() < 1e-9


def test_weight_lerp_against_a_scalar_triple_loop():
    f = fx.ramp_spheres()
    pm = f.posed[0]
    _, p, dp = rt.world_points(f.depth0, f.intr, rt.camera_to_world(f.start(2.0, 0.3), f.vs), f.vs)
    q = p @ pm.Tt[:, :3].T + pm.Tt[:, 3]
    cell = np.floor(q).astype(np.int64)
    ok, d, g, om, *_ = rt.read_map(pm, q, cell, dp)
    pick = np.flatnonzero(ok)[::37]
    assert len(pick) > 30
    m = f.maps[0]
    distinct = 0
    for i in pick:
        acc_w = acc_d = 0.0
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    tap = cell[i] + (dx, dy, dz)
                    k = 1.0
                    for a, o in enumerate((dx, dy, dz)):
                        fr = q[i, a] - cell[i, a]
                        k *= fr if o else 1.0 - fr
                    wd, _ = m.lookup_weights(tap)
                    sdf, _, found = m.lookup(tap)
                    assert found and wd > 0
                    acc_w += k * float(wd)
                    acc_d += k * float(sdf) / 32767.0
        assert abs(acc_w - om[i]) < 1e-9 * max(acc_w, 1.0) and abs(acc_d - d[i]) < 1e-12
        distinct += abs(om[i] - float(m.lookup_weights(cell[i])[0])) > 0.5
    assert distinct > len(pick) // 2     # the trilinear weight is not tap 0's


def test_ramp_fixture_separates_the_weight_laws():
    """On the two ramp spheres the two maps' values have opposite signs, so the blend is the weights': the law's sums lie
    far outside what weights from tap 0, or an unweighted mean, give (as test_ramp_moves_the_blended_surface_across_the_image
    shows for the composite raycast)."""
    f = fx.ramp_spheres()
    P = rt.camera_to_world(f.start(2.0, 0.3), f.vs)
    ev = rt.evaluate(f.posed, f.depth0, f.intr, P)
    assert ev.maps_per_pixel > 1.9
    for law in ("tap0", "unweighted"):
        wrong = rt.evaluate(f.posed, f.depth0, f.intr, P, weight_law=law)
        width = ev.hi - ev.lo
        outside = np.maximum(wrong.sums - ev.hi, ev.lo - wrong.sums) / width.clip(1e-300)
        moved = np.abs(wrong.d - ev.d)[np.isfinite(ev.d)] * (f.maps[0].mu / f.vs)
        print(f"{law}: sum b^2 {wrong.sums[27]:.5g} against {ev.sums[27]:.5g} ({outside[27]:.0f} interval widths outside); the value "
              f"moves by {np.median(moved):.3g} voxel (median)")
        assert outside[27] > 20 and (outside[21:27] > 5).all() and np.median(moved) > 0.05


def test_a_map_without_the_point_contributes_nothing():
    f = fx.three_maps()
    P = rt.camera_to_world(f.start(2.0, 0.3), f.vs)
    all3 = rt.evaluate(f.posed, f.depth0, f.intr, P)
    two = rt.evaluate([f.posed[0], f.posed[2]], f.depth0, f.intr, P)
    assert np.array_equal(all3.sums, two.sums)
    one = rt.evaluate(f.posed[:1], f.depth0, f.intr, P)
    assert not np.array_equal(one.sums[:28], two.sums[:28])


def test_the_binding_exists(pkg):
    import ctypes
    assert ctypes.sizeof(pkg.TrackSdfParams) == 32 and ctypes.sizeof(pkg.TrackSdfResult) == 32
    assert callable(pkg.CApi.track_camera_sdf) and callable(pkg.CApi.debug_track_sdf_sums)
    exported = pkg.exported_symbols()
    assert "dslam_track_camera_sdf" in exported and "dslam_debug_track_sdf_sums" in exported
    assert b"k_track_sdf" in open(pkg.LIB_PATH, "rb").read()
