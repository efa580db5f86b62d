"""CPU checks of the photometric depth-to-SDF tracker's float64 reference (ref64_track_sdf_rgb.py) and its fixtures
(track_sdf_rgb_fixtures.py): what the GPU tests of test_gpu_track_sdf_rgb.py assume holds on the reference alone, the
contrast the feature exists for (a textured plane is tracked where the depth-only law slides), the reference's own
consistency, and that it tells the wrong laws apart."""
import numpy as np
import pytest

import ref64_track_sdf as rt
import ref64_track_sdf_rgb as rr
import track_sdf_rgb_fixtures as cf


@pytest.mark.parametrize("name", list("abcdefgh"))
def test_fixture_conditions(name):
    """Few ties, and more than half of the valid pixels colour-valid, except where the fixture is about colour that lacks."""
    f = cf.fixtures()[name]
    ev = cf.reference_evaluation(f, cf.evaluation_pose(f))
    print(f"({name}) {f.name}: {ev.candidates} candidates, {ev.valid} valid, {ev.colour_valid} colour-valid, {ev.ties} ties; "
          f"cost {ev.cost_depth:.4g} + k^2 {ev.cost_colour:.4g}")
    assert ev.candidates > 0.99 * f.w * f.h and ev.valid > 0.5 * ev.candidates and ev.tie_share < 0.01
    if name == "d":
        assert 0.3 * ev.valid < ev.colour_valid < 0.9 * ev.valid
    elif name == "e":
        assert ev.colour_valid == 0 and ev.sums[33] == 0.0 and ev.cost_colour == 0.0625
    else:
        assert ev.colour_valid > 0.5 * ev.valid
    assert np.all(ev.lo <= ev.sums) and np.all(ev.sums <= ev.hi)
    lo, hi = ev.cost_interval()
    assert lo <= ev.cost <= hi


@pytest.mark.parametrize("start", range(4))
def test_the_textured_plane_is_tracked_where_depth_alone_slides(start):
    """The feature: from each of the four starts the run with the photometric term ends within a quarter of its start
    distance, and the depth-only law from the same start ends no closer than half of it."""
    f, s, M, res = cf.reference_run("a", start)
    _, _, M_d, res_d = cf.depth_only_run("a", start)
    d0, d_rgb, d_depth = f.distance(s), f.distance(M), f.distance(M_d)
    print(f"start {start}: {d0:.4g} voxel -> {d_rgb:.4g} with the term ({res['evaluations']} evaluations, stop "
          f"{res['stop_reason']}, conditioning {res['conditioning']:.3g}, colour rms {res['colour_rms_last']:.4g}); "
          f"{d_depth:.4g} without (stop {res_d['stop_reason']}, conditioning {res_d['conditioning']:.3g})")
    assert d_rgb < 0.25 * d0
    assert d_depth >= 0.5 * d0
    assert res_d["conditioning"] < 1e-6 and res["conditioning"] > 1e-3
    assert res["colour_valid_last"] > 0.5 * res["valid_last"]


def test_the_term_conditions_the_plane():
    f = cf.plane()
    P = rt.camera_to_world(cf.evaluation_pose(f), f.vs)
    without = rt.evaluate(f.posed, f.depth0, f.intr, P)
    with_term = cf.reference_evaluation(f, cf.evaluation_pose(f))
    c0 = rt.conditioning(rt.pivot(without.sums, without.t)[1])
    c1 = rt.conditioning(rt.pivot(with_term.sums, with_term.t)[1])
    print(f"conditioning of the textured plane: {c0:.3g} without the term, {c1:.3g} with it")
    assert c0 < 1e-6 and c1 > 1e-3


def test_a_level_without_the_term_is_the_depth_only_evaluation():
    f = cf.posed_plane()
    pose = cf.evaluation_pose(f)
    for level in (0, 1):
        depth, intr = rt.pyramid(f.depth0, f.intr, level + 1)[level]
        base = rt.evaluate(f.posed, depth, intr, rt.camera_to_world(pose, f.vs))
        ev = cf.reference_evaluation(f, pose, level=level, colour_levels=1, run_till_level=level - 1)
        assert not ev.term and np.array_equal(ev.sums[:33], base.sums) and not ev.sums[33:].any()
        assert ev.cost == base.cost and np.array_equal(ev.lo[:33], base.lo) and np.array_equal(ev.hi[:33], base.hi)
    # and a map without colour leaves the depth sums alone on a level with the term
    g = cf.no_colour()
    base = rt.evaluate(g.posed, g.depth0, g.intr, rt.camera_to_world(cf.evaluation_pose(g), g.vs))
    ev = cf.reference_evaluation(g, cf.evaluation_pose(g))
    assert ev.term and np.array_equal(ev.sums[:33], base.sums) and ev.cost == base.cost + 0.0625


def test_the_colour_gradient_agrees_with_central_differences():
    """h is the gradient of a posed map's colour field with respect to the world point, the rotation back included."""
    f = cf.posed_plane()
    pm = f.posed[0]
    _, p, dp = rt.world_points(f.depth0, f.intr, rt.camera_to_world(cf.evaluation_pose(f), f.vs), f.vs)
    T = pm.Tt
    delta = 1e-3

    def field(pw):
        q = pw @ T[:, :3].T + T[:, 3]
        return q, rr.colour_field([pm], [q], [np.zeros_like(q)], [cells])

    q = p @ T[:, :3].T + T[:, 3]
    cells = np.floor(q).astype(np.int64)
    frac = q - cells
    inner = np.all((frac > 4 * delta) & (frac < 1 - 4 * delta), axis=1)   # the differences stay inside the cell
    _, (k, C, _, h, _) = field(p)
    assert (k[inner] == 1).sum() > 3000
    worst = 0.0
    for axis in range(3):
        step = np.zeros(3)
        step[axis] = delta
        _, (_, Cp, _, _, _) = field(p + step)
        _, (_, Cm, _, _, _) = field(p - step)
        diff = (Cp - Cm) / (2 * delta)
        worst = max(worst, float(np.abs(diff - h[:, axis])[inner & (k == 1)].max()))
    scale = float(np.abs(h[inner]).max())
    print(f"analytic colour gradient against central differences: largest difference {worst:.3g} of {scale:.3g} per voxel")
    assert scale > 0.01 and worst < 1e-6 * scale + 1e-9


WRONG = [("w_depth", "c"), ("tap0", "c"), ("unrotated", "b"), ("sign", "a"), ("swap_br", "a")]


@pytest.mark.parametrize("law,name", WRONG)
def test_wrong_laws_lie_outside_the_interval(law, name):
    f = cf.fixtures()[name]
    pose = cf.evaluation_pose(f)
    ev = cf.reference_evaluation(f, pose)
    wrong = cf.reference_evaluation(f, pose, law=law)
    out = ev.outside(wrong.sums)
    width = (ev.hi - ev.lo).clip(1e-300)
    far = np.maximum(wrong.sums - ev.hi, ev.lo - wrong.sums) / width
    print(f"{law} on ({name}): sums {out.tolist()} outside the interval, the farthest by {far.max():.3g} interval widths")
    assert len(out) >= 1 and far.max() > 5


def test_the_grey_pyramid_is_the_stated_float32_expression():
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (45, 70, 4), dtype=np.uint8)
    g = rr.grey_pyramid(rgba, 3)
    assert [x.shape for x in g] == [(45, 70), (22, 35), (11, 17)] and all(x.dtype == np.float32 for x in g)
    exact = (0.299 * rgba[..., 0] + 0.587 * rgba[..., 1] + 0.114 * rgba[..., 2]) / 255.0
    assert np.abs(g[0] - exact).max() < 4 * 2.0 ** -24
    assert g[1][3, 5] == np.float32(np.float32(np.float32(g[0][6, 10] + g[0][6, 11]) + np.float32(g[0][7, 10] + g[0][7, 11])) * np.float32(0.25))
    alpha = rgba.copy()
    alpha[..., 3] = 0
    assert np.array_equal(rr.grey_level0(alpha), g[0])


def test_the_binding_exists(pkg):
    import ctypes
    assert ctypes.sizeof(pkg.TrackSdfRgbParams) == 48 and ctypes.sizeof(pkg.TrackSdfRgbResult) == 48
    assert callable(pkg.CApi.track_camera_sdf_rgb) and callable(pkg.CApi.debug_track_sdf_rgb_sums)
    assert callable(pkg.CApi.debug_track_sdf_rgb_grey)
    exported = pkg.exported_symbols()
    for name in ("dslam_track_camera_sdf_rgb", "dslam_debug_track_sdf_rgb_sums", "dslam_debug_track_sdf_rgb_grey"):
        assert name in exported
    lib = open(pkg.LIB_PATH, "rb").read()
    assert b"k_track_sdf_rgb" in lib and b"k_grey_level0" in lib and b"k_grey_subsample" in lib
