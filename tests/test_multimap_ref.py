"""CPU checks of the composite raycast (dslam_get_image_multi): the float64 reference of ref64_multimap.py reduces to
ref64.cast_rays for one map at the identity, the blending law is what it says, and the library / header carry the entry
point."""
import os
import re

import numpy as np
import pytest

import analytic_maps as am
import ref64
import ref64_checks as rc
import ref64_multimap as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("make", [am.sphere_outside, am.tilted_plane])
def test_one_identity_map_equals_single_map_reference(make):
    W, H = 64, 48
    m = make()
    M, intr = rc.camera(W, H, yaw=0.1, pitch=-0.05)
    single = ref64.cast_rays(m, M, intr, W, H)
    multi = rm.cast_rays([rm.Posed(m, np.eye(4))], M, intr, W, H)
    for k in ("p", "hit", "tie", "p_stop", "sdf_stop"):
        assert np.array_equal(single[k], multi[k], equal_nan=True), k
    assert single["hit"].sum() > 0.1 * W * H


def test_posed_map_matches_its_own_camera():
    """A map built at the identity and moved by T (geometry moved with it) renders from M like the map from M T^-1."""
    W, H = 48, 40
    m = am.sphere_outside()
    M, intr = rc.camera(W, H)
    T = np.eye(4)
    T[:3, :3] = rc.camera(W, H, yaw=0.2, roll=0.1)[0][:3, :3]
    T[:3, 3] = (0.02, -0.01, 0.03)
    multi = rm.cast_rays([rm.Posed(m, T)], M, intr, W, H)
    single = ref64.cast_rays(m, rm.camera_of(M, T), intr, W, H)
    ok = ~multi["tie"] & ~single["tie"]
    assert np.array_equal(multi["hit"][ok], single["hit"][ok])
    both = multi["hit"] & single["hit"] & ok
    assert both.sum() > 0.05 * W * H
    # world hit points of the composite, mapped into the map, are the single-map hits
    q = multi["p"][both] @ T[:3, :3].T + T[:3, 3] / m.vs
    assert np.abs(q - single["p"][both]).max() < 1e-3


def test_blending_law_weighted_mean():
    """Two maps of the same sphere with radii two voxels apart and w_depth 5 / 20: the combined surface sits where
    (5 d_A + 20 d_B) / 25 = 0, i.e. 0.8 of the way from A's surface to B's."""
    W, H = 48, 40
    c, r = np.array([0.03, -0.02, 0.45]), 0.16
    a = rm.set_weights(am.build_map(am.Sphere(c, r), am.VS, am.MU, c - 0.2, c + 0.2), 5)
    b = rm.set_weights(am.build_map(am.Sphere(c, r + 2 * am.VS), am.VS, am.MU, c - 0.2, c + 0.2), 20)
    M, intr = rc.camera(W, H)
    out = rm.cast_rays([rm.Posed(a, np.eye(4)), rm.Posed(b, np.eye(4))], M, intr, W, H)
    h = out["hit"] & ~out["tie"]
    assert h.sum() > 0.05 * W * H
    dist = (np.linalg.norm(out["p"][h] * am.VS - c, axis=1) - r) / am.VS
    assert np.abs(np.median(dist) - 1.6) < 0.1, np.median(dist)


def test_library_exports_entry_point_and_header_declares_limit(pkg):
    assert "dslam_get_image_multi" in pkg.exported_symbols()
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    assert re.search(r"#define\s+DSLAM_MAX_RENDER_MAPS\s+64\b", txt)
    assert "dslam_get_image_multi(" in txt
    assert pkg.MAX_RENDER_MAPS == 64
