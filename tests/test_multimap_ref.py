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
import weighted_fixtures as wf

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


# ---------------------------------------------------------------------------------------------------------------------
# weights that vary from voxel to voxel (weighted_fixtures.py)
# ---------------------------------------------------------------------------------------------------------------------
def test_trilinear_read_of_a_weight_field_against_a_plain_loop():
    """ref64_multimap._trilinear (sdf, colour, trilinear w_depth and w_color, found) against a scalar triple loop over the
    stored voxels, on points around the surface of a texture x ramp map and past the edge of its blocks."""
    pm = wf.ramp_spheres()[0]
    m = pm.m
    rng = np.random.default_rng(11)
    blocks = m.block_pos[rng.integers(0, len(m.block_pos), 300)]
    q = blocks * 8 + rng.uniform(-1.5, 9.5, (300, 3))
    stored = {}
    for b, vox in zip(m.block_pos, m.voxels):
        stored[tuple(int(v) for v in b)] = vox
    want = np.zeros((len(q), 7))
    for n, pt in enumerate(q):
        x0, y0, z0 = (int(np.floor(v)) for v in pt)
        cx, cy, cz = pt[0] - x0, pt[1] - y0, pt[2] - z0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    x, y, z = x0 + dx, y0 + dy, z0 + dz
                    coeff = (cx if dx else 1 - cx) * (cy if dy else 1 - cy) * (cz if dz else 1 - cz)
                    vox = stored.get((x >> 3, y >> 3, z >> 3))
                    if vox is None:
                        want[n, 0] += coeff * 1.0            # the default voxel: sdf 32767, nothing else
                        continue
                    v = vox[(x & 7) + 8 * (y & 7) + 64 * (z & 7)]
                    want[n, 0] += coeff * int(v["sdf"]) / 32767.0
                    want[n, 1:4] += coeff * v["clr"].astype(np.float64)
                    want[n, 4] += coeff * int(v["w_depth"])
                    want[n, 5] += coeff * int(v["w_color"])
                    want[n, 6] = 1.0
    s, wd, f = rm._trilinear(pm, q)
    c, wc, fc = rm._trilinear(pm, q, colour=True)
    got = np.concatenate([s[:, None], c, wd[:, None], wc[:, None], f[:, None].astype(np.float64)], axis=1)
    assert np.abs(got - want).max() < 1e-9, np.abs(got - want).max(axis=0)
    assert np.array_equal(f, fc) and 0 < (want[:, 6] == 0).sum() < 100 and (want[:, 4] > 0).sum() > 200
    assert len(np.unique(np.round(want[:, 4], 6))) > 150          # the weights do vary
    # the overrides: a number makes every stored voxel weigh that much
    flat = rm.Posed(m, pm.T)
    flat.w_depth, flat.w_color = 3.0, 2.0
    _, wd3, _ = rm._trilinear(flat, q)
    _, wc2, _ = rm._trilinear(flat, q, colour=True)
    share = np.zeros(len(q))
    for d in np.ndindex(2, 2, 2):
        cf = np.prod(np.where(np.array(d)[::-1] == 1, q - np.floor(q), 1 - (q - np.floor(q))), axis=1)
        share += cf * m.lookup(np.floor(q).astype(np.int64) + np.array(d)[::-1])[2]
    assert np.abs(wd3 - 3.0 * share).max() < 1e-12 and np.abs(wc2 - 2.0 * share).max() < 1e-12


def test_default_fields_leave_the_maps_as_they_were():
    """A map built without fields, with a constant field, and re-weighted by set_weights: the same bytes."""
    a = am.sphere_outside(w_depth=7, colour=lambda x: 100.0 + 200.0 * x)
    b = am.sphere_outside(colour=lambda x: 100.0 + 200.0 * x, w_depth_field=lambda p: np.full(p.shape[:-1], 7),
                          w_color_field=lambda p: np.full(p.shape[:-1], 1))
    assert a.voxels.tobytes() == b.voxels.tobytes() and a.vba.tobytes() == b.vba.tobytes() and a.hash.tobytes() == b.hash.tobytes()
    wd, wc = a.lookup_weights(a.block_pos * 8 + 3)
    assert (wd == 7).all() and (wc == 1).all()
    wd, wc = a.lookup_weights(a.block_pos.min(0) * 8 - 40)
    assert wd == 0 and wc == 0
    rm.set_weights(a, 9, 4)
    wd, wc = a.lookup_weights(a.block_pos * 8 + 3)
    assert (wd == 9).all() and (wc == 4).all()
    # w_depth 0: an unobserved voxel, or with keep_sdf the analytic sdf and the colour under the weight 0
    zero = lambda p: np.where(p[..., 0] % 2 == 0, 0, 5)
    c = am.sphere_outside(colour=lambda x: 100.0 + 200.0 * x, w_depth_field=zero)
    k = am.sphere_outside(colour=lambda x: 100.0 + 200.0 * x, w_depth_field=zero, keep_sdf=True)
    gone = c.voxels["w_depth"] == 0
    assert gone.mean() == 0.5 and (c.voxels["sdf"][gone] == 32767).all() and not c.voxels["clr"][gone].any()
    assert not c.voxels["w_color"][gone].any() and (c.voxels["w_color"][~gone] == 1).all()
    assert np.array_equal(k.voxels["w_depth"], c.voxels["w_depth"]) and np.array_equal(k.voxels["sdf"], a.voxels["sdf"])
    assert np.array_equal(k.voxels["clr"], a.voxels["clr"])


def test_ramp_moves_the_blended_surface_across_the_image():
    """On the texture x ramp spheres the reference's surface lies near map A's own sphere where A is heavy and near map B's
    (2 voxels further out) where B is, and a blend with each map's mean weight is far from it."""
    maps, M, intr, ref = wf.render_reference("ramp")
    h = ref["hit"] & ~ref["tie"]
    p = ref["p"][h]
    out = np.linalg.norm(p * am.VS - wf.C_WORLD, axis=1) / am.VS - wf.RADIUS / am.VS     # 0: A's sphere, 2: B's
    u = []
    for pm in maps:
        c = (pm.T[:3, :3].astype(np.float64) @ wf.C_WORLD + pm.T[:3, 3]) / am.VS
        u.append((pm.to_map(p)[:, 0] - c[0]) / 80.0 + 0.5)
    a_heavy, b_heavy = (u[0] > 0.65) & (u[1] > 0.65), (u[0] < 0.35) & (u[1] < 0.35)   # the ramps' flat ends
    print(f"offset from A's sphere: median {np.median(out[a_heavy]):.3f} voxel on the {a_heavy.sum()} pixels where A is heavy, "
          f"{np.median(out[b_heavy]):.3f} on the {b_heavy.sum()} where B is")
    assert a_heavy.sum() > 150 and b_heavy.sum() > 150
    assert np.median(out[a_heavy]) < 0.7 and np.median(out[b_heavy]) > 1.3
    d = ref64.camera_depth(M, ref["p"], am.VS)
    for name, alt in (("per-map mean weights", wf.mean_weight_maps(maps)), ("nearest tap's weight", wf.nearest_weight_maps(maps))):
        ra = rm.cast_rays(alt, M, intr, wf.W, wf.H)
        both = h & ra["hit"]
        margin = np.median(np.abs(d - ref64.camera_depth(M, ra["p"], am.VS))[both]) / am.VS
        print(f"median |ddepth| {margin:.3f} voxel between the law and the blend with {name}")
        assert both.sum() > 0.9 * h.sum() and margin >= 0.3, name


@pytest.mark.parametrize("name", ["ramp", "slab"])
def test_tie_share_of_the_weighted_gpu_fixtures(name):
    """The pixels the GPU tests cannot hold to the bound: at most the 1 % test_blending_law_against_float64 lets pass."""
    maps, M, intr, ref = wf.render_reference(name)
    refs = [ref] + ([rm.cast_rays(maps[::-1], M, intr, wf.W, wf.H, sharp_ties=True)] if name == "slab" else [])
    for r in refs:
        share = (r["tie"] & r["hit"]).sum() / r["hit"].sum()
        print(f"{name}: {r['hit'].sum()} hits, tie share {share:.3%}")
        assert r["hit"].sum() > 0.1 * wf.W * wf.H and share <= 0.01


def test_sharp_ties_are_a_subset_and_weights_flip_nothing_off_a_boundary():
    """The sharp tie flags only drop flags of the plain ones, and what they drop decided nothing: with the camera moved by
    2e-5 voxel (what float32 rounding does to a march position, a fifth of the tolerance), every pixel the plain flags mark
    and the sharp ones do not keeps its hit and moves its depth by less than the 1e-3 voxel the GPU tests hold it to."""
    for name in ("ramp", "slab"):
        maps, M, intr, ref = wf.render_reference(name)
        plain = rm.cast_rays(maps, M, intr, wf.W, wf.H)
        dropped = plain["tie"] & ~ref["tie"]
        assert not (ref["tie"] & ~plain["tie"]).any() and dropped.sum() > 10
        moved = np.array(M, np.float64)
        moved[:3, 3] += 2e-5 * am.VS * np.array([1.0, -1.0, 1.0])
        other = rm.cast_rays(maps, moved, intr, wf.W, wf.H, sharp_ties=True)
        assert np.array_equal(other["hit"][dropped], ref["hit"][dropped])
        h = dropped & ref["hit"]
        d = np.abs(ref64.camera_depth(M, ref["p"], am.VS) - ref64.camera_depth(moved, other["p"], am.VS))[h] / am.VS
        print(f"{name}: {dropped.sum()} flags dropped, {h.sum()} of them hits, depth moves by up to {d.max():.3g} voxel")
        assert d.max() < 1e-3
    maps = wf.slab_spheres()
    # den > 0 as a predicate on data: over every trilinear read the march makes off a flagged boundary, sum(w) == 0
    # exactly or sum(w) >= the smallest coefficient times the smallest weight -- never a value a rounding could flip
    rng = np.random.default_rng(5)
    for pm in maps:
        q = pm.m.block_pos[rng.integers(0, len(pm.m.block_pos), 4000)] * 8 + rng.uniform(0.0, 8.0, (4000, 3))
        off = ~rm._floor_tie(q, 1e-4)
        _, w, f = rm._trilinear(pm, q[off])
        assert ((w == 0) | (w >= 1e-4 ** 3)).all() and (w == 0).sum() > 100 and (f & (w == 0)).sum() > 100


def test_library_exports_entry_point_and_header_declares_limit(pkg):
    assert "dslam_get_image_multi" in pkg.exported_symbols()
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    assert re.search(r"#define\s+DSLAM_MAX_RENDER_MAPS\s+64\b", txt)
    assert "dslam_get_image_multi(" in txt
    assert pkg.MAX_RENDER_MAPS == 64
