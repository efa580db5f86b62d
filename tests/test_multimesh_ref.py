"""No-GPU checks of the composite mesh (dslam_mesh_scene_multi): the float64 reference of ref64_multimesh.py against a
plain marching-cubes restatement and against closed-form geometry, the tie share of the fixtures the GPU tests compare
cube by cube, and the boundary (symbol, declaration, wrapper)."""
import os
import re

import numpy as np
import pytest

import analytic_maps as am
import multimesh_fixtures as fx
import ref64_multimap as rm
import ref64_multimesh as r64
import weighted_fixtures as wf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_marching_cubes(m):
    """dslam_mesh_scene restated voxel by voxel: per cube a list of triangles [k, 3, 3] in metres, keyed by its voxel."""
    vs = float(np.float32(m.vs))
    out = {}
    blocks = r64.live_blocks(m)
    loc = [(x, y, z) for z in range(8) for y in range(8) for x in range(8)]
    for b in blocks:
        g = b[None, :] * 8 + np.array(loc)
        s, _, f = m.lookup(g[:, None, :] + r64.CORNERS[None])
        ok = f.all(1) & (s != 32767).all(1)
        for c in np.nonzero(ok)[0]:
            v = s[c] / 32767.0
            case = sum(1 << k for k in range(8) if v[k] < 0)
            row = r64.TABLE[case]
            tris = []
            for t in range(0, 15, 3):
                if row[t] < 0:
                    break
                tri = []
                for e in row[t:t + 3]:
                    a, bb = r64.EDGES[e]
                    pa, pb = g[c] + r64.CORNERS[a], g[c] + r64.CORNERS[bb]
                    if abs(v[a]) < 1e-5:
                        p = pa.astype(float)
                    elif abs(v[bb]) < 1e-5:
                        p = pb.astype(float)
                    elif abs(v[a] - v[bb]) < 1e-5:
                        p = pa.astype(float)
                    else:
                        p = pa + (0.0 - v[a]) / (v[bb] - v[a]) * (pb - pa)
                    tri.append(p * vs)
                tris.append(tri)
            if tris:
                out[tuple(g[c])] = np.array(tris)
    return out


def test_one_identity_map_is_plain_marching_cubes():
    m = am.colour_plane(holes=0.1, seed=3)
    ref, = r64.mesh_maps([rm.Posed(m, fx.I4)])
    plain = _plain_marching_cubes(m)
    assert len(plain) > 2000 and not ref["tie"].any()
    kept = np.nonzero(ref["kept"])[0]
    assert {tuple(g) for g in ref["g"][kept]} == set(plain)
    for c in kept:
        want = plain[tuple(ref["g"][c])]
        assert ref["ntri"][c] == len(want)
        assert np.array_equal(ref["tris"][c, :len(want)], want)


def test_two_spheres_reference_lies_on_the_blended_radius():
    maps, c_world, r = fx.two_spheres()
    ref = fx.reference("two_spheres")
    tris = r64.triangles(ref)
    assert len(tris) > 10000
    d = np.linalg.norm(tris.reshape(-1, 3) - c_world, axis=1) / am.VS
    assert np.abs(d - (r / am.VS + 1.6)).max() <= 0.25, np.abs(d - (r / am.VS + 1.6)).max()
    assert ref[1]["ntri"].sum() == 0   # the first map has no hole: the second adds nothing


def test_seam_reference_lies_on_the_wall():
    off, edge = fx.seam_wall_offsets(r64.triangles(fx.reference("seam_planes")))
    assert len(off) > 20000 and edge.mean() < 0.25
    assert off[~edge].max() <= 0.25 and off[edge].max() <= 1.0, (off[~edge].max(), off[edge].max())


@pytest.mark.parametrize("name", ["two_spheres", "seam_planes", "weighted_spheres"])
def test_tie_share_of_the_gpu_fixtures(name):
    ref = fx.reference(name)
    assert sum(int(r["produce"].sum()) for r in ref) > 5000
    share = r64.tie_share(ref)
    print(f"{name}: tie share {share:.4%}")
    assert share <= 0.02, f"{name}: {share:.3%} of the triangle-producing cubes are ties"


def test_weighted_reference_uncovers_the_slab_and_reads_each_voxels_weight():
    """mesh_maps on weighted_fixtures.mesh_spheres: map 1's cubes whose centre lies in map 0's slab without weight are kept,
    those on a weighted voxel of map 0 are covered; and a lattice value of map 0, recomputed in a plain loop from the
    stored voxels (own sdf and w_depth, map 1's 8 taps and their weights), gives the vertex the reference puts on the edge."""
    maps = fx.fixture("weighted_spheres")
    ref = fx.reference("weighted_spheres")
    A, B = maps
    r = ref[1]
    to_world = np.linalg.inv(r["T"])
    centre = A.to_map((r["g"] + 0.5) @ to_world[:3, :3].T + to_world[:3, 3])
    v = centre[:, 1] - (A.T[:3, :3].astype(np.float64) @ wf.C_WORLD + A.T[:3, 3])[1] / am.VS
    near = np.floor(centre + 0.5).astype(np.int64)
    held = A.m.lookup(near)[2]
    lo, hi = wf.MESH_SLAB
    prod = r["produce"] & ~r["tie"]
    inside, outside = prod & held & (v > lo + 1.5) & (v < hi - 1.5), prod & held & ((v < lo - 1.5) | (v > hi + 1.5))
    assert inside.sum() > 1000 and r["kept"][inside].all() and (A.m.lookup_weights(near[inside])[0] == 0).all()
    assert outside.sum() > 10000 and not r["kept"][outside].any() and (A.m.lookup_weights(near[outside])[0] > 0).all()
    # blended lattice values of map 0 on the x edges of some kept cubes, from the stored voxels
    r0 = ref[0]
    stored = [{tuple(int(c) for c in pos): vox for pos, vox in zip(pm.m.block_pos, pm.m.voxels)} for pm in maps]

    def voxel(k, p):
        vox = stored[k].get(tuple(int(c) >> 3 for c in p))
        return None if vox is None else vox[(int(p[0]) & 7) + 8 * (int(p[1]) & 7) + 64 * (int(p[2]) & 7)]

    T01 = r64.voxel_transform(B) @ np.linalg.inv(r64.voxel_transform(A))

    def blended(g):
        own = voxel(0, g)
        q = T01[:3, :3] @ g + T01[:3, 3]
        q0 = np.floor(q).astype(np.int64)
        c = q - q0
        val = wt = 0.0
        found = False
        for d in np.ndindex(2, 2, 2):
            tap = voxel(1, q0 + np.array(d)[::-1])
            cf = np.prod(np.where(np.array(d)[::-1] == 1, c, 1 - c))
            val += cf * (1.0 if tap is None else int(tap["sdf"]) / 32767.0)
            wt += cf * (0 if tap is None else int(tap["w_depth"]))
            found |= tap is not None
        s, w = int(own["sdf"]) / 32767.0, int(own["w_depth"])
        return (w * s + wt * val) / (w + wt) if found and w + wt > 0 else s

    checked = 0
    for cidx in np.nonzero(r0["kept"] & ~r0["tie"])[0][::97]:
        g = r0["g"][cidx].astype(np.float64)
        v0, v1 = blended(g), blended(g + np.array([1.0, 0.0, 0.0]))
        if (v0 < 0) == (v1 < 0):
            continue
        want = (g + np.array([v0 / (v0 - v1), 0.0, 0.0])) @ np.linalg.inv(r0["T"])[:3, :3].T + np.linalg.inv(r0["T"])[:3, 3]
        dist = np.abs(r0["tris"][cidx, :r0["ntri"][cidx]].reshape(-1, 3) / float(np.float32(am.VS)) - want).max(axis=1).min()
        assert dist < 1e-9, (g, dist)
        checked += 1
    assert checked > 50


def test_boundary_exports_declares_and_wraps_the_call(pkg):
    assert "dslam_mesh_scene_multi" in pkg.exported_symbols()
    header = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+dslam_mesh_scene_multi\s*\(", header)
    assert callable(getattr(pkg.CApi, "mesh_scene_multi", None))
