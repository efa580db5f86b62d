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


@pytest.mark.parametrize("name", ["two_spheres", "seam_planes"])
def test_tie_share_of_the_gpu_fixtures(name):
    ref = fx.reference(name)
    assert sum(int(r["produce"].sum()) for r in ref) > 5000
    share = r64.tie_share(ref)
    print(f"{name}: tie share {share:.4%}")
    assert share <= 0.02, f"{name}: {share:.3%} of the triangle-producing cubes are ties"


def test_boundary_exports_declares_and_wraps_the_call(pkg):
    assert "dslam_mesh_scene_multi" in pkg.exported_symbols()
    header = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+dslam_mesh_scene_multi\s*\(", header)
    assert callable(getattr(pkg.CApi, "mesh_scene_multi", None))
