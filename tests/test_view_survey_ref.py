"""The view survey without a GPU: dslam_view_frustum_planes of the built library against
ref_view_survey.py bit for bit, the conservativeness of the reference's own float32 reach test on points drawn inside
frusta, and dslam_select_view_maps against the plain-Python restatement.  Both library calls are pure host functions, so
the library is loaded as test_abi.py loads it and no engine is opened."""
import ctypes

import numpy as np
import pytest

import ref_view_survey as rv
import view_survey_fixtures as vf

F32P, I32P = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib(pkg):
    pkg._share_torch_hip_runtime()
    return ctypes.CDLL(pkg.LIB_PATH)


def abi_view(pkg, v):
    return pkg.SurveyView.of(v.M, v.intr, v.width, v.height, float(v.near_m), float(v.far_m))


# ---------------------------------------------------------------------------------------------------------------------
# the planes
# ---------------------------------------------------------------------------------------------------------------------
def test_planes_equal_the_reference_bitwise(pkg, lib):
    cases = vf.random_views()
    assert len(cases) >= 200
    kinds = dict(no_far=0, no_near=0, one_pixel=0, centre_outside=0)
    for view, vs in cases:
        out = np.full(28, -7.0, np.float32)
        assert lib.dslam_view_frustum_planes(ctypes.byref(abi_view(pkg, view)), ctypes.c_float(vs), out.ctypes.data_as(F32P)) == 0
        want = rv.frustum_planes(view, vs)
        assert out.tobytes() == want.tobytes(), (view.M, view.intr, view.width, view.height, view.near_m, view.far_m, vs,
                                                 out.reshape(7, 4), want)
        kinds["no_far"] += view.far_m == 0
        kinds["no_near"] += view.near_m == 0
        kinds["one_pixel"] += (view.width, view.height) == (1, 1)
        kinds["centre_outside"] += not (0 <= view.intr[2] < view.width and 0 <= view.intr[3] < view.height)
        # of the law itself: unit normals, and with no far plane a row that always passes
        assert np.allclose(np.linalg.norm(want[:5, :3].astype(np.float64), axis=1), 1.0, atol=1e-5)
        if view.far_m == 0:
            assert want[5].tolist() == [0.0, 0.0, 0.0, np.inf]
    print(f"{len(cases)} views: {kinds}")
    assert all(v >= 10 for v in kinds.values()), kinds


def test_plane_rejections_leave_the_output_untouched(pkg, lib):
    view, vs = vf.random_views()[0]

    def refused(v=view, voxel=vs, null=()):
        out = np.full(28, -7.0, np.float32)
        rc = lib.dslam_view_frustum_planes(None if "view" in null else ctypes.byref(abi_view(pkg, v)), ctypes.c_float(voxel),
                                           None if "out" in null else out.ctypes.data_as(F32P))
        assert rc == -1 and (out == -7.0).all()

    def changed(**kw):
        v = rv.View(view.M.copy(), view.intr.copy(), view.width, view.height, view.near_m, view.far_m)
        for k, val in kw.items():
            setattr(v, k, val)
        return v

    refused(null=("view",))
    refused(null=("out",))
    for bad in (np.nan, np.inf):
        M = view.M.copy(); M[1, 3] = bad
        refused(changed(M=M))
        intr = view.intr.copy(); intr[2] = bad
        refused(changed(intr=intr))
        refused(changed(near_m=np.float32(bad)))
        refused(changed(far_m=np.float32(bad)))
        refused(voxel=bad)
    skew = view.M.copy(); skew[:3, :3] *= 1.001
    refused(changed(M=skew))
    for k in (0, 1):
        for f in (0.0, -5.0):
            intr = view.intr.copy(); intr[k] = f
            refused(changed(intr=intr))
    refused(changed(width=0))
    refused(changed(height=0))
    refused(changed(height=-3))
    refused(changed(near_m=np.float32(-0.1)))
    refused(changed(far_m=np.float32(-1.0)))
    refused(changed(near_m=np.float32(0.5), far_m=np.float32(0.5)))
    refused(changed(near_m=np.float32(0.5), far_m=np.float32(0.25)))
    refused(voxel=0.0)
    refused(voxel=-0.005)


# ---------------------------------------------------------------------------------------------------------------------
# the reference's reach test is conservative
# ---------------------------------------------------------------------------------------------------------------------
def test_a_point_inside_a_frustum_lies_in_a_block_that_reaches():
    """Points at integer pixels and depths in (near, far] of seeded views, taken into maps under random rigid T_i whose
    translation is up to 10^4 voxels long: the block that holds each point reaches under the float32 law with a margin of
    0.5 voxel.  In exact arithmetic the block's centre lies within 4 sqrt(3) voxels of the point and the point has
    s_k > 0, so s_k(centre) + rho > 0.5; what is lost of that is float32 rounding."""
    rng = np.random.default_rng(2025)
    rho = rv.rho_of(0.5)
    points, smallest, per_view = 0, np.inf, 500
    for view, vs in vf.random_views():
        vs = float(np.float32(vs))
        T = vf.rigid(rng, 1.0)
        T[:3, 3] = (T[:3, 3].astype(np.float64) * rng.uniform(0.0, 1.0e4) * vs).astype(np.float32)    # |t| <= 10^4 voxels
        assert np.linalg.norm(T[:3, 3].astype(np.float64)) / vs <= 1.0e4 * 1.0001
        near, far = float(view.near_m), float(view.far_m) if view.far_m > 0 else float(view.near_m) + 10.0
        x = rng.integers(0, view.width, per_view).astype(np.float64)
        y = rng.integers(0, view.height, per_view).astype(np.float64)
        D = far - rng.uniform(0.0, 1.0, per_view) * (far - near) * 0.999999      # in (near, far]
        assert (D > near).all() and (D <= far).all()
        fx, fy, cx, cy = (float(v) for v in view.intr)
        pc = np.stack([D * (x - cx) / fx, D * (y - cy) / fy, D, np.ones(per_view)], -1)
        pw = pc @ np.linalg.inv(view.M.astype(np.float64)).T          # metres, world
        q = (pw @ T.astype(np.float64).T)[:, :3] / vs                 # voxels, map
        B = np.floor(q / 8.0).astype(np.int64)
        assert np.abs(B).max() < 32768
        planes = rv.frustum_planes(view, vs)
        s, _ = rv.plane_values(planes, rv.world_points(B, T, vs))
        assert rv.reaching(planes, rv.world_points(B, T, vs), rho)[0].all(), (view.M, T, float((s.astype(np.float64) + float(rho)).min()))
        smallest = min(smallest, float((s.astype(np.float64) + float(rho)).min()))
        points += per_view
    print(f"{points} points: the smallest s_k + rho at a margin of 0.5 voxel is {smallest:.4f} voxels")
    assert points >= 100000
    assert smallest > 0.0, f"the smallest s_k + rho seen over {points} points is {smallest}"


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
def lib_select(pkg, lib, reach, nearest, params, nv=None, n=None, null=()):
    reach, nearest = np.ascontiguousarray(reach, np.int32), np.ascontiguousarray(nearest, np.int32)
    maps, res = np.full(pkg.MAX_RENDER_MAPS + 1, -7, np.int32), pkg.ViewSelectResult(-7, -7)
    rc = lib.dslam_select_view_maps(None if "reach" in null else reach.ctypes.data_as(I32P),
                                    None if "nearest" in null else nearest.ctypes.data_as(I32P),
                                    ctypes.c_int(reach.shape[0] if nv is None else nv), ctypes.c_int(reach.shape[1] if n is None else n),
                                    ctypes.byref(params) if params is not None else None,
                                    None if "maps" in null else maps.ctypes.data_as(I32P), None if "result" in null else ctypes.byref(res))
    return rc, maps, res


def test_selection_equals_the_reference(pkg, lib):
    cases = vf.selection_cases()
    assert len(cases) >= 200
    seen = dict(capped=0, kept_without_reach=0, nearest_ties=0, sum_ties=0)
    for reach, nearest, params in cases:
        rc, maps, res = lib_select(pkg, lib, reach, nearest, pkg.ViewSelectParams(**params))
        want, counts = rv.select(reach, nearest, **params)
        assert rc == 0 and maps[:res.selected].tolist() == want and res.as_dict() == counts, (params, maps, want)
        assert (maps[res.selected:] == -7).all()                      # nothing is written past `selected`
        assert want == sorted(want) and len(set(want)) == len(want)   # ascending
        keep = params["always_keep"]
        if keep >= 0:
            assert keep in want
            seen["kept_without_reach"] += all(r[keep] == 0 for r in reach)
        if counts["selected"] < counts["reaching"]:
            seen["capped"] += 1
            assert counts["selected"] == (params["max_maps"] or pkg.MAX_RENDER_MAPS)
            # ties at the cut: a dropped candidate with the nearest depth of a kept one (and then with its sum)
            near = lambda i: min(row[i] for row in nearest)
            total = lambda i: sum(row[i] for row in reach)
            min_blocks = params["min_blocks"] or 1
            dropped = [i for i in range(len(reach[0])) if i not in want and max(r[i] for r in reach) >= min_blocks]
            kept = [i for i in want if i != keep]
            seen["nearest_ties"] += any(near(d) == near(k) for d in dropped for k in kept)
            seen["sum_ties"] += any(near(d) == near(k) and total(d) == total(k) for d in dropped for k in kept)
    print(f"{len(cases)} selections: {seen}")
    assert seen["capped"] >= 40 and seen["kept_without_reach"] >= 10 and seen["nearest_ties"] >= 20 and seen["sum_ties"] >= 3, seen
    # NULL params: the defaults, no map kept regardless
    reach, nearest, _ = cases[0]
    rc, maps, res = lib_select(pkg, lib, reach, nearest, None)
    assert rc == 0 and maps[:res.selected].tolist() == rv.select(reach, nearest)[0]


def test_selection_rejections_leave_the_outputs_untouched(pkg, lib):
    reach, nearest, _ = vf.selection_cases()[1]

    def refused(params=None, **kw):
        rc, maps, res = lib_select(pkg, lib, reach, nearest, params, **kw)
        assert rc == -1 and (maps == -7).all() and (res.reaching, res.selected) == (-7, -7)

    for what in ("reach", "nearest", "maps", "result"):
        refused(null=(what,))
    refused(nv=0)
    refused(nv=pkg.MAX_SURVEY_VIEWS + 1)
    refused(n=0)
    refused(n=pkg.MAX_SURVEY_MAPS + 1)
    refused(pkg.ViewSelectParams(min_blocks=-1))
    refused(pkg.ViewSelectParams(max_maps=-1))
    refused(pkg.ViewSelectParams(always_keep=-2))
    refused(pkg.ViewSelectParams(always_keep=len(reach[0])))
    refused(pkg.ViewSelectParams(max_maps=pkg.MAX_RENDER_MAPS + 1))
    bad_pad = pkg.ViewSelectParams()
    bad_pad.pad = -1
    refused(bad_pad)
