"""The reference of the occupancy and distance grids (ref_distance_field.py) checked on the CPU, before the GPU is held to
it bit for bit: the transform against a brute force and against scipy, the max_cells rule and both formats, the fixtures'
state counts, and that the laws a kernel must not follow give other states on the fixtures -- which is what makes the GPU's
equality mean something."""
import numpy as np
import pytest

import analytic_maps as am
import distance_field_fixtures as df
import ref_distance_field as rd

F = np.float32


def test_edt_equals_a_brute_force_over_all_seed_pairs():
    grid = df.unit_grid((9, 7, 5))
    rng = np.random.default_rng(4)
    for density in (0.02, 0.2):
        states = np.where(rng.random(rd.cells(grid)) < density, 3, rng.integers(0, 2, rd.cells(grid))).astype(np.uint8)
        for seeds in (1, 2, 3):
            for r in (0, 1, 3):
                assert np.array_equal(rd.edt(states, grid, seeds, r), rd.edt_brute(states, grid, seeds, r)), (density, seeds, r)
    none = np.ones(rd.cells(grid), np.uint8)
    assert (rd.edt(none, grid) == rd.FAR).all() and (rd.edt_brute(none, grid) == rd.FAR).all()


def scipy_d2(states, grid, seeds):
    ndi = pytest.importorskip("scipy.ndimage")
    seed = rd.seed_mask(states, seeds).reshape(grid.dims[::-1])
    if not seed.any():
        return np.full(rd.cells(grid), rd.FAR, np.int32)
    return np.rint(ndi.distance_transform_edt(~seed) ** 2).astype(np.int32).reshape(-1)


@pytest.mark.parametrize("name", "ABC")
def test_edt_equals_scipy_on_the_fixture_grids(name):
    for seeds in (1, 2, 3):
        assert np.array_equal(rd.edt(df.ramp_states(name), df.GRIDS[name], seeds), scipy_d2(df.ramp_states(name), df.GRIDS[name], seeds))


@pytest.mark.parametrize("dims,density", df.TRANSFORM_SHAPES)
def test_edt_equals_scipy_on_the_transform_shapes(dims, density):
    states, grid = df.random_states(dims, density), df.unit_grid(dims)
    assert np.array_equal(rd.edt(states, grid), scipy_d2(states, grid, 1))


def test_the_max_cells_rule_and_both_formats():
    dims = (65, 63, 17)
    states, grid = df.random_states(dims, 0.001), df.unit_grid(dims)
    full = rd.edt(states, grid)
    assert full.max() > 25 and full.max() < rd.FAR
    for r in (1, 5):
        d = rd.edt(states, grid, max_cells=r)
        assert (full == r * r).sum() > 0, "a cell at exactly R^2"
        assert np.array_equal(d, np.where(full > r * r, rd.FAR, full))
        assert (d == r * r).sum() == (full == r * r).sum()
    m = rd.to_metres(rd.edt(states, grid, max_cells=5), 3, F(0.005))
    assert m.dtype == F and np.isinf(m).sum() == (full > 25).sum()
    scale = F(3) * F(0.005)
    assert m[full == 25][0] == F(5) * scale and m[full == 2][0] == np.sqrt(F(2)) * scale and m[full == 0][0] == 0


def test_the_fixtures_have_the_recorded_counts():
    for name, (occupied, free, unknown) in df.COUNTS.items():
        s = df.ramp_states(name)
        assert ((s == 3).sum(), (s == 1).sum(), (s == 0).sum()) == (occupied, free, unknown), name
        assert ((s == 2).sum()) == 0
    assert df.ramp_distances("A").max() == df.LARGEST_D2_A
    # a map edge inside every grid and part of the maps outside it: each map alone leaves cells of the other unmarked
    for name in "ABC":
        both = df.ramp_states(name)
        for which in ((0,), (1,)):
            alone = df.ramp_states(name, which)
            assert ((alone | both) == both).all() and (alone != both).sum() > 100
        assert np.array_equal(df.ramp_states(name, (0,)) | df.ramp_states(name, (1,)), both)


# the near-saturated threshold: thr = -32767, the value every voxel deeper than mu behind the surface holds
DEEP = -0.0199999


def test_other_laws_give_other_states():
    """Each law a kernel must not follow differs from the law in at least 100 cells of grid A.  For `sdf < thr` that takes
    the threshold -32767 (occupied_below = -0.0199999): a stored sdf equals a threshold inside the band in a handful of
    voxels only (2 cells of grid A at the default), while -32767 is what every clamped voxel holds."""
    law = df.ramp_states("A")
    assert (df.ramp_states("A", rounding="nearest") != law).sum() >= 100
    assert (df.ramp_states("A", use_T=True) != law).sum() >= 100
    assert (df.ramp_states("A", gate="w_color") != law).sum() >= 100
    assert rd.threshold(DEEP, am.MU) == -32767
    deep = df.ramp_states("A", occupied_below=DEEP)
    assert (deep == 3).sum() >= 100 and (deep != law).sum() >= 100
    assert (df.ramp_states("A", occupied_below=DEEP, strict=True) != deep).sum() >= 100


def test_B_of_inverts_the_voxel_pose():
    maps = df.ramp_maps()
    for _, _, T in maps:
        B = rd.B_of(T, am.VS).astype(np.float64)
        Tm = np.asarray(T, F).astype(np.float64)
        Tv = np.concatenate([Tm[:3, :3], Tm[:3, 3:4] / float(F(am.VS))], axis=1)
        p = np.array([12.0, -7.0, 93.0])
        assert np.allclose(B[:, :3] @ (Tv[:, :3] @ p + Tv[:, 3]) + B[:, 3], p, atol=1e-3)
    I = rd.B_of(np.eye(4), am.VS)
    p = np.array([[3, -4, 5], [0, 0, 0], [-262144, 262143, 7]])
    assert np.array_equal(rd.transform(I, p), p.astype(F))
