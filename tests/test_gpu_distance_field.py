"""dslam_mark_occupancy, dslam_distance_transform and dslam_distance_field on the MI355X, everything
bit for bit against tests/ref_distance_field.py: the states of the fixture grids on the two posed ramp maps and on a fused
room, the transform on seeded random states at every shape at which its kernels take another path, the combined call, and
the argument checks."""
import numpy as np
import pytest

import analytic_maps as am
import distance_field_fixtures as df
import ref_distance_field as rd
import util
import weighted_fixtures as wf

pytestmark = pytest.mark.gpu

F = np.float32
I4 = np.eye(4, dtype=F)
DEEP = -0.0199999   # thr = -32767 (test_distance_field_ref.py)


def grid_of(pkg, g):
    return pkg.Grid.of(g.origin, g.cell, g.dims)


@pytest.fixture(scope="module")
def ramp(pkg, gpu):
    """(scenes, poses) of the two ramp spheres on the device."""
    maps = wf.ramp_spheres()
    scenes = []
    for pm in maps:
        scene = gpu.create_scene(pm.m.scene_params(pkg))
        am.upload(gpu, scene, pm.m)
        scenes.append(scene)
    return scenes, [np.asarray(pm.T, F) for pm in maps]


@pytest.fixture(scope="module")
def room(pkg, gpu, synth):
    """One fused s_tiny room under the identity: (scene, its resident (block_pos, voxels), voxel_size, mu, a grid of cell 2
    half as wide as its blocks' box about the median block, so that part of the map lies outside the grid)."""
    wl = synth.s_tiny()
    scene, _, _ = util.run_sequence(gpu, pkg, wl, util.small_params(pkg, wl), 5)
    pos, vox = rd.resident(gpu.download_hash_table(scene), gpu.download_voxel_blocks(scene))
    lo, hi = pos.min(axis=0) * 8, (pos.max(axis=0) + 1) * 8
    dims = np.clip((hi - lo) // 4, 8, 64)
    grid = rd.grid_of(np.median(pos, axis=0).astype(np.int64) * 8 + 3 - dims, 2, dims)
    return scene, (pos, vox), wl.scene_kwargs["voxel_size"], wl.scene_kwargs["mu"], grid


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def pattern(n, dtype=np.uint8):
    import torch
    t = torch.full((n * np.dtype(dtype).itemsize,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------------------------------------
# 1. marking
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", "ABC")
def test_states_of_the_ramp_maps_equal_the_reference(pkg, gpu, ramp, name):
    scenes, poses = ramp
    g = grid_of(pkg, df.GRIDS[name])
    both = gpu.mark_occupancy(scenes, poses, g)
    assert np.array_equal(both, df.ramp_states(name))
    # each map alone, both list orders (equal by the OR), an appended empty scene
    for i in (0, 1):
        assert np.array_equal(gpu.mark_occupancy([scenes[i]], [poses[i]], g), df.ramp_states(name, (i,))), i
    assert np.array_equal(gpu.mark_occupancy(scenes[::-1], poses[::-1], g), both)
    empty = gpu.create_scene(scenes[0].params)
    for order in ((0, 1, 2), (2, 0, 1), (0, 2, 1)):
        s, t = [(scenes + [empty])[k] for k in order], [(poses + [poses[0]])[k] for k in order]
        assert np.array_equal(gpu.mark_occupancy(s, t, g), both), order
    assert not gpu.mark_occupancy([empty], [I4], g).any()


def test_states_at_the_saturated_threshold_and_a_weight_gate(pkg, gpu, ramp):
    """occupied_below = -0.0199999 (thr = -32767, where `sdf <= thr` and `sdf < thr` part on every clamped voxel) and
    min_weight = 7 (between the texture's levels) on grid A."""
    scenes, poses = ramp
    g = grid_of(pkg, df.GRIDS["A"])
    assert np.array_equal(gpu.mark_occupancy(scenes, poses, g, occupied_below=DEEP), df.ramp_states("A", occupied_below=DEEP))
    gated = df.ramp_states("A", min_weight=7)
    assert (gated != df.ramp_states("A")).sum() >= 100 and (df.ramp_states("A", min_weight=8) != gated).sum() >= 100
    assert np.array_equal(gpu.mark_occupancy(scenes, poses, g, min_weight=7), gated)
    assert np.array_equal(gpu.mark_occupancy(scenes, poses, g, min_weight=1), df.ramp_states("A"))


def test_states_of_a_fused_room_equal_the_reference_of_its_download(pkg, gpu, room):
    scene, blocks, vs, mu, grid = room
    g = grid_of(pkg, grid)
    maps = [(blocks[0], blocks[1], I4)]
    # (at this map's mu = 4 voxels and cell = 2, +-0.005 m moves the threshold by a sixteenth of a voxel, which a cell of 8
    # voxels absorbs; half of mu either way does change cells, so those two are checked to differ)
    for kw in (dict(), dict(min_weight=3), dict(occupied_below=0.005), dict(occupied_below=-0.005), dict(occupied_below=0.04),
               dict(occupied_below=-0.04)):
        want = rd.mark(maps, grid, vs, mu, **kw)
        assert np.array_equal(gpu.mark_occupancy([scene], [I4], g, **kw), want), kw
        if not kw:
            assert min((want == 3).sum(), (want == 1).sum(), (want == 0).sum()) >= 100
            base = want
        elif "min_weight" in kw or abs(kw["occupied_below"]) > 0.01:
            assert (want != base).sum() > 0, kw


def test_a_grid_wholly_outside_the_maps_is_unknown(pkg, gpu, ramp):
    scenes, poses = ramp
    for origin in ((4000, 0, 0), (df.LO[0], df.LO[1], -2000), (-(1 << 20), -(1 << 20), -(1 << 20)), ((1 << 20) - 64, 0, 0)):
        out = np.full(32 * 17 * 9, 0xA5, np.uint8)
        gpu.mark_occupancy(scenes, poses, pkg.Grid.of(origin, 2, (32, 17, 9)), out=out)
        assert not out.any(), origin


def test_marking_host_form_equals_device_form(pkg, gpu, ramp):
    scenes, poses = ramp
    for name in "AB":
        g = grid_of(pkg, df.GRIDS[name])
        d_out = pattern(g.cells)
        gpu.mark_occupancy_device(scenes, poses, g, d_out.data_ptr())
        gpu.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), df.ramp_states(name))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the transform alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,density", df.TRANSFORM_SHAPES)
def test_transform_of_random_states_equals_the_reference(pkg, gpu, dims, density):
    states, grid = df.random_states(dims, density), df.unit_grid(dims)
    assert np.array_equal(gpu.distance_transform(grid_of(pkg, grid), states), rd.edt(states, grid))


def test_transform_without_a_seed_with_all_seeds_and_with_one_in_a_corner(pkg, gpu):
    dims = (65, 63, 17)
    grid, g = df.unit_grid(dims), grid_of(pkg, df.unit_grid(dims))
    n = rd.cells(grid)
    free = np.ones(n, np.uint8)
    assert (gpu.distance_transform(g, free) == pkg.DIST_FAR).all()
    assert np.isposinf(gpu.distance_transform(g, free, fmt=pkg.DIST_METRES, voxel_size=0.005)).all()
    assert not gpu.distance_transform(g, np.full(n, 3, np.uint8)).any()
    for corner in (0, n - 1, dims[0] - 1):
        one = free.copy()
        one[corner] = 3
        d = gpu.distance_transform(g, one)
        assert np.array_equal(d, rd.edt(one, grid)) and d.max() == 64 ** 2 + 62 ** 2 + 16 ** 2


@pytest.mark.parametrize("r", [1, 5])
def test_max_cells_keeps_a_cell_at_exactly_r_squared(pkg, gpu, r):
    dims = (65, 63, 17)
    states, grid = df.random_states(dims, 0.001), df.unit_grid(dims)
    full = rd.edt(states, grid)
    d = gpu.distance_transform(grid_of(pkg, grid), states, max_cells=r)
    assert np.array_equal(d, rd.edt(states, grid, max_cells=r))
    assert (d == r * r).sum() == (full == r * r).sum() > 0 and (d[full > r * r] == pkg.DIST_FAR).all()


@pytest.mark.parametrize("dims,density", [((65, 63, 17), 0.001), ((64, 64, 64), 0.5)])
def test_each_seeds_mode_and_both_formats(pkg, gpu, dims, density):
    states, grid = df.random_states(dims, density), df.unit_grid(dims, cell=3)
    g = grid_of(pkg, grid)
    for seeds in (pkg.SEED_OCCUPIED, pkg.SEED_UNKNOWN, pkg.SEED_OCCUPIED | pkg.SEED_UNKNOWN):
        want = rd.edt(states, grid, seeds)
        assert np.array_equal(gpu.distance_transform(g, states, seeds=seeds), want), seeds
        for r in (0, 5):
            m = gpu.distance_transform(g, states, seeds=seeds, max_cells=r, fmt=pkg.DIST_METRES, voxel_size=0.005)
            assert m.dtype == F
            assert np.array_equal(m.view(np.uint32), rd.to_metres(rd.edt(states, grid, seeds, r), 3, F(0.005)).view(np.uint32)), (seeds, r)


def test_transform_host_form_equals_device_form_and_scratch_is_reused(pkg, gpu):
    """The device form on the largest shape, then -- a second call on a smaller grid after a larger one -- both forms on a
    small one, whose results must not see what the larger call left in the engine's buffers."""
    big, small = ((64, 64, 64), 0.5), ((65, 63, 17), 0.001)
    for dims, density in (big, small, ((3, 1024, 2), 0.002), small):
        states, grid = df.random_states(dims, density), df.unit_grid(dims)
        g = grid_of(pkg, grid)
        want = rd.edt(states, grid)
        d_states, d_out = dev(states), pattern(g.cells, np.int32)
        gpu.distance_transform_device(g, d_states.data_ptr(), d_out.data_ptr())
        gpu.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.int32), want), dims
        assert np.array_equal(gpu.distance_transform(g, states), want), dims


# ---------------------------------------------------------------------------------------------------------------------
# 3. the combined call
# ---------------------------------------------------------------------------------------------------------------------
def test_distance_field_equals_mark_then_transform_and_the_reference(pkg, gpu, ramp):
    scenes, poses = ramp
    g = grid_of(pkg, df.GRIDS["A"])
    states, dist = gpu.distance_field(scenes, poses, g)
    apart_states = gpu.mark_occupancy(scenes, poses, g)
    assert np.array_equal(states, apart_states) and np.array_equal(dist, gpu.distance_transform(g, apart_states))
    assert np.array_equal(states, df.ramp_states("A")) and np.array_equal(dist, df.ramp_distances("A"))
    assert dist.max() == df.LARGEST_D2_A
    # either output alone carries the same bits
    only_states, none = gpu.distance_field(scenes, poses, g, want_dist=False)
    assert none is None and np.array_equal(only_states, states)
    none, only_dist = gpu.distance_field(scenes, poses, g, want_states=False)
    assert none is None and np.array_equal(only_dist, dist)
    # permuting the map list changes nothing
    s2, d2 = gpu.distance_field(scenes[::-1], poses[::-1], g)
    assert np.array_equal(s2, states) and np.array_equal(d2, dist)
    # the other seeds, a bound, metres
    for seeds, r in ((pkg.SEED_UNKNOWN, 0), (3, 4)):
        _, d = gpu.distance_field(scenes, poses, g, seeds=seeds, max_cells=r)
        assert np.array_equal(d, df.ramp_distances("A", seeds, r)), (seeds, r)
    _, m = gpu.distance_field(scenes, poses, g, fmt=pkg.DIST_METRES)
    assert np.array_equal(m.view(np.uint32), rd.to_metres(df.ramp_distances("A"), 2, F(am.VS)).view(np.uint32))


def test_distance_field_device_form(pkg, gpu, ramp):
    scenes, poses = ramp
    for name in "AC":
        g = grid_of(pkg, df.GRIDS[name])
        d_states, d_dist = pattern(g.cells), pattern(g.cells, np.int32)
        gpu.distance_field_device(scenes, poses, g, d_states.data_ptr(), d_dist.data_ptr())
        gpu.synchronize()
        assert np.array_equal(d_states.cpu().numpy(), df.ramp_states(name))
        assert np.array_equal(d_dist.cpu().numpy().view(np.int32), df.ramp_distances(name))
        # one output alone leaves the other array as it was
        d_states2, d_dist2 = pattern(g.cells), pattern(g.cells, np.int32)
        gpu.distance_field_device(scenes, poses, g, 0, d_dist2.data_ptr())
        gpu.distance_field_device(scenes, poses, g, d_states2.data_ptr(), 0)
        gpu.synchronize()
        assert np.array_equal(d_dist2.cpu().numpy(), d_dist.cpu().numpy()) and np.array_equal(d_states2.cpu().numpy(), d_states.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 4. arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_outputs_untouched(pkg, gpu, ramp):
    S, T = ramp
    G = pkg.Grid.of
    ok = G((0, 0, 0), 2, (8, 8, 8))
    n = ok.cells
    states_h, dist_h = np.full(1 << 12, 0xA5, np.uint8), np.full(1 << 12, 0xA5A5A5A5, np.uint32)
    d_states, d_dist = pattern(1 << 12), pattern(1 << 12, np.int32)
    sp, dp = d_states.data_ptr(), d_dist.data_ptr()
    in_states = np.ones(1 << 12, np.uint8)
    sheared = T[0].copy()
    sheared[0, 1] += 0.1
    other = pkg.open_engine(0)   # (lives as long as the session, as in test_gpu_register_graph.py)
    foreign = other.create_scene(S[0].params)
    mu = float(F(am.MU))
    bad_grids = [G((0, 0, 0), 0, (8, 8, 8)), G((0, 0, 0), 65, (8, 8, 8)), G((0, 0, 0), 1, (0, 8, 8)), G((0, 0, 0), 1, (8, 1025, 8)),
                 G((0, 0, 0), 1, (1024, 1024, 65)), G((-(1 << 20) - 1, 0, 0), 1, (8, 8, 8)), G((0, (1 << 20) - 15, 0), 2, (8, 8, 8)),
                 G((0, 0, 0), 2, (8, 8, 8), pad=1), G((0, 0, 0), 1, (8, 8, -1))]
    bad = [
        lambda: gpu.mark_occupancy([], np.zeros((0, 4, 4), F), ok, out=states_h),                        # the map-list errors
        lambda: gpu.mark_occupancy([S[0], S[0]], T, ok, out=states_h),
        lambda: gpu.mark_occupancy(S, [sheared, T[1]], ok, out=states_h),
        lambda: gpu.mark_occupancy([S[0], None], T, ok, out=states_h),
        lambda: gpu.mark_occupancy([S[0], foreign], T, ok, out=states_h),
        lambda: gpu.distance_field(S, [sheared, T[1]], ok, states_out=states_h, dist_out=dist_h),
        lambda: gpu.mark_occupancy(S, T, ok, min_weight=-1, out=states_h),                               # min_weight
        lambda: gpu.mark_occupancy(S, T, ok, min_weight=256, out=states_h),
        lambda: gpu.mark_occupancy_device(S, T, ok, sp, min_weight=256),
        lambda: gpu.mark_occupancy(S, T, ok, occupied_below=mu, out=states_h),                           # occupied_below
        lambda: gpu.mark_occupancy(S, T, ok, occupied_below=-mu, out=states_h),
        lambda: gpu.mark_occupancy(S, T, ok, occupied_below=float("nan"), out=states_h),
        lambda: gpu.distance_field(S, T, ok, occupied_below=float("inf"), states_out=states_h, dist_out=dist_h),
        lambda: gpu.distance_field_device(S, T, ok, sp, dp, occupied_below=0.03),
        lambda: gpu.distance_transform(ok, in_states, seeds=0, out=dist_h),                              # seeds
        lambda: gpu.distance_transform(ok, in_states, seeds=4, out=dist_h),
        lambda: gpu.distance_field(S, T, ok, seeds=4, states_out=states_h, dist_out=dist_h),
        lambda: gpu.distance_transform(ok, in_states, max_cells=-1, out=dist_h),                         # max_cells
        lambda: gpu.distance_transform(ok, in_states, max_cells=1775, out=dist_h),
        lambda: gpu.distance_field_device(S, T, ok, sp, dp, max_cells=1775),
        lambda: gpu.distance_transform(ok, in_states, fmt=2, out=dist_h),                                # format
        lambda: gpu.distance_transform(ok, in_states, fmt=-1, out=dist_h),
        lambda: gpu.distance_field(S, T, ok, fmt=2, states_out=states_h, dist_out=dist_h),
        lambda: gpu.distance_transform(ok, in_states, fmt=pkg.DIST_METRES, voxel_size=0.0, out=dist_h),
        lambda: gpu.distance_transform_device(ok, sp, dp, fmt=7),
        lambda: gpu.mark_occupancy_device(S, T, ok, 0),                                                  # a NULL array that is needed
        lambda: gpu.distance_transform(ok, None, out=dist_h),
        lambda: gpu.distance_transform_device(ok, 0, dp),
        lambda: gpu.distance_transform_device(ok, sp, 0),
        lambda: gpu.distance_field(S, T, ok, want_states=False, want_dist=False),
        lambda: gpu.distance_field_device(S, T, ok, 0, 0),
        lambda: gpu.mark_occupancy_device(S, T, ok, sp + 8),                                             # a misaligned device pointer
        lambda: gpu.distance_transform_device(ok, sp + 4, dp),
        lambda: gpu.distance_transform_device(ok, sp, dp + 4),
        lambda: gpu.distance_field_device(S, T, ok, sp + 1, dp),
        lambda: gpu.distance_field_device(S, T, ok, sp, dp + 8),
    ]
    for g in bad_grids:                                                                                  # a grid outside the limits
        bad += [lambda g=g: gpu.mark_occupancy(S, T, g, out=states_h), lambda g=g: gpu.distance_transform(g, in_states, out=dist_h),
                lambda g=g: gpu.distance_field_device(S, T, g, sp, dp)]
    for i, call in enumerate(bad):
        with pytest.raises(pkg.DslamError, match="status -1"):
            call()
        assert (states_h == 0xA5).all() and (dist_h == 0xA5A5A5A5).all(), i
    gpu.synchronize()
    assert (d_states.cpu().numpy() == 0xA5).all() and (d_dist.cpu().numpy() == 0xA5).all()
    # the largest values that are allowed
    assert gpu.distance_transform(ok, in_states[:n], max_cells=pkg.DIST_MAX_CELLS).shape == (n,)
    assert gpu.mark_occupancy(S, T, ok, min_weight=255, occupied_below=float(np.nextafter(F(mu), F(0)))).shape == (n,)
