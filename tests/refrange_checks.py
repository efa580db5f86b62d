"""Check bodies of the range-image tests: an engine's visible list and range image against the law of ref_range.py, for
every producer of the projections -- the separate calls (FindVisibleBlocks, then CreateExpectedDepths' own projection
launch), GetImage's selection that projects as it lists, and the front end GetImage adopts from ProcessFrame.  They take
an `api` (the HIP engine or the CPU oracle) and are run by test_oracle_range_image.py and test_gpu_range_image.py.

What is compared, each time: the list equals the reference's once the visibility ties are taken out of both, it is
ascending and holds no entry without a voxel block; the corner of the range image is bit-equal, as float32, to the
reference off the tie cells, and a cell no accepted box covers holds exactly (FAR_AWAY, VERY_CLOSE)."""
import numpy as np

import range_fixtures as rf
import ref_range as rr
import util

DEFAULT_BUDGET = 65536 * 4


def is_hip(api):
    return api.has("debug_front_end_counts")


def compare_list(api, scene, rs, ref, table, what):
    ids = api.download_visible_ids(rs)
    assert api.stats(scene, rs)["no_visible_entries"] == len(ids), what
    assert (np.diff(ids) > 0).all(), f"{what}: the list is not ascending"
    assert (table["ptr"][ids] >= 0).all(), f"{what}: an entry without a voxel block is listed"
    got, want = (a[~np.isin(a, ref.vis_tie_ids)] for a in (ids, ref.ids))
    assert np.array_equal(got, want), (f"{what}: {len(got)} listed, {len(want)} expected; first difference at "
                                        f"{_first_difference(got, want)}")
    return ids


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(a[:n] != b[:n])[0]
    return int(d[0]) if len(d) else n


def compare_range(api, rs, ref, what):
    got = api.download_range_image(rs)[:ref.ch, :ref.cw]
    assert got.dtype == np.float32
    ok = ~ref.tie_cells
    empty = ok & (ref.image[..., 0] == rr.FAR_AWAY)
    assert (got[empty] == np.array([rr.FAR_AWAY, rr.VERY_CLOSE])).all(), \
        f"{what}: {int((got[empty] != np.array([rr.FAR_AWAY, rr.VERY_CLOSE])).any(-1).sum())} of {int(empty.sum())} uncovered cells are not (FAR_AWAY, VERY_CLOSE)"
    bad = ok & (got.view(np.uint32) != ref.image.view(np.uint32)).any(-1)
    if bad.any():
        y, x = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {int(ok.sum())} cells differ; cell ({x}, {y}) holds {got[y, x]}, "
                             f"the law says {ref.image[y, x]}")


def check_count_windows(api, scene, rs, ids, table, n_local):
    """CountVisibleBlocks against the engine's own list: no tie rule needed."""
    ptr = table["ptr"][ids].astype(np.int64)
    lo, hi = (int(v) for v in np.quantile(ptr, [0.3, 0.7]))
    windows = [(5, 4), (0, n_local - 1), (lo, hi), (hi, hi)]
    for a, b in windows:
        want = int(((ptr >= a) & (ptr <= b)).sum())
        assert api.count_visible_blocks(scene, rs, a, b) == want, (a, b, want)
    assert 0 < ((ptr >= lo) & (ptr <= hi)).sum() < len(ptr)


def _scene(api, pkg, case):
    scene = api.create_scene(case.params(pkg))
    case.upload(api, scene)
    return scene


def check_separate_calls(api, pkg, case):
    """FindVisibleBlocks, CountVisibleBlocks, CreateExpectedDepths; then another pose and the first one again on the same
    render state, so that a range image that is not reset would show."""
    scene = _scene(api, pkg, case)
    rs = api.create_render_state(scene, case.W, case.H)
    for k, (M, ref) in enumerate(((case.M, case.ref), (case.M_other, case.ref_other), (case.M, case.ref))):
        what = f"{case.name}, separate calls, run {k}"
        api.find_visible_blocks(scene, rs, M, case.intr)
        ids = compare_list(api, scene, rs, ref, case.table, what)
        if k == 0:
            check_count_windows(api, scene, rs, ids, case.table, case.m.num_local_blocks)
        api.create_expected_depths(scene, rs, M, case.intr)
        compare_range(api, rs, ref, what)


def check_get_image(api, pkg, case):
    """GetImage into a fresh free render state: the selection projects as it lists.  Nothing was fused, so the HIP engine
    has no front end to adopt."""
    scene = _scene(api, pkg, case)
    free = api.create_render_state(scene, case.W, case.H)
    before = api.debug_front_end_counts() if is_hip(api) else None
    for k, (M, ref) in enumerate(((case.M, case.ref), (case.M_other, case.ref_other), (case.M, case.ref))):
        what = f"{case.name}, GetImage, run {k}"
        api.get_image(scene, free, M, case.intr, pkg.IMAGE_DEPTH)
        compare_list(api, scene, free, ref, case.table, what)
        compare_range(api, free, ref, what)
    if before is not None:
        assert api.debug_front_end_counts()[1] == before[1], "a front end was adopted where none was computed"


def check_budget(api, pkg, which, kind):
    """The render-tile budget through the debug hook, by both call sequences."""
    case, budget, ref = rf.budget(which, kind)
    scene = _scene(api, pkg, case)
    rs = api.create_render_state(scene, case.W, case.H)
    free = api.create_render_state(scene, case.W, case.H)
    api.debug_set_render_tile_budget(budget)
    try:
        what = f"{case.name}, budget {kind} = {budget}, separate calls"
        api.find_visible_blocks(scene, rs, case.M, case.intr)
        compare_list(api, scene, rs, ref, case.table, what)
        api.create_expected_depths(scene, rs, case.M, case.intr)
        compare_range(api, rs, ref, what)
        what = f"{case.name}, budget {kind} = {budget}, GetImage"
        api.get_image(scene, free, case.M, case.intr, pkg.IMAGE_DEPTH)
        compare_list(api, scene, free, ref, case.table, what)
        compare_range(api, free, ref, what)
    finally:
        api.debug_set_render_tile_budget(DEFAULT_BUDGET)


def check_fused(api, pkg, synth):
    """Four frames through ProcessFrame, then GetImage at the last frame's pose, intrinsics and size: on the HIP engine the
    front end the fusion launch computed is adopted.  The reference reads the table downloaded after the last ProcessFrame.
    Returns the reference (reach and tie shares are asserted here, from it alone)."""
    wl = synth.s_tiny()
    scene = api.create_scene(util.small_params(pkg, wl))
    rs, view = api.create_render_state(scene, wl.W, wl.H), api.create_view(wl.W, wl.H)
    free = api.create_render_state(scene, wl.W, wl.H)
    for i in range(4):
        rgba, mm, M = wl.frame(i)
        api.view_update(view, rgba, mm, timestamp=float(i))
        api.process_frame(scene, view, rs, M, wl.intr)
    table = api.download_hash_table(scene)
    ref = rr.RangeLaw(table, M, wl.intr, scene.params.voxel_size, wl.W, wl.H)
    blocks, cells = ref.tie_shares()
    print(f"fused: {len(ref.ids)} listed, {ref.n_tie_blocks} tie blocks, tie cells {cells:.2%}")
    assert len(ref.ids) >= 100 and (ref.image[..., 0] != rr.FAR_AWAY).sum() >= 20
    assert blocks <= rf.TIE_BLOCKS and cells <= rf.TIE_CELLS, (ref.n_tie_blocks, len(ref.ids), cells)
    before = api.debug_front_end_counts() if is_hip(api) else None
    api.get_image(scene, free, M, wl.intr, pkg.IMAGE_DEPTH)
    if before is not None:
        assert api.debug_front_end_counts()[1] == before[1] + 1, "GetImage did not adopt the fusion launch's front end"
    compare_list(api, scene, free, ref, table, "fused")
    compare_range(api, free, ref, "fused")
    return ref
