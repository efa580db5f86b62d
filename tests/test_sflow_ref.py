"""tests/ref_sflow.py against libviso2's own output (tests/golden/sflow_*.npz, written by tests/golden/make_sflow_golden.py
from the reference's unmodified sources): the eight feature arrays, the raw matches, the dense-set subset law.  Also the
conditions that keep those comparisons from being vacuous, and the crafted cases for the law's corners.  No GPU."""
import numpy as np
import pytest

import ref_sflow as rf
import sflow_fixtures as sf

SETS = sf.SETS
RAW_CASES = [n for n, c in sf.CASES.items() if not c[7]]


def true_displacement(name, m):
    W, H, half, d, (mx, my), method, seed, dense = sf.CASES[name]
    return ((m[:, 0] - m[:, 3] == d) & (m[:, 6] - m[:, 9] == d) & (m[:, 1] == m[:, 4]) & (m[:, 7] == m[:, 10]) &
            (m[:, 6] - m[:, 0] == mx) & (m[:, 7] - m[:, 1] == my))


@pytest.mark.parametrize("name", list(sf.CASES))
def test_the_fixture_inputs_are_the_seeded_frames(name):
    g, f = sf.golden(name), sf.case_frames(name)
    for k in sf.IMAGES:
        assert np.array_equal(g["img_" + k], f[k]), k
        assert g["img_" + k].shape == (sf.CASES[name][1], sf.CASES[name][0]) and g["img_" + k].shape[1] <= 320


@pytest.mark.parametrize("name", list(sf.CASES))
def test_features_equal_the_library(name):
    g, r = sf.golden(name), sf.reference(name)
    seen = 0
    for key, (image, which) in SETS.items():
        if key in g:
            assert g[key].dtype == np.int32 and np.array_equal(g[key], r["features"][(image, which)]), key
            seen += len(g[key])
    assert seen > 0


@pytest.mark.parametrize("name", RAW_CASES)
def test_raw_matches_equal_the_library(name):
    g, r = sf.golden(name), sf.reference(name)
    assert np.array_equal(g["raw_matches"], r["matches"][(int(g["method"]), 0)])


def test_dense_matches_of_the_library_are_a_subset():
    g, r = sf.golden("dense_160x96"), sf.reference("dense_160x96")
    ours = set(map(tuple, r["matches"][(2, 1)].tolist()))
    assert len(g["matches"]) >= 300
    assert all(tuple(m) in ours for m in g["matches"].tolist())
    assert len(ours) == len(r["matches"][(2, 1)])     # no record twice


def test_the_fixtures_are_not_vacuous():
    for name in RAW_CASES:
        W, H, half, d, motion, method, seed, dense = sf.CASES[name]
        m = sf.golden(name)["raw_matches"]
        if W < 96:
            assert len(m) == 0, name                      # too small for a sparse circle: the empty result is the case
            continue
        assert len(m) >= (50 if (W, H, method) == (160, 96, 2) else 10), name
        if method == 2:
            assert true_displacement(name, m).sum() * 4 >= 3 * len(m), name
    flow, stereo = sf.golden("flow_160x96")["raw_matches"], sf.golden("stereo_160x96")["raw_matches"]
    assert ((flow[:, 6] - flow[:, 0] == 3) & (flow[:, 7] - flow[:, 1] == 2)).sum() * 4 >= 3 * len(flow)
    assert ((stereo[:, 6] - stereo[:, 9] == 7) & (stereo[:, 7] == stereo[:, 10])).sum() * 4 >= 3 * len(stereo)
    assert (flow[:, 3:6] == -1).all() and (flow[:, 9:] == -1).all() and (stereo[:, :6] == -1).all()


def test_filter_bounds_hold_at_the_extremes():
    """The int16 argument of the header, on the images that reach the bounds."""
    edge = np.zeros((16, 16), np.int32)
    edge[:, :8] = 255
    du, dv, f1, f2 = rf.filters(edge)
    top = 128 + (rf.SOBEL_BOUND >> 7)
    assert du[8, 8] == top and du[8, 3] == 128 and (dv[2:-2, 2:-2] == 128).all()       # left minus right, at the bound
    assert rf.filters(edge.T.copy())[1][8, 8] == top                                 # top minus bottom
    assert rf.filters(255 - edge)[0][8, 8] == 128 + (-rf.SOBEL_BOUND >> 7)            # an arithmetic shift: floor
    dot = np.zeros((16, 16), np.int32)
    dot[8, 8] = 255
    f1 = rf.filters(dot)[2]
    assert f1[8, 8] == 8 * 255 and f1[7, 7] == 255 and f1[6, 6] == -255 and f1[5, 5] == 0   # centred: no displacement
    quad = np.zeros((16, 16), np.int32)
    quad[:8, :8] = quad[8:, 8:] = 255
    assert rf.filters(quad)[3][8, 8] == rf.CHECKER_BOUND and rf.filters(255 - quad)[3][8, 8] == -rf.CHECKER_BOUND
    assert rf.SOBEL_BOUND == 3 * 16 * 255 and rf.CHECKER_BOUND == 8 * 255 and rf.MAX_COST == 32 * 255


def test_cells_and_sets():
    assert [rf.sparse_n(n) for n in (1, 3, 4, 10, 12)] == [3, 9, 10, 10, 12]
    # a cell exists while its start is below size - n - 9: it may end on size - 10
    assert rf.cells_along(25, 3) == 1 and rf.cells_along(24, 3) == 0 and rf.cells_along(29, 3) == 2 and rf.cells_along(28, 3) == 1
    for size in range(1, 80):
        for n in (1, 3, 9):
            assert rf.cells_along(size, n) == len(range(n + 9, size - n - 9, n + 1))


def test_parameter_encoding():
    assert rf.resolve({}) == rf.DEFAULTS
    assert rf.resolve(rf.encode(half_resolution=0))["half_resolution"] == 0
    assert rf.resolve(dict(nms_n=0, channels=4)) == dict(rf.DEFAULTS, channels=4)
    for bad in (dict(nms_n=-1), dict(nms_n=33), dict(nms_tau=-5), dict(match_binsize=-1), dict(match_radius=-1), dict(match_disp_tolerance=-1),
                dict(half_resolution=2), dict(channels=3)):
        with pytest.raises(ValueError):
            rf.resolve(bad)
    with pytest.raises(ValueError):
        rf.check_size(4096, 4096, rf.resolve(dict(match_binsize=1)))
    with pytest.raises(ValueError):
        rf.check_size(1, 8, rf.resolve({}))


# ---------------------------------------------------------------------------------------------------------------------
# the crafted cases put on the table what they say they do
# ---------------------------------------------------------------------------------------------------------------------
def positions(rec):
    return [(r[0], r[1], r[3]) for r in rec.tolist()]


def test_plateau_the_first_in_the_scan_wins():
    c, r = sf.crafted_reference("plateau")
    f1 = r["filters"][0][rf.FILTER_F1]
    assert f1[18, 17] == f1[16, 19] == f1[16:20, 16:20].max()
    have = positions(r["features"][(rf.IMAGE_1C, 1)])
    assert (17, 18, 1) in have and (19, 16, 1) not in have


def test_clamped_hood_decides():
    c, r = sf.crafted_reference("clamped_hood")
    f1 = r["filters"][0][rf.FILTER_F1]
    assert f1[20, 57] > f1[20, 55] and 57 <= 55 + 3 and 57 > c["W"] - 10
    assert (55, 20, 1) in positions(r["features"][(rf.IMAGE_1C, 1)])


def test_tie_the_bin_walk_decides_not_the_index():
    c, r = sf.crafted_reference("tie")
    prev = r["features"][(rf.IMAGE_1P, 1)]
    assert positions(prev) == [(20, 60, 1), (30, 30, 1)]
    assert np.array_equal(prev[0, 4:], prev[1, 4:])                 # equal descriptors: equal costs
    m = r["matches"][(0, 1)]
    assert m.tolist() == [[30, 30, 1, -1, -1, -1, 25, 45, 0, -1, -1, -1]]


def test_no_candidate_answers_feature_zero():
    c, r = sf.crafted_reference("lonely_closes")
    assert positions(r["features"][(rf.IMAGE_1P, 1)]) == [(40, 30, 0)]
    assert all(positions(r["features"][(i, 1)]) == [(30, 30, 1)] for i in (rf.IMAGE_2P, rf.IMAGE_1C, rf.IMAGE_2C))
    assert r["matches"][(2, 1)].tolist() == [[40, 30, 0, 30, 30, 0, 30, 30, 0, 30, 30, 0]]     # closed through feature 0
    c, r = sf.crafted_reference("lonely_open")
    assert positions(r["features"][(rf.IMAGE_1P, 1)]) == [(20, 30, 1), (40, 30, 0)]
    assert len(r["matches"][(2, 1)]) == 0


@pytest.mark.parametrize("name", ["two_classes_flow", "two_classes_stereo"])
def test_one_match_per_pixel(name):
    c, r = sf.crafted_reference(name)
    cur = r["features"][(rf.IMAGE_1C, 1)]
    on_pixel = [k for k, f in enumerate(cur.tolist()) if (f[0], f[1]) == (20, 20)]
    assert len(on_pixel) == 2 and sorted(cur[on_pixel, 3].tolist()) == [1, 3]
    m = r["matches"][(c["method"], 1)]
    assert on_pixel[0] in m[:, 8] and on_pixel[1] not in m[:, 8]
    assert len(m) == len(cur) - 1                                     # everything else matches itself
