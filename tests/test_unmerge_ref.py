"""ref_unmerge.py alone, on the analytic pairs of register_fixtures.py and the weighted planes of weighted_fixtures.py: the
sequential restatement of dslam_unmerge_maps' law has the properties the law promises, and the
round trip merge -> unmerge stays within the bound ref_unmerge.py derives, with no voxel excluded.  No GPU."""
import numpy as np
import pytest

import analytic_maps as am
import ref_merge as rm
import ref_unmerge as ru
import register_fixtures as fx
import unmerge_fixtures as uf

I4 = fx.I4
PAIRS = {"box": lambda: fx.box_pair("small"), "holes": fx.holes_pair, "negative": fx.negative_pair}


def round_trip(what, src, dst, X, with_colour=1):
    before = dst.copy()
    merged = dst.copy()
    mres = rm.merge(src, merged, X, with_colour=with_colour)
    assert mres["exhausted"] == 0 and merged.vba["w_depth"].max() < merged.max_w, f"{what}: the merge clamped"
    after = merged.copy()
    ures = ru.unmerge(src, after, X, with_colour=with_colour)
    for k in ("src_blocks", "blocks_touched", "src_candidates", "out_of_range", "voxels_changed"):
        assert ures[k] == mres[k], (what, k, ures, mres)
    assert ures["candidates_without_block"] == ures["depth_underweight"] == ures["colour_underweight"] == 0, ures
    figures = ru.check_round_trip(what, src, before, merged, after, X, with_colour)
    print(f"{what}: merge {mres}\n  unmerge {ures}\n  round trip {figures}")
    return mres, ures, figures


@pytest.mark.parametrize("ws,W0,want", [(1, 1, 3), (3, 5, 2), (7, 2, 5), (40, 3, 15)])
def test_round_trip_on_the_box_pair_with_uniform_weights(ws, W0, want):
    assert ru.depth_bound(W0, ws) == want
    pair = fx.box_pair("small")
    src, dst = uf.uniform(rm.State.of_map(pair.src_map), ws), uf.uniform(rm.State.of_map(pair.dst_map), W0)
    mres, ures, fig = round_trip(f"box, ws {ws}, W0 {W0}", src, dst, pair.X_true.astype(np.float32))
    assert mres["src_blocks"] == 268 and mres["blocks_touched"] == 448 and mres["blocks_allocated"] == 124
    assert fig["worst_sdf"] <= want and fig["observed"] > 50000 and fig["created"] > 200


@pytest.mark.parametrize("kind", ["holes", "negative"])
def test_round_trip_on_the_holes_and_negative_pairs(kind):
    pair = PAIRS[kind]()
    mres, ures, fig = round_trip(kind, rm.State.of_map(pair.src_map), rm.State.of_map(pair.dst_map), pair.X_true.astype(np.float32))
    assert mres["blocks_allocated"] > 100 and fig["observed"] > 10000 and fig["created"] > 200


@pytest.mark.parametrize("with_colour", [1, 0])
@pytest.mark.parametrize("how", ["identity", "off_lattice"])
@pytest.mark.parametrize("onto", ["plain", "coloured"])
def test_round_trip_with_weights_that_vary_per_voxel(onto, how, with_colour):
    src, dst, twin = uf.unclamped_planes()
    X = I4 if how == "identity" else fx.off_lattice(1.5, 0.45)
    target = dst if onto == "plain" else twin
    mres, ures, fig = round_trip(f"weighted planes onto the {onto} map, {how}, with_colour {with_colour}", src, target.copy(), X,
                                 with_colour)
    assert fig["observed"] > 10000
    if onto == "coloured" and with_colour:
        assert fig["coloured"] > 10000


def test_after_a_clamp_the_law_holds_and_the_round_trip_is_not_exact():
    src, dst = uf.plane_maps()
    merged = dst.copy()
    rm.merge(src, merged, I4)
    assert merged.vba["w_depth"].max() == 100                 # 99 + 3 clamped
    after = merged.copy()
    ures = ru.unmerge(src, after, I4)
    live = merged.live()
    ptrs = merged.hash["ptr"][live]
    reader = rm.SourceReader(src)
    clamped = 0
    for entry, ptr in zip(live, ptrs):
        P = merged.hash["pos"][entry].astype(np.int64)[None] * 8 + rm.LOCAL
        ws = reader.read(P)["w_depth"].astype(np.int64)
        W = merged.vba[ptr]["w_depth"].astype(np.int64)
        assert np.array_equal(after.vba[ptr]["w_depth"], W - ws)          # the law: what is held minus what is taken
        hit = (dst.vba[ptr]["w_depth"] == 99) & (ws == 3)
        assert (after.vba[ptr]["w_depth"][hit] == 97).all()               # ... which is not what was there
        clamped += int(hit.sum())
    assert clamped > 1000 and ures["depth_underweight"] == 0


def test_remerge_is_unmerge_then_merge_and_idles_on_equal_transforms():
    pair = fx.box_pair("small")
    src, dst = rm.State.of_map(pair.src_map), rm.State.of_map(pair.dst_map)
    X_new = pair.X_true.astype(np.float32)
    X_old = (pair.X_true @ fx.off_lattice().astype(np.float64)).astype(np.float32)
    merged = dst.copy()
    rm.merge(src, merged, X_old)
    one, two = merged.copy(), merged.copy()
    un, re = ru.remerge(src, one, X_old, X_new)
    un2 = ru.unmerge(src, two, X_old)
    re2 = rm.merge(src, two, X_new)
    assert not one.differences(two) and un == un2 and re == re2
    assert un["voxels_changed"] > 50000 and re["voxels_changed"] > 50000 and re["blocks_allocated"] > 0
    idle = merged.copy()
    un, re = ru.remerge(src, idle, X_old, X_old.copy())
    assert not idle.differences(merged) and un == ru.ZERO_UNMERGE and re == ru.ZERO_MERGE


def test_without_a_merge_a_lighter_destination_is_left_alone_and_counted():
    pair = fx.box_pair("small")
    src, dst = uf.uniform(rm.State.of_map(pair.src_map), 5), uf.uniform(rm.State.of_map(pair.dst_map), 2)
    after = dst.copy()
    res = ru.unmerge(src, after, pair.X_true.astype(np.float32))
    assert not after.differences(dst) and res["voxels_changed"] == 0
    assert res["depth_underweight"] > 50000 and res["candidates_without_block"] > 1000 and res["blocks_touched"] == 448 - 124


def test_uncombine_inverts_combine_on_chosen_voxels():
    """A handful of voxels by hand: the branches of both halves."""
    v = np.zeros(6, am.VOXEL_DTYPE)
    s = np.zeros(6, am.VOXEL_DTYPE)
    v["sdf"], v["w_depth"], v["clr"], v["w_color"] = [1000, 1000, 1000, -32767, 500, 32767], [4, 3, 2, 9, 4, 0], 90, [4, 3, 2, 9, 0, 0]
    s["sdf"], s["w_depth"], s["clr"], s["w_color"] = [2000, 2000, 2000, 32767, 700, 100], [3, 3, 3, 1, 0, 2], 30, [3, 3, 3, 1, 2, 0]
    out, under_d, under_c = ru.uncombine(s, v)
    assert (under_d, under_c) == (2, 2)                                      # voxels 2 and 5; voxels 2 and 4
    assert out[2].tobytes() == v[2].tobytes() and out[5].tobytes() == v[5].tobytes() and out[4].tobytes() == v[4].tobytes()
    # rem = 1: (4 * 1000 - 3 * 2000) / 1 = -2000 to within the truncations; colour (4 * 90 - 3 * 30) / 1 = 270 -> clamped
    assert out[0]["w_depth"] == 1 and abs(int(out[0]["sdf"]) + 2000) <= 1 and out[0]["w_color"] == 1 and (out[0]["clr"] == 255).all()
    # rem = 0: empty depth half, zero colour half
    assert out[1]["w_depth"] == 0 and out[1]["sdf"] == 32767 and out[1]["w_color"] == 0 and not out[1]["clr"].any()
    # the clamp at -1: (9 * -1 - 1 * 1) / 8 < -1
    assert out[3]["w_depth"] == 8 and out[3]["sdf"] == -32767
