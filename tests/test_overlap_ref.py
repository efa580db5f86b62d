"""The references of the overlap survey and the pair selection (ref_overlap.py) checked on the CPU:
the survey against counts that follow from set operations on block coordinates (no transform arithmetic), the selection
against brute-force properties on random count matrices, and the default threshold against the pairs the joint
registration's fixtures report as active."""
import ctypes
import re
from fractions import Fraction

import numpy as np
import pytest

import overlap_fixtures as of
import ref_overlap as ro
import register_fixtures as fx
import register_graph_fixtures as gf


# ---------------------------------------------------------------------------------------------------------------------
# the survey
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of.set_cases(), ids=lambda c: c.name)
def test_survey_reference_against_set_arithmetic(case):
    tables = [ro.Table.of_map(m) for m in case.maps]
    live, blocks, octants = ro.survey(tables, case.T, of.VS_EXACT)
    ab_blocks, ab_octants, ba_blocks, ba_octants = case.want
    print(f"{case.name}: live {live.tolist()}, blocks {blocks.tolist()}, octants {octants.tolist()}; set arithmetic {case.want}")
    assert live.tolist() == [len(m.block_pos) for m in case.maps]
    assert (blocks[0, 1], octants[0, 1], blocks[1, 0], octants[1, 0]) == (ab_blocks, ab_octants, ba_blocks, ba_octants)
    assert blocks[0, 0] == live[0] and octants[1, 1] == 8 * live[1]
    assert 0 < ab_blocks < live[0] and 0 < ba_blocks < live[1]       # (neither nothing nor everything)
    # the chain walk is part of the lookup: both tables keep blocks in their excess areas
    assert all((t.table["ptr"][t.num_buckets:] >= 0).any() for t in tables)


def test_lookup_follows_the_chain_and_skips_what_is_not_resident():
    m = of.set_cases()[0].maps[0]
    t = ro.Table.of_map(m)
    assert t.holds(m.block_pos).all() and not t.holds(m.block_pos + np.array([100, 0, 0])).any()
    in_excess = np.flatnonzero(t.table["ptr"][t.num_buckets:] >= 0) + t.num_buckets
    swapped = t.table.copy()
    swapped["ptr"][in_excess[:3]] = -1
    heads = np.flatnonzero(swapped["ptr"][:t.num_buckets] >= 0)[:3]
    swapped["ptr"][heads] = -1
    gone = np.concatenate([in_excess[:3], heads])
    t2 = ro.Table(swapped, t.num_buckets)
    held = t2.holds(t.table["pos"][t.table["ptr"] >= 0].astype(np.int64))
    assert held.sum() == len(m.block_pos) - 6 and len(t2.resident_blocks()) == len(m.block_pos) - 6
    assert not t2.holds(t.table["pos"][gone].astype(np.int64)).any()


def test_a_position_no_int_holds_is_not_shared():
    a, b = of.set_cases()[1].maps
    T = np.stack([np.eye(4, dtype=np.float32)] * 2)
    T[1, 0, 3] = 3.0e7 * of.VS_EXACT      # 3e7 voxels: q.x is past 2^31 / 8 blocks but within an int
    live, blocks, octants = ro.survey([ro.Table.of_map(a), ro.Table.of_map(b)], T, of.VS_EXACT)
    assert octants[0, 1] == octants[1, 0] == 0 and blocks[0, 1] == 0
    T[1, 0, 3] = 1.0e12 * of.VS_EXACT     # past every int
    live, blocks, octants = ro.survey([ro.Table.of_map(a), ro.Table.of_map(b)], T, of.VS_EXACT)
    assert octants[0, 1] == octants[1, 0] == 0 and octants[0, 0] == 8 * live[0]


# ---------------------------------------------------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------------------------------------------------
def _components_by_search(n, edges):
    comp = [-1] * n
    for root in range(n):
        if comp[root] >= 0:
            continue
        comp[root] = root
        stack = [root]
        while stack:
            m = stack.pop()
            for s, d in edges:
                other = d if s == m else (s if d == m else -1)
                if other >= 0 and comp[other] < 0:
                    comp[other] = root
                    stack.append(other)
    return comp


def check_selection(live, shared, params, pairs, component, result, pass1=None):
    """The brute-force properties of one selection (also used on the library's output by the GPU file)."""
    n = len(live)
    min_shared = params["min_shared_octants"] or 64
    max_pairs = params["max_pairs"] or 128
    qualifying = [(s, d) for s in range(n) for d in range(n) if s != d and shared[s][d] >= min_shared]
    # components: a plain graph search
    want = _components_by_search(n, qualifying)
    assert list(component) == want and result["num_components"] == len(set(want))
    # the one-direction choice, by exact fractions
    kept = []
    for s, d in qualifying:
        if params["one_direction"] and (d, s) in qualifying:
            mine, other = Fraction(shared[s][d], 8 * live[s]), Fraction(shared[d][s], 8 * live[d])
            if mine < other or (mine == other and s > d):
                continue
        kept.append((s, d))
    assert result["qualifying"] == len(kept)
    pairs = [tuple(int(v) for v in p) for p in pairs]
    assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs) and set(pairs) <= set(kept)
    assert result["selected"] == len(pairs) == min(len(kept), max_pairs)
    # the selected pairs span every component
    assert _components_by_search(n, pairs) == want
    # no pair left out outranks a pair that is in without being needed for the span: take the spanning pairs out greedily by
    # rank (the law's pass 1) and compare ranks
    rank = lambda p: (-shared[p[0]][p[1]], p[0], p[1])
    if pass1 is None:
        sets, pass1 = list(range(n)), []
        for s, d in sorted(kept, key=rank):
            if sets[s] != sets[d]:
                gone = sets[d]
                sets = [sets[s] if v == gone else v for v in sets]
                pass1.append((s, d))
    assert set(pass1) <= set(pairs)
    pass2 = [p for p in pairs if p not in pass1]
    left_out = [p for p in kept if p not in pairs]
    if pass2 and left_out:
        assert max(rank(p) for p in pass2) < min(rank(p) for p in left_out)
    return len(left_out)


def test_selection_reference_on_random_matrices():
    capped = spanning_only = one_dir = several = 0
    for live, shared, params in of.selection_cases():
        pairs, component, result, pass1 = ro.select(live, shared, **params)
        left = check_selection(live, shared, params, pairs, component, result, pass1)
        capped += left > 0
        spanning_only += left > 0 and params["max_pairs"] == len(live) - 1
        one_dir += bool(params["one_direction"]) and result["qualifying"] > 0
        several += result["num_components"] > 1
    print(f"{len(of.selection_cases())} matrices: the cap binds in {capped} ({spanning_only} at max_pairs = N - 1), one "
          f"direction in {one_dir}, more than one component in {several}")
    assert len(of.selection_cases()) >= 200 and capped >= 20 and spanning_only >= 5 and one_dir >= 40 and several >= 40


def test_selection_on_crafted_matrices():
    # a chain 0 - 1 - 2 whose weakest link must survive the smallest cap; 3 alone
    live = [10, 10, 10, 10]
    shared = [[80, 70, 0, 0], [75, 80, 64, 0], [0, 66, 80, 63], [0, 0, 0, 80]]
    pairs, comp, res, _ = ro.select(live, shared, max_pairs=3)
    assert comp == [0, 0, 0, 3] and res == dict(qualifying=4, selected=3, num_components=2)
    assert pairs == [(0, 1), (1, 0), (2, 1)]          # (2, 1) with 66 joins map 2; (1, 2) with 64 is what the cap drops
    pairs, _, res, _ = ro.select(live, shared, one_direction=1)
    assert pairs == [(1, 0), (2, 1)] and res["qualifying"] == 2
    # coverage, not the count, decides the direction: 100 of 8 x 100 against 90 of 8 x 20; a tie keeps (a, b)
    pairs, _, _, _ = ro.select([100, 20], [[800, 100], [90, 160]], one_direction=1)
    assert pairs == [(1, 0)]
    pairs, _, _, _ = ro.select([100, 20], [[800, 500], [100, 160]], one_direction=1)
    assert pairs == [(0, 1)]
    # the default threshold
    assert ro.select([10, 10], [[80, 63], [63, 80]])[0] == [] and ro.select([10, 10], [[80, 64], [63, 80]])[0] == [(0, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the default threshold against what registration accepts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "large"])
def test_default_threshold_keeps_every_active_fixture_pair(name):
    """Every pair section 15 reports as active (the nested triangle and its large variant, the ring on the large maps) has
    at least 64 shared octants under the identity starts and under the true poses; a pair started 3 m away has none."""
    ms = gf.map_set(name)
    tables = [ro.Table.of_map(m) for m in ms.maps]
    pairs = sorted(set(gf.TRIANGLE) | (set(gf.RING) if name == "large" else set()))
    for what, T in (("identity starts", gf.identity_starts()), ("true poses", np.stack(ms.T_true).astype(np.float32))):
        live, blocks, octants = ro.survey(tables, T, ms.maps[0].vs)
        print(f"{name}, {what}: live {live.tolist()}, shared octants {octants.tolist()}")
        assert all(octants[s, d] >= ro.DEFAULT_MIN_SHARED for s, d in pairs), (what, octants)
        sel, comp, res, _ = ro.select(live.tolist(), octants.tolist())
        assert set(pairs) <= set(sel) and res["num_components"] == 1
    far = gf.off_lattice_starts().copy()
    far[2] = gf.FAR
    _, _, octants = ro.survey(tables, far, ms.maps[0].vs)
    assert octants[1, 2] == octants[2, 1] == octants[0, 2] == 0 and octants[0, 1] >= ro.DEFAULT_MIN_SHARED
    if name == "small":
        sphere = ro.Table.of_map(fx.sphere_pair().dst_map)
        _, _, o4 = ro.survey(tables + [sphere], np.concatenate([gf.off_lattice_starts(), gf.FAR[None]]), ms.maps[0].vs)
        assert not o4[:3, 3].any() and not o4[3, :3].any()


# ---------------------------------------------------------------------------------------------------------------------
# the boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_library_selection_equals_the_reference_without_a_device(pkg):
    """dslam_select_register_pairs takes no engine and touches no device: the built library, loaded as test_abi.py loads
    it, gives the reference's pairs, components and counts on every random matrix, writes nothing past `selected`, and
    leaves its outputs alone when it refuses."""
    pkg._share_torch_hip_runtime()
    lib = ctypes.CDLL(pkg.LIB_PATH)
    i32 = ctypes.POINTER(ctypes.c_int32)

    def call(live, shared, params, n=None, null=()):
        live, shared = np.asarray(live, np.int32), np.ascontiguousarray(np.asarray(shared, np.int32))
        pairs, comp, res = np.full((pkg.MAX_REGISTER_PAIRS, 2), -7, np.int32), np.full(len(live), -7, np.int32), pkg.PairSelectResult()
        res.selected = -7
        rc = lib.dslam_select_register_pairs(None if "live" in null else live.ctypes.data_as(i32),
                                             None if "shared" in null else shared.ctypes.data_as(i32),
                                             ctypes.c_int(len(live) if n is None else n),
                                             ctypes.byref(params) if params is not None else None,
                                             None if "pairs" in null else pairs.ctypes.data_as(i32),
                                             None if "component" in null else comp.ctypes.data_as(i32),
                                             None if "result" in null else ctypes.byref(res))
        return rc, pairs, comp, res

    for live, shared, params in of.selection_cases():
        rc, pairs, comp, res = call(live, shared, pkg.PairSelectParams(**params))
        want_pairs, want_comp, want, _ = ro.select(live, shared, **params)
        assert rc == 0 and [tuple(p) for p in pairs[:res.selected].tolist()] == want_pairs and comp.tolist() == want_comp
        assert dict(qualifying=res.qualifying, selected=res.selected, num_components=res.num_components) == want
        assert (pairs[res.selected:] == -7).all()
    live, shared, _ = of.selection_cases()[0]
    rc, pairs, comp, res = call(live, shared, None)                  # NULL params: the defaults
    assert rc == 0 and [tuple(p) for p in pairs[:res.selected].tolist()] == ro.select(live, shared)[0]
    n = len(live)
    refused = [dict(null=(w,)) for w in ("live", "shared", "pairs", "component", "result")]
    refused += [dict(n=1), dict(n=pkg.MAX_RENDER_MAPS + 1)]
    refused += [dict(params=pkg.PairSelectParams(min_shared_octants=-1)), dict(params=pkg.PairSelectParams(one_direction=-1)),
                dict(params=pkg.PairSelectParams(max_pairs=-1)), dict(params=pkg.PairSelectParams(max_pairs=pkg.MAX_REGISTER_PAIRS + 1))]
    for kw in refused:
        rc, pairs, comp, res = call(live, shared, kw.pop("params", None), **kw)
        assert rc == -1 and (pairs == -7).all() and (comp == -7).all() and res.selected == -7, kw
    wide = [8] * 6
    rc, pairs, comp, res = call(wide, np.full((6, 6), 64), pkg.PairSelectParams(max_pairs=4))    # below N - 1
    assert rc == -1 and (pairs == -7).all() and res.selected == -7
    rc, pairs, comp, res = call(wide, np.full((6, 6), 64), pkg.PairSelectParams(max_pairs=5))
    assert rc == 0 and res.selected == 5 and res.qualifying == 30 and res.num_components == 1


def test_header_library_and_wrapper_carry_the_entry_points(pkg):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dslam_fusion.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+dslam_survey_overlaps\s*\(", txt) and re.search(r"\bint\s+dslam_select_register_pairs\s*\(", txt)
    exported = pkg.exported_symbols()
    assert "dslam_survey_overlaps" in exported and "dslam_select_register_pairs" in exported
    assert callable(pkg.CApi.survey_overlaps) and callable(pkg.CApi.select_register_pairs)
    assert ctypes.sizeof(pkg.PairSelectParams) == 16 and ctypes.sizeof(pkg.PairSelectResult) == 16
    assert ro.MAX_REGISTER_PAIRS == pkg.MAX_REGISTER_PAIRS
