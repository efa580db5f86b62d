"""The float64 reference of dslam_register_graph (ref64_register_graph.py) on three analytic maps of one box corner whose
true poses are known: what the joint solve converges to, that one pair is the pairwise reference, the stop reason of a
graph that is not connected, what an inactive pair leaves alone, and the plumbing of the library entry points.  The
figures recorded here are the reference's own; the GPU file derives its limits from them, so each is asserted to be within
a factor of two of what the reference measures now."""
import ctypes
import os
import re

import numpy as np
import pytest

import ref64_register as rr
import ref64_register_graph as rg
import register_fixtures as fx
import register_graph_fixtures as gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# case -> (evaluations, stop reason, conditioning, distances in voxels): for anchor 0 of maps 1 and 2 to their true poses
# (MapSet.distance), for the ring of the pair transforms 0 -> 1 and 0 -> 2 (MapSet.pair_distance)
RECORDED = {"triangle": (6, 0, 0.146, (0.0068, 0.0120)),
            "large": (9, 0, 0.143, (0.0081, 0.0113)),
            "ring": (30, 1, 0.298, (0.0083, 0.0027))}
RING_VALID_LAST = [25395, 33233, 49218, 48474, 33231]


def _within_factor_two(recorded, now):
    assert recorded / 2 <= now <= recorded * 2, f"recorded {recorded}, the reference now reaches {now:.4g}"


def _distances(case, ms, T):
    if gf.CASES[case][2] == 0:
        return ms.distance(T[1], 1), ms.distance(T[2], 2)
    return ms.pair_distance(T, 0, 1), ms.pair_distance(T, 0, 2)


@pytest.mark.parametrize("case", ["triangle", "large", "ring"])
def test_converges(case):
    ms, T, res = gf.reference_run(case)
    evaluations, stop, cond, dist = RECORDED[case]
    now = _distances(case, ms, T)
    print(f"{case}: {[len(m.block_pos) for m in ms.maps]} blocks, {res['evaluations']} evaluations, stop {res['stop_reason']}, "
          f"conditioning {res['conditioning']:.3g}, cost {res['cost_first']:.4g} -> {res['cost_last']:.4g}, distances "
          f"{now[0]:.4g} / {now[1]:.4g} voxel; valid {[p['valid_last'] for p in res['pairs']]}")
    assert len(ms.maps[0].block_pos) == 268
    assert res["evaluations"] == evaluations and res["stop_reason"] == stop
    assert res["active_pairs"] == len(gf.CASES[case][1])
    _within_factor_two(cond, res["conditioning"])
    for recorded, d in zip(dist, now):
        _within_factor_two(recorded, d)
    assert T[gf.CASES[case][2]].tobytes() == gf.I4.tobytes()          # the anchor is never written
    if case == "ring":
        assert [p["valid_last"] for p in res["pairs"]] == RING_VALID_LAST
        assert abs(res["cost_last"] - 0.139) < 0.001 and res["cost_last"] < res["cost_first"]
    else:
        assert all(p["valid_last"] == p["candidates"] for p in res["pairs"])
        assert [p["candidates"] for p in res["pairs"]][:2] == [25395, 25395]
        assert res["pairs"][2]["candidates"] == (48636 if case == "triangle" else 49218)
        # the joint solve is no worse than a chain of pairwise ones would leave the far map (0.0145 voxel, prototype)
        assert now[1] < 0.0145 or case != "triangle"


def test_one_pair_is_the_pairwise_reference():
    """Two maps, the pair (0, 1), anchor 0, T_0 the identity: X~ = T~_1 exactly and the run is register(src 0, dst 1)."""
    ms = gf.map_set("small")
    X, pw = rr.register(ms.data[0], ms.data[1], fx.I4)
    T, res = rg.register_graph(ms.data[:2], gf.identity_starts(2), [(0, 1)], 0)
    assert T[1].tobytes() == X.tobytes() and T[0].tobytes() == fx.I4.tobytes()
    assert res["evaluations"] == pw["evaluations"] and res["stop_reason"] == pw["stop_reason"] == 0
    assert res["pairs"][0]["valid_last"] == pw["valid_last"] and res["pairs"][0]["candidates"] == pw["candidates"]
    assert res["cost_first"] == pw["cost_first"] and res["cost_last"] == pw["cost_last"]
    assert abs(res["conditioning"] - pw["conditioning"]) <= 1e-9 * pw["conditioning"]
    # ... and from a start that is not the identity
    start = gf.identity_starts(2)
    start[1] = fx.off_lattice()
    X, pw = rr.register(ms.data[0], ms.data[1], start[1], max_evaluations=4)
    T, res = rg.register_graph(ms.data[:2], start, [(0, 1)], 0, max_evaluations=4)
    assert T[1].tobytes() == X.tobytes() and res["evaluations"] == pw["evaluations"] == 4 and res["stop_reason"] == 1


def test_a_graph_that_is_not_connected_stops_with_reason_3():
    ms = gf.map_set("small")
    start = gf.off_lattice_starts()
    T, res = rg.register_graph(ms.data, start, [(0, 1)], 0)
    assert res["stop_reason"] == 3 and res["evaluations"] == 1 and res["conditioning"] == 0.0
    assert T.tobytes() == start.tobytes()
    assert res["active_pairs"] == 1 and res["cost_last"] == res["cost_first"]
    # connected on paper, but the pair that reaches map 2 is not active
    far = start.copy()
    far[2] = rr.rigid(0.0, fx.AXIS, (3.0, 0.0, 0.0)).astype(np.float32)
    T, res = rg.register_graph(ms.data, far, [(0, 1), (1, 2)], 0)
    assert res["stop_reason"] == 3 and T.tobytes() == far.tobytes()
    assert [p["active"] for p in res["pairs"]] == [1, 0] and res["pairs"][1]["valid_first"] == 0


def test_an_inactive_pair_changes_nothing():
    """Map 0 against register_fixtures.sphere_pair()'s destination, started 3 m away (at the identity the two surfaces
    still share 8934 voxels within the gate): the pair is reported and then left out of the cost, and no pose moves on
    its account."""
    ms = gf.map_set("small")
    maps = ms.data + [fx.sphere_pair().dst]
    start = np.concatenate([gf.off_lattice_starts(), gf.FAR[None]])
    T_with, with_ = rg.register_graph(maps, start, gf.TRIANGLE + [(0, 3)], 0)
    T_without, without = rg.register_graph(maps, start, gf.TRIANGLE, 0)
    sphere = with_["pairs"][3]
    assert sphere["active"] == 0 and sphere["valid_first"] == 0 and sphere["valid_last"] == 0 and sphere["candidates"] == 25395
    assert abs(sphere["cost_first"] - 0.5625) < 1e-12 and sphere["cost_last"] == sphere["cost_first"]
    assert with_["active_pairs"] == without["active_pairs"] == 3
    # (map 3 is in no active pair, so neither call may take a step: stop reason 3)
    assert with_["stop_reason"] == without["stop_reason"] == 3
    assert T_with.tobytes() == T_without.tobytes() == start.tobytes()
    for key in ("evaluations", "cost_first", "cost_last", "conditioning"):
        assert with_[key] == without[key], key
    # the cost is that of the three maps alone: the fourth map and its pair are in nothing
    _, three = rg.register_graph(ms.data, start[:3], gf.TRIANGLE, 0, max_evaluations=1)
    assert with_["cost_first"] == three["cost_first"]


def test_an_inactive_pair_between_connected_maps_changes_nothing():
    """min_valid = 30000 makes (0, 1), whose source has 25395 candidates, inactive while (1, 0) and (1, 2) connect all
    maps to anchor 1: the run is the one without (0, 1), step for step."""
    name, pairs, anchor, params = gf.INACTIVE_BETWEEN
    ms = gf.map_set(name)
    T_with, with_ = rg.register_graph(ms.data, gf.identity_starts(), pairs, anchor, **params)
    T_without, without = rg.register_graph(ms.data, gf.identity_starts(), pairs[1:], anchor, **params)
    print(f"valid at the start {[p['valid_first'] for p in with_['pairs']]}, {with_['evaluations']} evaluations, stop "
          f"{with_['stop_reason']}, cost {with_['cost_first']:.4g} -> {with_['cost_last']:.4g}")
    assert [p["active"] for p in with_["pairs"]] == [0, 1, 1] and with_["pairs"][0]["valid_first"] == 25395
    assert with_["pairs"][0]["valid_last"] == 25395 and with_["pairs"][0]["cost_last"] == with_["pairs"][0]["cost_first"]
    assert with_["evaluations"] == params["max_evaluations"] and with_["cost_last"] < with_["cost_first"]
    assert T_with.tobytes() == T_without.tobytes() and T_with[anchor].tobytes() == gf.I4.tobytes()
    assert T_with[0].tobytes() != gf.I4.tobytes() and T_with[2].tobytes() != gf.I4.tobytes()
    for key in ("evaluations", "stop_reason", "active_pairs", "cost_first", "cost_last", "conditioning"):
        assert with_[key] == without[key], key


def test_tie_share_of_the_compared_evaluations():
    """Every evaluation the GPU file compares sum by sum has under 1 % tie voxels."""
    ms = gf.map_set("small")
    T, res = rg.register_graph(ms.data, gf.off_lattice_starts(), gf.TRIANGLE, 0, max_evaluations=1)
    for p, ev in res["first"].evs.items():
        print(f"pair {gf.TRIANGLE[p]}: {ev.ties} ties of {ev.candidates} candidates, {ev.valid} valid")
        assert ev.tie_share < 0.01 and ev.valid > 0.5 * ev.candidates
    assert res["stop_reason"] == 1 and T.tobytes() == gf.off_lattice_starts().tobytes()
    for case in ("triangle", "large", "ring"):
        trace = gf.reference_run(case)[2]["trace"]
        assert all(ev.tie_share < 0.01 for t in trace[1:] for ev in t["je"].evs.values()), case
    # the work-split evaluations
    big = fx.sphere_pair().dst
    X = rr.voxel_transform(fx.off_lattice(1.5, 0.45), big.vs)
    assert rr.evaluate(big, big, X).tie_share < 0.01
    few = rr.MapData.of_map(gf.few_map())
    assert rr.evaluate(few, fx.box_pair("small").dst, rr.voxel_transform(fx.off_lattice(), few.vs)).tie_share < 0.01


def test_rigid_arithmetic_is_the_mirrors():
    """inv and product in the stated scalar order agree with numpy's to rounding, and the identity source gives X~ = T~_d
    exactly."""
    Ta = rr.voxel_transform(fx.true_transform("large"), 0.005)
    Tb = rr.voxel_transform(rr.rigid(-25e-3, gf.AXIS2, 0.02 * gf.DIR2, fx.BOX_CENTRE), 0.005)
    full = lambda X: np.vstack([X, [0, 0, 0, 1]])
    assert np.allclose(rg.rigid_inverse(Ta), np.linalg.inv(full(Ta))[:3], rtol=0, atol=1e-12)
    assert np.allclose(rg.rigid_product(Tb, rg.rigid_inverse(Ta)), (full(Tb) @ np.linalg.inv(full(Ta)))[:3], rtol=0, atol=1e-12)
    eye = np.eye(4)[:3]
    assert np.array_equal(rg.pair_transform(np.stack([eye, Tb]), 0, 1), Tb)


# ---------------------------------------------------------------------------------------------------------------------
# plumbing: these fail without the feature
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points(pkg):
    exported = pkg.exported_symbols()
    assert "dslam_register_graph" in exported and "dslam_debug_register_graph_sums" in exported


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+dslam_register_graph\s*\(", txt) and re.search(r"\bint\s+dslam_debug_register_graph_sums\s*\(", txt)
    assert "dslam_register_graph_result" in txt and "dslam_register_pair_result" in txt
    assert re.search(r"#define\s+DSLAM_MAX_REGISTER_PAIRS\s+128\b", txt)


def test_python_binding_and_struct_sizes(pkg):
    assert ctypes.sizeof(pkg.RegisterGraphResult) == 24 and ctypes.sizeof(pkg.RegisterPairResult) == 24
    assert callable(pkg.CApi.register_graph) and callable(pkg.CApi.debug_register_graph_sums)
    assert [n for n, _ in pkg.RegisterGraphResult._fields_] == ["evaluations", "stop_reason", "active_pairs", "cost_first",
                                                               "cost_last", "conditioning"]
    assert [n for n, _ in pkg.RegisterPairResult._fields_] == ["candidates", "valid_first", "valid_last", "active",
                                                              "cost_first", "cost_last"]
    assert pkg.MAX_REGISTER_PAIRS == 128
