"""The float64 reference of dslam_register_maps (ref64_register.py) on analytic map pairs whose true transform is known:
what it converges to and from how far, what it reports on geometry that does not fix six freedoms, and the plumbing of the
library entry points.  The distances recorded here are the reference's own; the GPU file derives its limits from them, so
each is asserted to be within a factor of two of what the reference measures now."""
import ctypes
import os
import re

import numpy as np
import pytest

import analytic_maps as am
import ref64_register as rr
import register_fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# largest displacement of the source's bounding-box corners between the estimate and the true transform, in voxels
# (Pair.distance), as ref64_register.register reaches it
RECORDED_DISTANCE = {"small": 0.0086, "large": 0.0107, "xl": 0.0089, "truth": 0.0086, "holes": 0.0076}


def _within_factor_two(recorded, now):
    assert recorded / 2 <= now <= recorded * 2, f"recorded {recorded}, the reference now reaches {now:.4g}"


@pytest.mark.parametrize("name", ["small", "large", "xl"])
def test_converges(name):
    pair, X, res = fx.reference_run("box", name)
    assert len(pair.src_map.block_pos) == 268 and 400 <= len(pair.dst_map.block_pos) <= 700
    mrad, vox = pair.difference(X)
    print(f"{name}: start {pair.difference(fx.I4)}, {res['evaluations']} evaluations, end {mrad:.3g} mrad / {vox:.3g} voxel, "
          f"distance {pair.distance(X):.4g} voxel, conditioning {res['conditioning']:.3g}")
    assert res["candidates"] == 25395
    assert res["stop_reason"] == 0 and res["evaluations"] <= 30
    assert res["valid_last"] == res["candidates"]
    assert res["conditioning"] > 0.1
    _within_factor_two(RECORDED_DISTANCE[name], pair.distance(X))
    assert pair.distance(X) < 0.02 * pair.distance(fx.I4)


def test_outside_the_capture_range():
    pair, X, res = fx.reference_run("box", "xxl")
    print(f"xxl: stop {res['stop_reason']} after {res['evaluations']} evaluations, {res['valid_last']} of {res['candidates']} valid, "
          f"conditioning {res['conditioning']:.3g}")
    assert res["stop_reason"] != 0
    assert res["valid_last"] / res["candidates"] < 0.2
    assert res["conditioning"] < 1e-3


def test_starting_at_the_truth_stays_there():
    pair, X, res = fx.reference_run("box", "small", "truth")
    assert res["stop_reason"] == 0
    _within_factor_two(RECORDED_DISTANCE["truth"], pair.distance(X))
    assert pair.distance(X) <= 2 * RECORDED_DISTANCE["small"]


def test_degenerate_sphere():
    pair, X, res = fx.reference_run("sphere")
    assert len(pair.src_map.block_pos) == 341
    c = np.append(np.asarray(fx.SPHERE_CENTRE), 1.0)
    off = np.linalg.norm((np.asarray(X, np.float64) @ c - pair.X_true @ c)[:3]) / am.VS
    print(f"sphere: centre {off:.3g} voxel off after {res['evaluations']} evaluations (stop {res['stop_reason']}), conditioning "
          f"{res['conditioning']:.3g}")
    assert off < 0.05                       # from 2 voxels
    assert res["conditioning"] < 1e-2
    box = fx.reference_run("box", "small")[2]
    assert box["conditioning"] > 40 * res["conditioning"]


def test_degenerate_plane():
    # (8 evaluations: the map has 118 080 candidates, and the figures below do not need the other 22)
    pair, X, res = fx.reference_run("plane", max_evaluations=8)
    print(f"plane: conditioning {res['conditioning']:.3g}, cost {res['cost_first']:.4g} -> {res['cost_last']:.4g}")
    assert res["conditioning"] < 1e-4
    assert res["cost_last"] <= res["cost_first"]
    box = fx.reference_run("box", "small")[2]
    assert box["conditioning"] > 1000 * res["conditioning"]


def test_disjoint_maps():
    pair = fx.box_pair("small")
    X0 = rr.rigid(0.0, fx.AXIS, (3.0, 0.0, 0.0)).astype(np.float32)
    X, res = rr.register(pair.src, pair.dst, X0)
    assert res["stop_reason"] == 3 and res["evaluations"] == 1 and res["valid_last"] == 0 and res["conditioning"] == 0.0
    assert X.tobytes() == X0.tobytes()


def test_holes_and_chains():
    pair, X, res = fx.reference_run("holes")
    assert pair.src_map.max_chain == 8 and pair.src_map.num_buckets == 0x40
    mrad, vox = pair.difference(X)
    print(f"holes: {res['valid_last']} of {res['candidates']} valid, end {mrad:.3g} mrad / {vox:.3g} voxel, distance "
          f"{pair.distance(X):.4g} voxel")
    assert res["stop_reason"] == 0
    assert 0.5 * res["candidates"] < res["valid_last"] < 0.85 * res["candidates"]
    _within_factor_two(RECORDED_DISTANCE["holes"], pair.distance(X))


def test_tie_share_of_the_compared_evaluations():
    """Every evaluation the GPU file compares sum by sum has under 1 % tie voxels."""
    for what, pair, X0 in fx.single_evaluations():
        ev = rr.evaluate(pair.src, pair.dst, rr.voxel_transform(X0, pair.src.vs))
        print(f"{what}: {ev.ties} ties of {ev.candidates} candidates, {ev.valid} valid")
        assert ev.tie_share < 0.01, what
        assert ev.valid > 0.5 * ev.candidates
    for kind, name in (("box", "small"), ("box", "large"), ("box", "xl"), ("holes", None)):
        trace = fx.reference_run(kind, name)[2]["trace"]
        assert all(t["tie_share"] < 0.01 for t in trace[1:]), (kind, name)   # ([0] is the identity: the exact path)


def test_identity_evaluation_of_a_map_with_itself():
    pair = fx.box_pair("small")
    ev = rr.evaluate(pair.src, pair.src, rr.voxel_transform(fx.I4, pair.src.vs))
    assert ev.valid == ev.candidates == 25395   # (the band's voxels lie well inside the map's band of blocks)
    assert ev.sums[27] == 0.0 and not np.any(ev.sums[21:27])


# ---------------------------------------------------------------------------------------------------------------------
# plumbing: these fail without the feature
# ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points(pkg):
    exported = pkg.exported_symbols()
    assert "dslam_register_maps" in exported and "dslam_debug_register_sums" in exported


def test_header_declares_the_entry_points():
    txt = open(os.path.join(ROOT, "include", "dslam_fusion.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+dslam_register_maps\s*\(", txt) and re.search(r"\bint\s+dslam_debug_register_sums\s*\(", txt)
    assert "dslam_register_params" in txt and "dslam_register_result" in txt


def test_python_binding_and_struct_sizes(pkg):
    assert ctypes.sizeof(pkg.RegisterParams) == 24 and ctypes.sizeof(pkg.RegisterResult) == 32
    assert callable(pkg.CApi.register_maps) and callable(pkg.CApi.debug_register_sums)
    assert [n for n, _ in pkg.RegisterResult._fields_] == ["evaluations", "stop_reason", "candidates", "valid_last",
                                                          "cost_first", "cost_last", "conditioning", "pad"]
