"""The maps the unmerge tests share (test_unmerge_ref.py on the CPU, test_gpu_unmerge.py on the GPU): the analytic pairs of
register_fixtures.py and the planes of weighted_fixtures.py, re-weighted so that a merge does not clamp at max_w."""
import functools

import numpy as np

import analytic_maps as am
import ref_merge as rm
import weighted_fixtures as wf


def uniform(st, w):
    """A copy of `st` whose observed voxels all weigh `w`."""
    out = st.copy()
    out.vba["w_depth"] = np.where(out.vba["w_depth"] > 0, w, 0)
    return out


@functools.lru_cache(maxsize=None)
def unclamped_planes():
    """weighted_fixtures.weighted_planes with the destination's weights folded into 1 .. 90 (the source adds 7 at most: no
    clamp at 100), and the source once more as a destination with weights and colour weights of its own."""
    a, b = wf.weighted_planes()
    src, dst = rm.State.of_map(a), rm.State.of_map(b)
    w = dst.vba["w_depth"].astype(np.int64)
    dst.vba["w_depth"] = np.where(w > 0, 1 + (w - 1) % 90, 0)
    twin = rm.State.of_map(a)
    w, wc = twin.vba["w_depth"].astype(np.int64), twin.vba["w_color"].astype(np.int64)
    lin = np.arange(512)[None, :]
    twin.vba["w_depth"] = np.where(w > 0, 1 + (13 * w + 5 * lin) % 61, 0)
    twin.vba["w_color"] = np.where(wc > 0, 1 + (7 * wc + 3 * lin) % 11, 0)
    return src, dst, twin


def _colour(x):
    return 128.0 + (x - np.array([0.0, 0.0, 0.4])) @ np.array([[300.0, 0.0, 40.0], [0.0, 250.0, -60.0], [60.0, 80.0, 0.0]])


@functools.lru_cache(maxsize=None)
def plane_maps(w_dst=99):
    """test_gpu_merge.py's plane pair: a coloured map of weight 3 and an uncoloured one of weight `w_dst` that overlap in x
    (99: the merge clamps at max_w = 100)."""
    geom = am.Plane((0.1, 0.05, -1.0), -0.40)
    a = am.build_map(geom, am.VS, am.MU, (-0.15, -0.10, 0.2), (0.10, 0.10, 0.62), colour=_colour, w_depth=3)
    b = am.build_map(geom, am.VS, am.MU, (-0.05, -0.10, 0.2), (0.20, 0.10, 0.62), w_depth=w_dst)
    return rm.State.of_map(a), rm.State.of_map(b)
