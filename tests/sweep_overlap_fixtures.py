"""Shapes shared by the tests of the allocation sweep beside the ray march: 160x120 frames of a moving camera,
a hash table so small that every pass but the first meets occupied buckets (excess requests), and two voxel pools -- one
with room for the whole sequence, one that runs dry in the middle of a pass.  The oracle's run is made once per pool and
never changed: its map state after every frame, and the image of every frame."""
import numpy as np

import util

M = 12                      # frames of a sequence
SIZE = (160, 120)
TABLE = dict(num_buckets=0x400, num_excess=0x1000)
POOLS = {"roomy": 0x800, "dry": 608}

_FRAMES = {}
_ORACLE = {}


def frames(synth, size=SIZE):
    """(workload, [(rgba, mm, M)] for M + 1 frames) of s_tiny at `size`, rendered once."""
    if size not in _FRAMES:
        wl = synth.s_tiny(*size)
        _FRAMES[size] = (wl, [wl.frame(i) for i in range(M + 1)])
    return _FRAMES[size]


def params(pkg, wl, pool, **over):
    return util.small_params(pkg, wl, num_local_blocks=POOLS[pool], **TABLE, **over)


def oracle_run(oracle, pkg, wl, frs, n, prm, free_scale=1, pose_of=None, between=None, only_visible_at=()):
    """n frames of ProcessFrame + GetImage on the oracle: ([image], [snapshot after frame i])."""
    scene = oracle.create_scene(prm)
    rs = oracle.create_render_state(scene, wl.W, wl.H)
    free = oracle.create_render_state(scene, wl.W // free_scale, wl.H // free_scale)
    view = oracle.create_view(wl.W, wl.H)
    free_intr = [v / free_scale for v in wl.intr]
    imgs, snaps = [], []
    for i in range(n):
        if between is not None and i > 0:
            between(oracle, scene, rs, view, i)
        rgba, mm, Mi = frs[i]
        oracle.view_update(view, rgba, mm, timestamp=float(i))
        oracle.process_frame(scene, view, rs, Mi, wl.intr, only_update_visible_list=i in only_visible_at)
        imgs.append(oracle.get_image(scene, free, frs[pose_of(i) if pose_of else i][2], free_intr, pkg.IMAGE_DEPTH))
        snaps.append(util.snapshot(oracle, scene, rs))
    return np.array(imgs), snaps


def oracle_reference(oracle, pkg, synth, pool):
    """The plain sequence on the oracle for `pool`, computed once."""
    if pool not in _ORACLE:
        wl, frs = frames(synth)
        _ORACLE[pool] = oracle_run(oracle, pkg, wl, frs, M, params(pkg, wl, pool))
    return _ORACLE[pool]
