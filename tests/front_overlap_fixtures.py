"""Shapes shared by the tests of GetImage's front end on the auxiliary stream: those of
sweep_overlap_fixtures.py -- 160x120, 12 frames of s_tiny, the pools "roomy" and "dry" -- but with 0x800 buckets in front of
the 0x1000 excess entries: with 0x400 the bucket heads are nearly all taken after a few frames and the later passes create
excess entries only, while the selection's hidden-entry path has a bucket and an excess case (test_front_overlap_abi.py
shows what this table gives).  And the oracle's run over them with what the front end produces kept per frame: the free-view render state's
visible list, its count and the corner of its range image, next to the image and the map state.  Made once per pool and
never changed."""
import numpy as np

import sweep_overlap_fixtures as fx
import util

M = fx.M
TABLE = dict(num_buckets=0x800, num_excess=0x1000)
_ORACLE = {}


def params(pkg, wl, pool, **over):
    return util.small_params(pkg, wl, num_local_blocks=fx.POOLS[pool], **TABLE, **over)


def corner(api, rs, w, h):
    """The cells of the range image the ray march reads: ceil(w / 8) x ceil(h / 8)."""
    return np.array(api.download_range_image(rs)[:(h + 7) // 8, :(w + 7) // 8])


def oracle_reference(oracle, pkg, synth, pool):
    """Per frame of the plain sequence on the oracle: dict(image, snap, visible, count, corner, hash_before)."""
    if pool not in _ORACLE:
        wl, frs = fx.frames(synth)
        scene = oracle.create_scene(params(pkg, wl, pool))
        rs = oracle.create_render_state(scene, wl.W, wl.H)
        free = oracle.create_render_state(scene, wl.W, wl.H)
        view = oracle.create_view(wl.W, wl.H)
        out = []
        for i in range(M):
            rgba, mm, Mi = frs[i]
            before = oracle.download_hash_table(scene)
            oracle.view_update(view, rgba, mm, timestamp=float(i))
            oracle.process_frame(scene, view, rs, Mi, wl.intr)
            img = oracle.get_image(scene, free, Mi, wl.intr, pkg.IMAGE_DEPTH)
            out.append(dict(image=np.array(img), snap=util.snapshot(oracle, scene, rs), visible=oracle.download_visible_ids(free),
                            count=oracle.stats(scene, free)["no_visible_entries"], corner=corner(oracle, free, wl.W, wl.H),
                            hash_before=before))
        _ORACLE[pool] = out
    return _ORACLE[pool]
